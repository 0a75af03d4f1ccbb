// Resident guards (saip_guard.hip): event-triggered phases of a rollout.  Every instance carries a phase 0 .. P-1; a table of G guards
// (transitions) says when it leaves a phase for another, a table of P phases what a phase does to the goal of one motion-force task.
// What one lane decides in one evaluation -- the signals from their inputs, the transition, the goal rows -- is here, shared by the kernel
// and by host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_sense_chain.h).  The pose is an input: the
// forward-kinematics walk stays in the kernel.
//
// A guard is GUARD_WORDS doubles { from, to, signal, axis, cmp, threshold, hold, blank }, a phase GUARD_PHASE_WORDS doubles
// { mode, dx, dy, dz }.  One evaluation of one instance:
//   p = phase; fired = -1
//   for g = 0 .. G-1:  if from[g] != p or since < blank[g]: run[g] = 0
//                      else: run[g] = cond(g) ? run[g] + 1 : 0;  if fired < 0 and run[g] >= hold[g]: fired = g
//   if fired >= 0:     fires[fired] += 1; phase = to[fired]; since = 0; every run[g] = 0
//                      if entry[phase] < 0: entry[phase] = clock;  latch[0..11] = the pose of this evaluation
//   else:              since += 1
//   HOLD / OFFSET:     goal rows 0..11 = latch (position + (dx, dy, dz) for OFFSET), rows 12..23 = 0.0;  FREE writes nothing
//   clock += 1
// cond(g) is signal >= threshold (cmp 0) or signal <= threshold (cmp 1); a NaN signal satisfies neither.  Integers only, but for the
// signals; no atomics: the instance owns its column of every array.
//
// Every product and sum is rounded on its own (no contraction into FMAs), in the order written, so a NumPy restatement
// (tests/guard_ref.py) reproduces an evaluation bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

// always_inline: the callee is inlined before it is optimised on its own, so the caller's GuardSignals and pose are split into registers
// with everything else (on the device: no scratch).
#if defined(__HIPCC__)
#define SAIP_GD_HD __host__ __device__ __attribute__((always_inline))
#else
#define SAIP_GD_HD __attribute__((always_inline))
#endif

namespace saip {

enum { GUARD_MAX_PHASES = 8, GUARD_MAX_GUARDS = 8, GUARD_WORDS = 8, GUARD_PHASE_WORDS = 4, GUARD_READOUT_ROWS = 8, GUARD_LATCH_ROWS = 12 };
enum { GUARD_FROM = 0, GUARD_TO, GUARD_SIGNAL, GUARD_AXIS, GUARD_CMP, GUARD_THRESHOLD, GUARD_HOLD, GUARD_BLANK };
enum { GUARD_SIGNAL_PERIODS = 0, GUARD_SIGNAL_FORCE, GUARD_SIGNAL_MOMENT, GUARD_SIGNAL_POSITION, GUARD_SIGNAL_POS_ERROR, GUARD_SIGNAL_ORI_ERROR,
	   GUARD_SIGNAL_JOINT_SPEED, GUARD_SIGNAL_COUNT };
enum { GUARD_CMP_GE = 0, GUARD_CMP_LE = 1 };
enum { GUARD_MODE_FREE = 0, GUARD_MODE_HOLD, GUARD_MODE_OFFSET, GUARD_MODE_COUNT };
// rows of the readout: what the last launch saw (a row it did not need holds NaN)
enum { GUARD_READ_FORCE = 0, GUARD_READ_MOMENT, GUARD_READ_POS_ERROR, GUARD_READ_ORI_ERROR, GUARD_READ_JOINT_SPEED, GUARD_READ_POSITION };
// what a launch has to compute (batch-uniform, decided on the host from the two tables)
enum { GUARD_NEED_FK = 1, GUARD_NEED_ERROR = 2, GUARD_NEED_FORCE = 4, GUARD_NEED_MOMENT = 8, GUARD_NEED_SPEED = 16 };

// sqrt((e0 e0 + e1 e1) + e2 e2): the arithmetic of the recorder's summaries (rec_norm2, then sqrt)
SAIP_GD_HD inline double gd_norm3(const double* e) {
#pragma clang fp contract(off)
	return sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

// the inputs of the signals for one instance; what the launch did not need is NaN
struct GuardSignals {
	double f[3], m[3];   // goal rows 30..32 and 33..35: the sensed force and moment in the sensor frame
	double pos[3];       // world position of the control point
	double ep, eo;       // norms of the selection-projected position / orientation error
	double speed;        // max_j |dq_j|
};

SAIP_GD_HD inline double gd_signal(int signal, int axis, int since, const GuardSignals& S) {
	switch (signal) {
		case GUARD_SIGNAL_PERIODS: return (double)since;
		case GUARD_SIGNAL_FORCE: return axis == 0 ? S.f[0] : axis == 1 ? S.f[1] : axis == 2 ? S.f[2] : gd_norm3(S.f);
		case GUARD_SIGNAL_MOMENT: return axis == 0 ? S.m[0] : axis == 1 ? S.m[1] : axis == 2 ? S.m[2] : gd_norm3(S.m);
		// (the last alternative is a value, as in the two lines above, not a third member: a select between members only is rewritten as a load at a
		// selected offset, which keeps S in memory)
		case GUARD_SIGNAL_POSITION: return axis == 0 ? S.pos[0] : axis == 1 ? S.pos[1] : axis == 2 ? S.pos[2] : NAN;
		case GUARD_SIGNAL_POS_ERROR: return S.ep;
		case GUARD_SIGNAL_ORI_ERROR: return S.eo;
		case GUARD_SIGNAL_JOINT_SPEED: return S.speed;
	}
	return NAN;  // an unknown signal (a table written through the device pointer) never fires
}

// One evaluation of one instance.  Word k of guard g is guards[(g * GUARD_WORDS + k) * gstride] (gstride: ld for a per-instance table whose
// pointer is already at the instance's column, 1 for a batch-uniform one); phases is [P][4], batch-uniform.  Element r of a state array is
// a[r * ss], of the goal block goal[r * gs]: ss and gs are the distances between two rows of one instance's column (ld on the device).
// pose: position 3, rotation 9 row-major; have_pose false: the launch computed none, and the latch keeps what it has.  run[] and fires[]
// are read and written in their rows: no per-lane array is indexed at run time.
SAIP_GD_HD inline void gd_step(const double* guards, long long gstride, int G, const double* phases, int P, const GuardSignals& S, const double* pose, bool have_pose,
								int* phase, int* since, int* clock, int* run, int* entry, int* fires, double* latch, long long ss, double* goal, long long gs) {
#pragma clang fp contract(off)
	const int p = *phase, sn = *since;
	int fired = -1, to = 0;
#pragma unroll
	for (int g = 0; g < GUARD_MAX_GUARDS; g++) {
		if (g >= G) continue;
		const double* w = guards + (long long)g * GUARD_WORDS * gstride;
		int r = 0;
		if (w[GUARD_FROM * gstride] == (double)p && !((double)sn < w[GUARD_BLANK * gstride])) {
			const double s = gd_signal((int)w[GUARD_SIGNAL * gstride], (int)w[GUARD_AXIS * gstride], sn, S), thr = w[GUARD_THRESHOLD * gstride];
			const bool c = w[GUARD_CMP * gstride] == (double)GUARD_CMP_LE ? s <= thr : s >= thr;  // (a NaN signal: false either way)
			r = c ? run[g * ss] + 1 : 0;
			if (fired < 0 && (double)r >= w[GUARD_HOLD * gstride]) {
				fired = g;
				const double t = w[GUARD_TO * gstride];
				to = t >= 1.0 ? (t < (double)P ? (int)t : P - 1) : 0;  // a table written through the device pointer cannot index past the phases
			}
		}
		run[g * ss] = r;
	}
	int now = p;
	if (fired >= 0) {
		fires[fired * ss] += 1;
		now = to;
		*phase = now;
		*since = 0;
#pragma unroll
		for (int g = 0; g < GUARD_MAX_GUARDS; g++)
			if (g < G) run[g * ss] = 0;
		if (entry[now * ss] < 0) entry[now * ss] = *clock;
		if (have_pose) {
#pragma unroll
			for (int e = 0; e < GUARD_LATCH_ROWS; e++) latch[e * ss] = pose[e];
		}
	} else {
		*since = sn + 1;
	}
	const double* ph = phases + (now >= 0 && now < P ? now : 0) * GUARD_PHASE_WORDS;
	const double mode = ph[0];
	if (mode == (double)GUARD_MODE_HOLD || mode == (double)GUARD_MODE_OFFSET) {
		const bool off = mode == (double)GUARD_MODE_OFFSET;
		for (int e = 0; e < 3; e++) goal[e * gs] = off ? latch[e * ss] + ph[1 + e] : latch[e * ss];
		for (int e = 3; e < GUARD_LATCH_ROWS; e++) goal[e * gs] = latch[e * ss];
		for (int e = 12; e < 24; e++) goal[e * gs] = 0.0;
	}
	*clock += 1;
}

// cost[i] + (entry >= 0 ? w_time * (double)entry : w_miss): saip_batch_guard_add_cost on the sampler's per-instance cost
SAIP_GD_HD inline double gd_cost(double cost, int entry, double w_time, double w_miss) {
#pragma clang fp contract(off)
	return cost + (entry >= 0 ? w_time * (double)entry : w_miss);
}

struct ModelDev;
struct TaskDev;
// one launch of saip_guard_apply.  Passed to the kernel by value.
struct GuardParams {
	int B, ld, n, task;
	int G, P, per_instance, need;    // need: GUARD_NEED_* bits
	const ModelDev* model;
	const TaskDev* tasks;
	const double* q;                 // what the controller reads: the measured copy while a sensing model is attached
	const double* dq;
	const double* guards;            // [G][8] or [G][8][ld]
	const double* phases;            // [P][4]
	double* goal;                    // the task's user goal block [36][ld]
	int *phase, *since, *clock;      // [ld] each
	int *run, *entry, *fires;        // [G][ld], [P][ld], [G][ld]
	double* latch;                   // [12][ld]
	double* readout;                 // [8][ld]
};

}  // namespace saip
