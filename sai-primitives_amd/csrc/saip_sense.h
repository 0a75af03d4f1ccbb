// The sensing model of the resident simulator (saip_sense.hip): what stands between the simulated robot and what the controller reads of
// it -- a constant offset, additive Gaussian noise and quantisation on every joint position and velocity and on the sensed wrench of up to
// SENSE_MAX_WRENCH_TASKS motion-force tasks.  The per-element arithmetic, shared by the kernels and by host-compiled checks (plain C++ when
// no HIP compiler is reading it, like saip_plant.h).
//
// A measured value is
//   m = x + off
//   if (sigma > 0) m = m + sigma z          z a standard normal
//   if (res   > 0) m = res rint(m / res)    round half to even
// A joint is SENSE_JOINT_WORDS words: q_off, q_res, q_sigma, dq_off, dq_res, dq_sigma; a wrench axis is SENSE_AXIS_WORDS words: off, res,
// sigma, six axes per task (goal rows 30..35).  The neutral row is all zeros: x + 0.0 is x for every x that is not -0.0, a NaN stays NaN.
//
// The normals are samp_normals of saip_sampler.h at counter (instance, row, table id << 16, period) under the 64-bit seed: table
// SENSE_TABLE_JOINT_NOISE, row j gives (z of q_j, z of dq_j); table SENSE_TABLE_WRENCH_NOISE, row 3 slot + a / 2 gives the z of axes a
// (even) and a + 1 of the task in slot `slot`.  Noise is a pure function of (seed, instance, row, period): nothing here is state.
//
// Every function below rounds each product and each sum on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/sensing_ref.py) reproduces the noise-free arithmetic bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_plant.h"
#include "saip_sampler.h"

#if defined(__HIPCC__)
#define SAIP_SE_HD __host__ __device__
#else
#define SAIP_SE_HD
#endif

namespace saip {

enum { SENSE_JOINT_WORDS = 6, SENSE_AXIS_WORDS = 3, SENSE_WRENCH_WORDS = 18, SENSE_MAX_WRENCH_TASKS = 2, SENSE_WRENCH_ROW0 = 30 };
enum { SENSE_Q_OFF = 0, SENSE_Q_RES, SENSE_Q_SIGMA, SENSE_DQ_OFF, SENSE_DQ_RES, SENSE_DQ_SIGMA };
enum { SENSE_OFF = 0, SENSE_RES, SENSE_SIGMA };
// the table id inside the random-number counter: 0..3 are the plant's and the inertia table's
enum { SENSE_TABLE_JOINTS = 4, SENSE_TABLE_WRENCHES = 5, SENSE_TABLE_JOINT_NOISE = 6, SENSE_TABLE_WRENCH_NOISE = 7 };
enum { SENSE_MODE_JOINTS = 1, SENSE_MODE_WRENCH = 2 };

SAIP_SE_HD inline double se_measure(double x, double off, double res, double sigma, double z) {
#pragma clang fp contract(off)
	double m = x + off;
	if (sigma > 0.0) m = m + sigma * z;
	if (res > 0.0) m = res * rint(m / res);
	return m;
}

// The two normals of row `row` of table `table` for instance i in period `period`; skipped (zeros) when neither sigma is positive: the
// measured values are the same.
SAIP_SE_HD inline void se_normals(uint32_t seed_lo, uint32_t seed_hi, uint32_t period, int table, int i, int row, double sigma0, double sigma1, double z[2]) {
	z[0] = z[1] = 0.0;
	if (sigma0 > 0.0 || sigma1 > 0.0) samp_normals(seed_lo, seed_hi, period, table, i, row, 0, z);
}

// One joint of one instance.  Word k of the joint is w[k * stride]: a batch-uniform table [n][6] has stride 1, a per-instance table
// [n][6][ld] has stride ld (w already points at the joint's first word in the instance's column).
SAIP_SE_HD inline void se_joint(const double* w, long long stride, uint32_t seed_lo, uint32_t seed_hi, uint32_t period, int i, int j, double q, double dq,
								 double* q_meas, double* dq_meas) {
	const double qs = w[SENSE_Q_SIGMA * stride], ds = w[SENSE_DQ_SIGMA * stride];
	double z[2];
	se_normals(seed_lo, seed_hi, period, SENSE_TABLE_JOINT_NOISE, i, j, qs, ds, z);
	*q_meas = se_measure(q, w[SENSE_Q_OFF * stride], w[SENSE_Q_RES * stride], qs, z[0]);
	*dq_meas = se_measure(dq, w[SENSE_DQ_OFF * stride], w[SENSE_DQ_RES * stride], ds, z[1]);
}

// Axes 2 pair and 2 pair + 1 of the wrench of slot `slot` of one instance, in place: w points at the slot's first word in the instance's
// column ([6][3] words, stride as above), f0 and f1 at the two goal rows.
SAIP_SE_HD inline void se_wrench_pair(const double* w, long long stride, uint32_t seed_lo, uint32_t seed_hi, uint32_t period, int i, int slot, int pair, double* f0,
									   double* f1) {
	const double* w0 = w + (long long)(2 * pair) * SENSE_AXIS_WORDS * stride;
	const double* w1 = w0 + (long long)SENSE_AXIS_WORDS * stride;
	const double s0 = w0[SENSE_SIGMA * stride], s1 = w1[SENSE_SIGMA * stride];
	double z[2];
	se_normals(seed_lo, seed_hi, period, SENSE_TABLE_WRENCH_NOISE, i, 3 * slot + pair, s0, s1, z);
	*f0 = se_measure(*f0, w0[SENSE_OFF * stride], w0[SENSE_RES * stride], s0, z[0]);
	*f1 = se_measure(*f1, w1[SENSE_OFF * stride], w1[SENSE_RES * stride], s1, z[1]);
}

// The random draw of word `word` of a per-instance table (joint j word k is 6 j + k, slot s axis a word e is 18 s + 3 a + e): pl_draw of
// saip_plant.h under the sensing tables' ids.
SAIP_SE_HD inline double se_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int table, int i, int word, double lo, double hi) {
	return pl_draw(seed_lo, seed_hi, round, table, i, word, lo, hi, false);
}

// one launch of saip_sense_apply.  Passed to the kernel by value.
struct SenseParams {
	int B, ld, n, mode;          // mode: SENSE_MODE_* bits
	int per_instance_joints, per_instance_wrenches;
	int n_slots, slot_mask;      // wrench slots attached; bit s: slot s is perturbed by this launch (its sensor has just been simulated)
	uint32_t seed_lo, seed_hi, period, pad_;
	const double* q;             // [n][ld] the true state: read only
	const double* dq;
	const double* joints;        // [n][6] or [n][6][ld]
	double* q_meas;              // [n][ld]
	double* dq_meas;
	const double* wrenches;      // [slots][6][3] or [slots][6][3][ld]
	double* goal[SENSE_MAX_WRENCH_TASKS];  // the goal block of the slot's task, [goal_comps][ld]: rows 30..35 in place
};
#if defined(__HIPCC__)
// Row `row` >= n of a sensing launch for instance b (b < B): one axis pair of the sensed wrench of one slot's task, goal rows 30..35 in
// place.  Shared by saip_sense_apply and saip_sense_chain_apply (saip_sense_chain.hip), so that a rollout period keeps one measurement launch.
__device__ inline void se_wrench_rows(const SenseParams& P, int row, int b) {
	const size_t ld = P.ld;
	const int r = row - P.n, slot = r / 3, pair = r % 3;
	if (!(P.mode & SENSE_MODE_WRENCH) || slot >= P.n_slots || !((P.slot_mask >> slot) & 1)) return;
	const long long ws = P.per_instance_wrenches ? (long long)ld : 1, wc = P.per_instance_wrenches ? (long long)b : 0;
	double* g = (slot == 0 ? P.goal[0] : P.goal[1]) + (size_t)(SENSE_WRENCH_ROW0 + 2 * pair) * ld + b;
	double f0 = g[0], f1 = g[ld];
	se_wrench_pair(P.wrenches + (long long)slot * SENSE_WRENCH_WORDS * ws + wc, ws, P.seed_lo, P.seed_hi, P.period, b, slot, pair, &f0, &f1);
	g[0] = f0;
	g[ld] = f1;
}
#endif
// one launch of saip_sense_randomize: either table may be left alone (null)
struct SenseRandomParams {
	int B, ld, n, n_slots;
	uint32_t seed_lo, seed_hi, round, pad_;
	double* joints;              // [n][6][ld] or null
	const double* joint_lo;      // [n][6], device
	const double* joint_hi;
	double* wrenches;            // [slots][18][ld] or null
	const double* wrench_lo;     // [slots][18], device
	const double* wrench_hi;
};

}  // namespace saip
