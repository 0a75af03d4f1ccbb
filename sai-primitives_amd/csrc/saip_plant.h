// The plant model of the resident simulator (saip_plant.hip): what stands between the commanded torques and the integrator when the robot
// is not the controller's model -- actuator gain, offset and saturation, viscous and Coulomb friction, penalty joint stops and up to
// PLANT_MAX_WRENCHES external wrenches on links.  The per-instance arithmetic, shared by the kernels and by host-compiled checks (plain C++
// when no HIP compiler is reading it, like saip_contact.h).
//
// A joint is PLANT_JOINT_WORDS words: gain, bias, tau_max, fv, fc, v_s, q_lo, q_hi, k_stop, c_stop.  With t the commanded torque:
//   u0 = (t == t) ? t : 0                 a NaN torque is no torque, as the integrator coasts
//   u1 = gain u0 + bias
//   u2 = min(max(u1, -tau_max), tau_max)
//   fr = fv dq + (fc > 0 ? (fc dq) / max(|dq|, v_s) : 0)
//   st = q < q_lo ?  max(0, k_stop (q_lo - q) - c_stop dq) : q > q_hi ? -max(0, k_stop (q - q_hi) + c_stop dq) : 0
//   tau_act = (u2 - fr) + st
// A wrench is PLANT_WRENCH_WORDS words: F (3), M (3), p_start, p_end; it acts in period p when p_start <= p < p_end.
//
// Every function below rounds each product and each sum on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/plant_ref.py) reproduces it bit for bit.  max and min are spelled as comparisons (pl_max, pl_min: the first argument
// wins a tie), not fmax / fmin, whose result for (+0, -0) is the library's choice: the sign of a clipped zero is the same everywhere.
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_sampler.h"

#if defined(__HIPCC__)
#define SAIP_PL_HD __host__ __device__
#else
#define SAIP_PL_HD
#endif

namespace saip {

enum { PLANT_JOINT_WORDS = 10, PLANT_WRENCH_WORDS = 8, PLANT_MAX_WRENCHES = 4, PLANT_SUMMARY_ROWS = 4 };
enum { PLANT_GAIN = 0, PLANT_BIAS, PLANT_TAU_MAX, PLANT_FV, PLANT_FC, PLANT_VS, PLANT_Q_LO, PLANT_Q_HI, PLANT_K_STOP, PLANT_C_STOP };
enum { PLANT_FRAME_WORLD = 0, PLANT_FRAME_LINK = 1 };
enum { PLANT_TABLE_JOINTS = 0, PLANT_TABLE_WRENCHES = 1 };  // the table id inside the random-number counter

// a < b ? b : a and b < a ? b : a: max and min of two numbers, the first argument on a tie (and whenever a comparison with a NaN fails)
SAIP_PL_HD inline double pl_max(double a, double b) { return a < b ? b : a; }
SAIP_PL_HD inline double pl_min(double a, double b) { return b < a ? b : a; }

struct PlantJointOut {
	double tau;    // (u2 - fr) + st
	double fr;     // friction torque (opposes dq)
	double st;     // joint-stop torque
	double clip;   // |u1 - u2|
};

// One joint of one instance.  Word k of the joint is w[k * stride]: a batch-uniform table [n][10] has stride 1, a per-instance table
// [n][10][ld] has stride ld (w already points at the joint's first word in the instance's column).
SAIP_PL_HD inline void pl_joint(const double* w, long long stride, double t, double q, double dq, PlantJointOut* out) {
#pragma clang fp contract(off)
	const double gain = w[PLANT_GAIN * stride], bias = w[PLANT_BIAS * stride], tau_max = w[PLANT_TAU_MAX * stride];
	const double fv = w[PLANT_FV * stride], fc = w[PLANT_FC * stride], vs = w[PLANT_VS * stride];
	const double q_lo = w[PLANT_Q_LO * stride], q_hi = w[PLANT_Q_HI * stride], ks = w[PLANT_K_STOP * stride], cs = w[PLANT_C_STOP * stride];
	const double u0 = t == t ? t : 0.0;
	const double u1 = gain * u0 + bias;
	const double u2 = pl_min(pl_max(u1, -tau_max), tau_max);
	double fr = fv * dq;
	if (fc > 0.0) fr = fr + (fc * dq) / pl_max(fabs(dq), vs);
	else fr = fr + 0.0;
	double st = 0.0;
	if (q < q_lo) st = pl_max(0.0, ks * (q_lo - q) - cs * dq);
	else if (q > q_hi) st = -pl_max(0.0, ks * (q - q_hi) + cs * dq);
	out->tau = (u2 - fr) + st;
	out->fr = fr;
	out->st = st;
	out->clip = fabs(u1 - u2);
}

// what the joint loop of one substep folds, in ascending joint order: sum |fr dq|, the largest clip, whether anything clipped or a stop acted
struct PlantFold {
	double work_fr, clip_max;
	int acted;
};
SAIP_PL_HD inline void pl_fold_init(PlantFold* f) {
	f->work_fr = 0.0;
	f->clip_max = 0.0;
	f->acted = 0;
}
SAIP_PL_HD inline void pl_fold_joint(PlantFold* f, const PlantJointOut& o, double dq) {
#pragma clang fp contract(off)
	f->work_fr = f->work_fr + fabs(o.fr * dq);
	f->clip_max = pl_max(f->clip_max, o.clip);
	if (o.clip > 0.0 || o.st != 0.0) f->acted = 1;
}

// does the wrench whose first word (of the instance's column) is w act in period p?
SAIP_PL_HD inline bool pl_wrench_acts(const double* w, long long stride, long long period) {
	const double p = (double)period;
	return w[6 * stride] <= p && p < w[7 * stride];
}
// F and M of the wrench in the world frame: as stored (PLANT_FRAME_WORLD) or rotated by the link's world rotation Rl, row-major, every row
// summed left to right (PLANT_FRAME_LINK)
SAIP_PL_HD inline void pl_wrench_world(const double* w, long long stride, int frame, const double* Rl, double* F, double* M) {
#pragma clang fp contract(off)
	const double f[3] = {w[0], w[stride], w[2 * stride]}, m[3] = {w[3 * stride], w[4 * stride], w[5 * stride]};
	for (int i = 0; i < 3; i++) {
		if (frame == PLANT_FRAME_LINK) {
			F[i] = (Rl[3 * i] * f[0] + Rl[3 * i + 1] * f[1]) + Rl[3 * i + 2] * f[2];
			M[i] = (Rl[3 * i] * m[0] + Rl[3 * i + 1] * m[1]) + Rl[3 * i + 2] * m[2];
		} else {
			F[i] = f[i];
			M[i] = m[i];
		}
	}
}
// the column of J^T [F; M] of one ancestor joint: aw the joint's world axis, oj its origin, p the application point; revolute
// aw . ((p - oj) x F + M), prismatic aw . F
SAIP_PL_HD inline double pl_wrench_torque(bool revolute, const double* aw, const double* oj, const double* p, const double* F, const double* M) {
#pragma clang fp contract(off)
	if (!revolute) return (aw[0] * F[0] + aw[1] * F[1]) + aw[2] * F[2];
	double r[3], m[3];
	for (int e = 0; e < 3; e++) r[e] = p[e] - oj[e];
	m[0] = (r[1] * F[2] - r[2] * F[1]) + M[0];
	m[1] = (r[2] * F[0] - r[0] * F[2]) + M[1];
	m[2] = (r[0] * F[1] - r[1] * F[0]) + M[2];
	return (aw[0] * m[0] + aw[1] * m[1]) + aw[2] * m[2];
}

// work_ext + x dq: one rounded product, one rounded sum
SAIP_PL_HD inline double pl_work_add(double work_ext, double x, double dq) {
#pragma clang fp contract(off)
	return work_ext + x * dq;
}

// The running summaries of one instance after one substep of length dt (s: its column, rows ld apart): sum dt sum_j |fr_j dq_j|, the largest
// clipped torque so far, substeps in which a joint clipped or a stop acted, sum dt sum ext dq.  work_ext is the sum of x dq_j over the
// acting wrenches in table order and, inside a wrench, over the ancestor joints in ascending order, x being what that wrench added to joint j.
SAIP_PL_HD inline void pl_summary_advance(double* s, long long ld, double dt, const PlantFold& f, double work_ext) {
#pragma clang fp contract(off)
	s[0] = s[0] + dt * f.work_fr;
	s[ld] = pl_max(s[ld], f.clip_max);
	s[2 * ld] = s[2 * ld] + (f.acted ? 1.0 : 0.0);
	s[3 * ld] = s[3 * ld] + dt * work_ext;
}

// The random draw of word `word` (its index inside the whole table: joint j word k is 10 j + k, wrench k word e is 8 k + e) of instance i:
// lo + u (hi - lo), u the first uniform of Philox counter (i, word, table id, round) under the 64-bit seed; lo == hi gives lo exactly (nothing is
// drawn, so an infinite bound stays what it is); window words (p_start, p_end) are floored.
SAIP_PL_HD inline double pl_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int table, int i, int word, double lo, double hi, bool floored) {
#pragma clang fp contract(off)
	double v = lo;
	if (!(lo == hi)) {
		const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)word, (uint32_t)table, round}, key[2] = {seed_lo, seed_hi};
		uint32_t x[4];
		samp_philox4x32_10(ctr, key, x);
		const double u = samp_uniform(x[0], x[1]);
		v = lo + u * (hi - lo);
		// the three roundings can leave the interval by an ulp: the draw stays inside [min(lo, hi), max(lo, hi)]
		v = pl_min(pl_max(v, lo < hi ? lo : hi), lo < hi ? hi : lo);
	}
	return floored ? floor(v) : v;
}

// one launch of saip_plant_apply.  Passed to the kernel by value.
struct ModelDev;
struct PlantSite {
	int body, frame;             // movable body the link is attached to (-1: the fixed base, the wrench moves nothing); PLANT_FRAME_*
	double pos[3], rot[9];       // the application point and the link frame, in the body frame
};
struct PlantParams {
	int B, ld, n, n_wrenches;
	int per_instance_joints, per_instance_wrenches;
	long long period;            // the period this substep belongs to (wrench windows)
	double dt;                   // length of the substep (weight of summary rows 0 and 3)
	const ModelDev* model;
	const double* q;             // [n][ld]
	const double* dq;            // [n][ld]
	const double* tau_cmd;       // [n][ld] commanded torques (NaN = none)
	const double* joints;        // [n][10] or [n][10][ld]
	const double* wrenches;      // [W][8] or [W][8][ld]
	double* tau_act;             // [n][ld]
	double* summary;             // [4][ld]
	PlantSite site[PLANT_MAX_WRENCHES];
};
// one launch of saip_plant_randomize: either table may be left alone (null)
struct PlantRandomParams {
	int B, ld, n, n_wrenches;
	uint32_t seed_lo, seed_hi, round, pad_;
	double* joints;              // [n][10][ld] or null
	const double* joint_lo;      // [n][10], device
	const double* joint_hi;
	double* wrenches;            // [W][8][ld] or null
	const double* wrench_lo;     // [W][8], device
	const double* wrench_hi;
};

}  // namespace saip
