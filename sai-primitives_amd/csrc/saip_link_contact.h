// Link contact of the resident simulator (saip_link_contact.hip): world-fixed obstacles push back on the robot's link spheres.  The
// per-instance arithmetic, shared by the kernel and by host-compiled checks (plain C++ when no HIP compiler is reading it, like
// saip_clearance.h and saip_plant.h).
//
// S link spheres (centre c_s = o_body + R_body r_s, radius r_s, velocity v_s = (tv + tw x c_s) - tc from the twist accumulators of
// SAIP_FK_TWIST_STEP at the sphere's body; a sphere on the fixed base has tv = tw = tc = 0) against O obstacles in the clearance monitor's
// eight words { kind, a[3], b[3], r } (saip_clearance.h), obstacle o with the material { k, c, mu, v_s } = mat[4 o ..].  Item (s, o):
//   half-space   n = a, d = cl_half_space_dist
//   capsule      u = w - t e and len = sqrt(u.u) as cl_capsule_dist forms them, d = len - (r_s + r_o), n = u / len.  With len == 0 (the
//                centre exactly on the axis) there is no direction: the item is inactive and pushes nothing, though its d counts for the
//                smallest distance.  That is a stated limit, not worked around.
//   active iff d < 0 (and len != 0).  Then vn = n.v, f_n = max(0, (-k d) - c vn), v_t = v - vn n,
//   f_t = -(mu f_n) v_t / max(|v_t|, v_s) (zero when mu == 0), f = f_n n + f_t.
// F_s = sum of f over the active obstacles in ascending order, from (0, 0, 0), acting at the sphere's centre.  Joint j gets
//   x_j = sum over the SORTED spheres (ascending sorted position) with an active item whose body joint j moves of
//         aw_j . ((c_s - o_j) x F_s) (revolute) or aw_j . F_s (prismatic), from 0.0; any other joint type adds nothing,
//   tau_sim[j] = u0_j + x_j, u0_j = tau_cmd[j] or 0 when that is NaN.  An instance with no active item, or with a sphere centre that is not
// finite (an invalid instance), gets tau_sim = u0.
//
// The work split is part of the definition: LINK_CONTACT_LANES = 8 lanes serve an instance, lane l owns sorted positions l, l + 8, ... with
// all of their obstacles and keeps a LinkContactPartial over them in that order; the eight partials fold as v[l] (+)= v[l + off] for
// off = 4, 2, 1 (lc_fold).  The host runs the eight lanes one after the other and folds in the same shape (lc_evaluate_host).
//
// Every function below rounds each product and each sum on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/link_contact_ref.py) reproduces it bit for bit; sqrt and the division are correctly rounded on the host and on the
// device.  max is a comparison whose first argument wins a tie (lc_max, as pl_max of saip_plant.h and for its reason).
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_clearance.h"
#include "saip_contact.h"

#if defined(__HIPCC__)
#define SAIP_LC_HD __host__ __device__
#else
#define SAIP_LC_HD
#endif

namespace saip {

enum { LINK_CONTACT_MAX_SPHERES = CLEARANCE_MAX_SPHERES, LINK_CONTACT_MAX_OBSTACLES = CLEARANCE_MAX_OBSTACLES, LINK_CONTACT_OBSTACLE_WORDS = CLEARANCE_OBSTACLE_WORDS,
	   LINK_CONTACT_MATERIAL_WORDS = 4, LINK_CONTACT_READOUT_ROWS = 8, LINK_CONTACT_SUMMARY_ROWS = 4, LINK_CONTACT_LANES = CLEARANCE_LANES,
	   LINK_CONTACT_GROUPS = CLEARANCE_GROUPS, LINK_CONTACT_MAX_JOINTS = 32 };
enum { LINK_CONTACT_EVALUATE = 0, LINK_CONTACT_APPLY = 1 };
// a vector per sorted sphere (or per joint) of the eight instances of one block: cl_centre_index, whose bank reasoning (saip_clearance.hip)
// holds for lanes that read positions l, l + 8, ... and for lanes that all read the same position
enum { LINK_CONTACT_VEC_WORDS = CLEARANCE_CENTRE_WORDS, LINK_CONTACT_FLAG_WORDS = CLEARANCE_CENTRE_PLANE };
SAIP_LC_HD inline int lc_flag_index(int i, int g) { return (i >> 3) * 64 + g * 8 + (i & 7); }

// The geometry of an attachment, batch-uniform, as the device keeps it.  The spheres are SORTED by body (spheres on the fixed base, body -1,
// first): position i of the sorted list is the caller's sphere slot[i]; every array below but `owner` is indexed by sorted position.
struct LinkContactGeom {
	int S, O, jmax, pad_;                       // jmax: the largest body (-1: every sphere sits on the base)
	int body[LINK_CONTACT_MAX_SPHERES];
	int slot[LINK_CONTACT_MAX_SPHERES];
	uint32_t anc[LINK_CONTACT_MAX_SPHERES];     // bit j set: joint j moves the sphere's body (chain: j <= body; tree: the body's ancestor mask)
	int owner[LINK_CONTACT_MAX_JOINTS];         // joint -> the lowest sorted position it moves (-1: it moves no sphere): the walk that stores it
	double r[LINK_CONTACT_MAX_SPHERES][3];      // the centre in the body frame
	double radius[LINK_CONTACT_MAX_SPHERES];
};

SAIP_LC_HD inline double lc_max(double a, double b) { return a < b ? b : a; }

struct LinkContactItem {
	double d;        // signed distance (negative: penetration)
	double f[3];     // force on the sphere, world frame (0 when inactive)
	double fn;       // normal force magnitude (0 when inactive)
	int active;
};
// One item.  w: the obstacle's first word (of the instance's column), words `stride` apart; m: its material { k, c, mu, v_s }.
SAIP_LC_HD inline void lc_item(const double* w, long long stride, const double* m, const double* c, const double* v, double rs, LinkContactItem* out) {
#pragma clang fp contract(off)
	const double a[3] = {w[stride], w[2 * stride], w[3 * stride]};
	double n[3] = {0.0, 0.0, 0.0}, d;
	bool dir = true;
	if (w[0] == (double)CLEARANCE_HALF_SPACE) {
		d = cl_half_space_dist(a, w[4 * stride], c, rs);
		for (int i = 0; i < 3; i++) n[i] = a[i];
	} else {
		const double b[3] = {w[4 * stride], w[5 * stride], w[6 * stride]};
		d = cl_capsule_dist(a, b, w[7 * stride], c, rs);
		if (d < 0.0) {
			// the direction: u and len once more, the operations of cl_capsule_dist in its order
			double e[3], x[3], u[3];
			for (int i = 0; i < 3; i++) {
				e[i] = b[i] - a[i];
				x[i] = c[i] - a[i];
			}
			const double L2 = cl_dot(e, e);
			const double t = L2 > 0.0 ? fmin(fmax(cl_dot(x, e) / L2, 0.0), 1.0) : 0.0;
			for (int i = 0; i < 3; i++) u[i] = x[i] - t * e[i];
			const double len = sqrt(cl_dot(u, u));
			dir = len != 0.0;
			if (dir)
				for (int i = 0; i < 3; i++) n[i] = u[i] / len;
		}
	}
	out->d = d;
	out->active = (d < 0.0 && dir) ? 1 : 0;
	out->fn = 0.0;
	for (int i = 0; i < 3; i++) out->f[i] = 0.0;
	if (!out->active) return;
	const double k = m[0], cd = m[1], mu = m[2], vs = m[3];
	const double vn = cl_dot(n, v);
	const double fn = lc_max(0.0, (-k * d) - cd * vn);
	double vt[3];
	for (int i = 0; i < 3; i++) vt[i] = v[i] - vn * n[i];
	const double s = lc_max(sqrt(cl_dot(vt, vt)), vs);
	const double g = mu * fn;
	for (int i = 0; i < 3; i++) {
		const double ft = mu == 0.0 ? 0.0 : -(g * vt[i]) / s;
		out->f[i] = fn * n[i] + ft;
	}
	out->fn = fn;
}

// what one lane keeps, and what the fold leaves in lane 0
struct LinkContactPartial {
	double f[3];     // sum of F_s over the lane's spheres
	double dmin;     // smallest d (+inf: no item) ...
	double fn_sum;   // sum of f_n
	double fmax;     // largest single-item |f|
	int k;           // item s O + o of dmin in the caller's sphere numbering (-1: no item); the lowest k among equals
	int active;      // active items
	int bad;         // a sphere centre of this lane's share is not finite
};

// what the lanes read of one instance: the tables (word w of obstacle o at obst[(8 o + w) stride + col]: [O][8] has stride 1 and col 0,
// [O][8][ld] has stride ld and col = the instance; the kernel's staged copy has stride 8 and col = the group) and the per-sphere constants
struct LinkContactView {
	int S, O;
	const int* slot;
	const double* radius;
	const double* obst;
	long long stride, col;
	const double* mat;       // [O][4]
};

// Sorted sphere i (centre c, velocity v) against the obstacles in ascending order: F_s accumulates in Fs (from what the caller put
// there), the lane's partial p takes minimum, sum f_n and largest |f|; returns the number of active items
SAIP_LC_HD inline int lc_sphere_items(const LinkContactView& W, int i, const double* c, const double* v, LinkContactPartial& p, double* Fs) {
#pragma clang fp contract(off)
	int act = 0;
	for (int o = 0; o < W.O; o++) {
		LinkContactItem it;
		lc_item(W.obst + (long long)o * LINK_CONTACT_OBSTACLE_WORDS * W.stride + W.col, W.stride, W.mat + LINK_CONTACT_MATERIAL_WORDS * o, c, v, W.radius[i], &it);
		const int k = W.slot[i] * W.O + o;
		if (it.d < p.dmin || (it.d == p.dmin && k < p.k)) {  // (a lane does not meet its items in ascending k: the tie is explicit)
			p.dmin = it.d;
			p.k = k;
		}
		if (!it.active) continue;
		act++;
		for (int e = 0; e < 3; e++) Fs[e] = Fs[e] + it.f[e];
		p.fn_sum = p.fn_sum + it.fn;
		p.fmax = lc_max(p.fmax, sqrt(cl_dot(it.f, it.f)));
	}
	return act;
}
// Lane `lane` of the instance in group g: C, V the centres and velocities (cl_centre_index by sorted position), F and A receive F_s
// (cl_centre_index) and the flag "has an active item" (lc_flag_index) of the lane's spheres.
SAIP_LC_HD inline void lc_lane(const LinkContactView& W, const double* C, const double* V, double* F, int* A, int g, int lane, LinkContactPartial* out) {
#pragma clang fp contract(off)
	LinkContactPartial p = {{0.0, 0.0, 0.0}, INFINITY, 0.0, 0.0, -1, 0, 0};
	for (int i = lane; i < W.S; i += LINK_CONTACT_LANES) {
		const double c[3] = {C[cl_centre_index(i, 0, g)], C[cl_centre_index(i, 1, g)], C[cl_centre_index(i, 2, g)]};
		const double v[3] = {V[cl_centre_index(i, 0, g)], V[cl_centre_index(i, 1, g)], V[cl_centre_index(i, 2, g)]};
		for (int e = 0; e < 3; e++)
			if (!cl_finite(c[e])) p.bad = 1;  // explicit: the comparisons below drop NaNs
		double Fs[3] = {0.0, 0.0, 0.0};
		const int act = lc_sphere_items(W, i, c, v, p, Fs);
		for (int e = 0; e < 3; e++) {
			F[cl_centre_index(i, e, g)] = Fs[e];
			p.f[e] = p.f[e] + Fs[e];
		}
		A[lc_flag_index(i, g)] = act > 0 ? 1 : 0;
		p.active += act;
	}
	*out = p;
}
// v (+)= w: + for the sums, the larger |f|, the partner's minimum if its distance is smaller, or equal with a smaller k
SAIP_LC_HD inline void lc_fold(LinkContactPartial* v, const LinkContactPartial& w) {
#pragma clang fp contract(off)
	for (int e = 0; e < 3; e++) v->f[e] = v->f[e] + w.f[e];
	v->fn_sum = v->fn_sum + w.fn_sum;
	v->fmax = lc_max(v->fmax, w.fmax);
	v->active = v->active + w.active;
	v->bad = v->bad | w.bad;
	if (w.dmin < v->dmin || (w.dmin == v->dmin && w.k < v->k)) {
		v->dmin = w.dmin;
		v->k = w.k;
	}
}
// the readout of one instance from the folded partial: net force 3, smallest d, its item, active items, sum f_n, largest |f|.  An invalid
// instance: NaN in the distance and force rows, item -1, count 0.
SAIP_LC_HD inline void lc_readout(const LinkContactPartial& v, double* ro) {
	const bool bad = v.bad != 0;
	for (int e = 0; e < 3; e++) ro[e] = bad ? (double)NAN : v.f[e];
	ro[3] = bad ? (double)NAN : v.dmin;
	ro[4] = bad ? -1.0 : (double)v.k;
	ro[5] = bad ? 0.0 : (double)v.active;
	ro[6] = bad ? (double)NAN : v.fn_sum;
	ro[7] = bad ? (double)NAN : v.fmax;
}
// The running summaries of one instance after one APPLY substep of length dt (s: its column, rows ld apart; ro: that substep's readout):
// sum dt sum f_n (NaN is sticky: an invalid substep adds NaN), the largest single-item |f|, the largest penetration max(0, -d), substeps
// with an active item.  An invalid substep leaves rows 1 - 3 as they are (every comparison with a NaN fails).
SAIP_LC_HD inline void lc_summary_advance(double* s, long long ld, double dt, const double* ro) {
#pragma clang fp contract(off)
	s[0] = s[0] + dt * ro[6];
	s[ld] = lc_max(s[ld], ro[7]);
	s[2 * ld] = lc_max(s[2 * ld], lc_max(0.0, -ro[3]));
	s[3 * ld] = s[3 * ld] + (ro[5] > 0.0 ? 1.0 : 0.0);
}
// cost + (w_impulse S0 + w_peak S1); a NaN S0 gives a NaN cost
SAIP_LC_HD inline double lc_add_cost(double cost, double S0, double S1, double w_impulse, double w_peak) {
#pragma clang fp contract(off)
	if (S0 != S0) return (double)NAN;
	return cost + (w_impulse * S0 + w_peak * S1);
}
// x_j of joint j (type jtype: 1 revolute, 2 prismatic; world axis aw, origin oj) over the sorted spheres: anc, C, F, A as above
SAIP_LC_HD inline double lc_joint_sum(int S, const uint32_t* anc, int j, int jtype, const double* aw, const double* oj, const double* C, const double* F,
									   const int* A, int g) {
#pragma clang fp contract(off)
	double x = 0.0;
	if (jtype != 1 && jtype != 2) return x;
	for (int i = 0; i < S; i++) {
		if (!((anc[i] >> j) & 1u) || !A[lc_flag_index(i, g)]) continue;
		const double c[3] = {C[cl_centre_index(i, 0, g)], C[cl_centre_index(i, 1, g)], C[cl_centre_index(i, 2, g)]};
		const double f[3] = {F[cl_centre_index(i, 0, g)], F[cl_centre_index(i, 1, g)], F[cl_centre_index(i, 2, g)]};
		x = x + ct_joint_torque(jtype == 1, aw, oj, c, f);
	}
	return x;
}
// u0 of a commanded torque: a NaN torque is no torque, as contact APPLY has it
SAIP_LC_HD inline double lc_u0(double t) { return t == t ? t : 0.0; }
// tau_sim[j] = u0_j + x_j, one rounded sum
SAIP_LC_HD inline double lc_tau(double u0, double x) {
#pragma clang fp contract(off)
	return u0 + x;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host form of one instance: the eight lanes one after the other, then the fold in the shape of the kernel's.  C, V, F: LINK_CONTACT_VEC_WORDS
// doubles, A: LINK_CONTACT_FLAG_WORDS ints (group 0).  Returns whether the torque loop runs: a valid instance with an active item.
inline bool lc_evaluate_host(const LinkContactView& W, const double* C, const double* V, double* F, int* A, double* ro) {
	LinkContactPartial v[LINK_CONTACT_LANES];
	for (int l = 0; l < LINK_CONTACT_LANES; l++) lc_lane(W, C, V, F, A, 0, l, &v[l]);
	for (int off = LINK_CONTACT_LANES / 2; off >= 1; off >>= 1)
		for (int l = 0; l < off; l++) lc_fold(&v[l], v[l + off]);
	lc_readout(v[0], ro);
	return !v[0].bad && v[0].active > 0;
}
#endif

// one launch of saip_link_contact_apply.  Passed to the kernel by value.
struct ModelDev;
struct LinkContactParams {
	int B, ld, n, mode;          // mode: LINK_CONTACT_EVALUATE or LINK_CONTACT_APPLY
	int per_instance, S, O, pad_;  // S, O: those of *geom
	double dt;                   // APPLY: length of the substep (weight of summary row 0)
	const ModelDev* model;
	const LinkContactGeom* geom;
	const double* q;             // [n][ld]
	const double* dq;            // [n][ld]
	const double* obst;          // [O][8] or [O][8][ld]
	const double* mat;           // [O][4]
	const double* tau_cmd;       // APPLY: [n][ld] commanded torques (NaN = none)
	double* tau_sim;             // APPLY: [n][ld]
	double* readout;             // [8][ld]
	double* summary;             // APPLY: [4][ld]
	double* keep;                // [9 S][ld] centres, velocities, F_s in the caller's sphere numbering, or nullptr
};

}  // namespace saip
