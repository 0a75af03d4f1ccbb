// The clearance monitor of the resident simulator (saip_clearance.hip): the per-instance arithmetic, shared by the kernel and by
// host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_contact.h and saip_sampler.h).
//
// S link spheres (centre c_s = o_body + R_body r_s, radius r_s) against O world-fixed obstacles and P self pairs.  An obstacle is eight words
// { kind, a[3], b[3], r }: kind 0 a capsule (the segment a-b with radius r; a == b is a sphere), kind 1 a half-space (a the unit normal,
// b[0] the offset).  Items are numbered k = s O + o for sphere x obstacle, then S O + p for pair p: N = S O + P items, each with a signed
// distance dist_k (negative: penetration).  Item k contributes pen_k = max(0, margin - dist_k)^2, under_k = dist_k < margin and a
// candidate (dist_k, k) for the minimum.
//
// The work split is part of the definition: CLEARANCE_LANES = 8 lanes evaluate an instance, lane l takes items l, l + 8, ... in ascending
// order and keeps a ClearancePartial; the eight partials fold as v[l] (+)= v[l + off] for off = 4, 2, 1 (cl_fold).  The host runs the
// eight lanes one after the other and folds in the same shape (cl_evaluate_host), so the sums round in the same order.
//
// Every function below rounds each product and each sum on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/clearance_ref.py) reproduces it bit for bit; sqrt and the division are correctly rounded on the host and on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAIP_CL_HD __host__ __device__
#else
#define SAIP_CL_HD
#endif

namespace saip {

enum { CLEARANCE_MAX_SPHERES = 32, CLEARANCE_MAX_OBSTACLES = 16, CLEARANCE_MAX_PAIRS = 64, CLEARANCE_OBSTACLE_WORDS = 8,
	   CLEARANCE_READOUT_ROWS = 8, CLEARANCE_SUMMARY_ROWS = 4, CLEARANCE_LANES = 8, CLEARANCE_GROUPS = 8 };
enum { CLEARANCE_EVALUATE = 0, CLEARANCE_MONITOR = 1 };
enum { CLEARANCE_CAPSULE = 0, CLEARANCE_HALF_SPACE = 1 };

// The sphere centres of the CLEARANCE_GROUPS instances of one block, component e of sphere s of instance (group) g.  The same index serves
// the host build (one instance: g = 0).  Why this shape: see phase 2 of saip_clearance.hip.
enum { CLEARANCE_CENTRE_PLANE = CLEARANCE_MAX_SPHERES * CLEARANCE_GROUPS, CLEARANCE_CENTRE_WORDS = 3 * CLEARANCE_CENTRE_PLANE };
SAIP_CL_HD inline int cl_centre_index(int s, int e, int g) { return e * CLEARANCE_CENTRE_PLANE + (s >> 3) * 64 + (g >> 2) * 32 + (g & 3) * 8 + (s & 7); }

// The geometry of an attachment that does not depend on the instance, as the device keeps it.  The spheres are SORTED by body (spheres on
// the fixed base, body -1, first): position i of the sorted list is the caller's sphere slot[i].  `radius` and `pair` speak of the
// caller's sphere indices, as the item numbers do.
struct ClearanceGeom {
	int S, O, P, pad_;
	int body[CLEARANCE_MAX_SPHERES];           // sorted
	int slot[CLEARANCE_MAX_SPHERES];           // sorted position -> sphere index
	double r[CLEARANCE_MAX_SPHERES][3];        // sorted: the centre in the body frame
	double radius[CLEARANCE_MAX_SPHERES];      // by sphere index
	uint8_t pair[CLEARANCE_MAX_PAIRS][2];      // sphere indices
};

SAIP_CL_HD inline bool cl_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN

// a . b = ((a0 b0 + a1 b1) + a2 b2)
SAIP_CL_HD inline double cl_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
	return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// c = o + R r of a row-major 3 x 3, rows summed left to right (as ct_mat_vec of saip_contact.h)
SAIP_CL_HD inline void cl_centre(const double* o, const double* R, const double* r, double* c) {
#pragma clang fp contract(off)
	for (int i = 0; i < 3; i++) c[i] = o[i] + ((R[3 * i] * r[0] + R[3 * i + 1] * r[1]) + R[3 * i + 2] * r[2]);
}
// sphere (centre c, radius rs) against the capsule a-b of radius ro
SAIP_CL_HD inline double cl_capsule_dist(const double* a, const double* b, double ro, const double* c, double rs) {
#pragma clang fp contract(off)
	double e[3], w[3], u[3];
	for (int i = 0; i < 3; i++) {
		e[i] = b[i] - a[i];
		w[i] = c[i] - a[i];
	}
	const double L2 = cl_dot(e, e);
	const double t = L2 > 0.0 ? fmin(fmax(cl_dot(w, e) / L2, 0.0), 1.0) : 0.0;
	for (int i = 0; i < 3; i++) u[i] = w[i] - t * e[i];
	return sqrt(cl_dot(u, u)) - (rs + ro);
}
// ... against the half-space n . x >= o
SAIP_CL_HD inline double cl_half_space_dist(const double* n, double o, const double* c, double rs) {
#pragma clang fp contract(off)
	return (cl_dot(n, c) - o) - rs;
}
// two spheres
SAIP_CL_HD inline double cl_pair_dist(const double* c1, double r1, const double* c2, double r2) {
#pragma clang fp contract(off)
	double u[3];
	for (int i = 0; i < 3; i++) u[i] = c1[i] - c2[i];
	return sqrt(cl_dot(u, u)) - (r1 + r2);
}

// what one lane keeps, and what the fold leaves in lane 0
struct ClearancePartial {
	double pen;      // sum of pen_k
	double dmin;     // smallest dist_k (+inf: no item) ...
	double pmin;     // ... over the pair items only
	int k;           // item of dmin (-1: no item); the lowest k among equals
	int under;       // items with dist_k < margin
	int bad;         // a sphere centre of this lane's share is not finite
};

// The obstacles of one instance.  Word w of obstacle o is obst[(o * CLEARANCE_OBSTACLE_WORDS + w) * stride + col]: a batch-uniform table
// [O][8] has stride 1 and col 0, a per-instance table [O][8][ld] has stride ld and col = the instance.  C: the centres (cl_centre_index),
// g: the instance's group.  Lane `lane` takes items lane, lane + 8, ... and the finiteness test of spheres lane, lane + 8, ...
SAIP_CL_HD inline void cl_lane(const ClearanceGeom& G, const double* obst, long long stride, long long col, double margin, const double* C, int g,
								int lane, ClearancePartial* out) {
#pragma clang fp contract(off)
	ClearancePartial v = {0.0, INFINITY, INFINITY, -1, 0, 0};
	for (int s = lane; s < G.S; s += CLEARANCE_LANES)
		for (int e = 0; e < 3; e++)
			if (!cl_finite(C[cl_centre_index(s, e, g)])) v.bad = 1;  // explicit: fmax and the comparisons below drop NaNs
	const int SO = G.S * G.O, N = SO + G.P;
	for (int k = lane; k < N; k += CLEARANCE_LANES) {
		double d;
		if (k < SO) {
			const int s = k / G.O, o = k - s * G.O;
			const double c[3] = {C[cl_centre_index(s, 0, g)], C[cl_centre_index(s, 1, g)], C[cl_centre_index(s, 2, g)]};
			const double* w = obst + (long long)o * CLEARANCE_OBSTACLE_WORDS * stride + col;
			const double a[3] = {w[stride], w[2 * stride], w[3 * stride]};
			if (w[0] == (double)CLEARANCE_HALF_SPACE) {
				d = cl_half_space_dist(a, w[4 * stride], c, G.radius[s]);
			} else {
				const double b[3] = {w[4 * stride], w[5 * stride], w[6 * stride]};
				d = cl_capsule_dist(a, b, w[7 * stride], c, G.radius[s]);
			}
		} else {
			const int s1 = G.pair[k - SO][0], s2 = G.pair[k - SO][1];
			const double c1[3] = {C[cl_centre_index(s1, 0, g)], C[cl_centre_index(s1, 1, g)], C[cl_centre_index(s1, 2, g)]};
			const double c2[3] = {C[cl_centre_index(s2, 0, g)], C[cl_centre_index(s2, 1, g)], C[cl_centre_index(s2, 2, g)]};
			d = cl_pair_dist(c1, G.radius[s1], c2, G.radius[s2]);
			if (d < v.pmin) v.pmin = d;
		}
		const double m = fmax(0.0, margin - d);
		v.pen = v.pen + m * m;
		if (d < margin) v.under++;
		if (d < v.dmin) {  // strict: the lowest k wins within a lane
			v.dmin = d;
			v.k = k;
		}
	}
	*out = v;
}
// v (+)= w: + for the sums; the partner's minimum if its distance is smaller, or equal with a smaller k
SAIP_CL_HD inline void cl_fold(ClearancePartial* v, const ClearancePartial& w) {
#pragma clang fp contract(off)
	v->pen = v->pen + w.pen;
	v->under = v->under + w.under;
	v->bad = v->bad | w.bad;
	if (w.dmin < v->dmin || (w.dmin == v->dmin && w.k < v->k)) {
		v->dmin = w.dmin;
		v->k = w.k;
	}
	if (w.pmin < v->pmin) v->pmin = w.pmin;
}
// the readout of one instance from the folded partial: dmin, k, penalty, items under the margin, the centre of the (first) sphere of
// item k, the smallest self-pair distance.  An instance with a centre that is not finite is invalid: NaN, k = -1, count 0.
SAIP_CL_HD inline void cl_readout(const ClearanceGeom& G, const ClearancePartial& v, const double* C, int g, double* ro) {
	const bool bad = v.bad != 0;
	const int k = bad ? -1 : v.k;
	ro[0] = bad ? (double)NAN : v.dmin;
	ro[1] = (double)k;
	ro[2] = bad ? (double)NAN : v.pen;
	ro[3] = bad ? 0.0 : (double)v.under;
	const int SO = G.S * G.O;
	const int s = k < 0 ? -1 : (k < SO ? k / G.O : (int)G.pair[k - SO][0]);
	for (int e = 0; e < 3; e++) ro[4 + e] = s < 0 ? (double)NAN : C[cl_centre_index(s, e, g)];
	ro[7] = bad ? (double)NAN : v.pmin;
}
// The running summaries of one instance after one monitored period of length dt (s: its column, rows ld apart): the minimum of dmin (NaN is
// sticky), sum dt penalty, periods with dmin < 0, the index of the first such period (-1: none yet).
SAIP_CL_HD inline void cl_summary_advance(double* s, long long ld, double dt, double dmin, double penalty, double period) {
#pragma clang fp contract(off)
	const double m = s[0];
	s[0] = (m != m || dmin != dmin) ? (double)NAN : (dmin < m ? dmin : m);
	s[ld] = s[ld] + dt * penalty;
	const bool hit = dmin < 0.0;
	s[2 * ld] = s[2 * ld] + (hit ? 1.0 : 0.0);
	if (hit && s[3 * ld] < 0.0) s[3 * ld] = period;
}
// cost + (w_penalty S1 + (S0 < d_safe ? w_collision : 0)); a NaN S0 gives a NaN cost
SAIP_CL_HD inline double cl_add_cost(double cost, double S0, double S1, double w_penalty, double w_collision, double d_safe) {
#pragma clang fp contract(off)
	if (S0 != S0) return (double)NAN;
	return cost + (w_penalty * S1 + (S0 < d_safe ? w_collision : 0.0));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the host form of one instance: the eight lanes one after the other, then the fold in the shape of the kernel's
inline void cl_evaluate_host(const ClearanceGeom& G, const double* obst, long long stride, long long col, double margin, const double* C, double* ro) {
	ClearancePartial v[CLEARANCE_LANES];
	for (int l = 0; l < CLEARANCE_LANES; l++) cl_lane(G, obst, stride, col, margin, C, 0, l, &v[l]);
	for (int off = CLEARANCE_LANES / 2; off >= 1; off >>= 1)
		for (int l = 0; l < off; l++) cl_fold(&v[l], v[l + off]);
	cl_readout(G, v[0], C, 0, ro);
}
#endif

// one launch of saip_clearance_eval.  Passed to the kernel by value.
struct ModelDev;
struct ClearanceParams {
	int B, ld, n, mode;          // mode: CLEARANCE_EVALUATE or CLEARANCE_MONITOR
	int per_instance, pad_;
	double dt;                   // MONITOR: the length of the period (weight of summary row 1)
	double period;               // MONITOR: index of the period, counted from the last reset
	double margin;
	const ModelDev* model;
	const ClearanceGeom* geom;
	const double* q;             // [n][ld]
	const double* obst;          // [O][8] or [O][8][ld]
	double* readout;             // [8][ld]
	double* summary;             // MONITOR: [4][ld]
	double* centres;             // [3 S][ld], or nullptr
};

}  // namespace saip
