// Rigid-body kinematics and dynamics of one robot instance (serial chain; the *_tree variants below for kinematic trees) in world coordinates, one lane per instance: forward kinematics,
// recursive Newton-Euler and the composite-rigid-body mass matrix.  Shared by the forward-dynamics step (saip_dynamics.hip) and the
// joint-space model queries (saip_model_query.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "saip_device.h"

namespace saip {

namespace {

struct V3 {
	double x, y, z;
};
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 mulR(const double* R, V3 v) {
	return V3{R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
__device__ __forceinline__ V3 mulRt(const double* R, V3 v) {
	return V3{R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z};
}

// Where a body's inertial parameters come from.  ModelInertials: the batch-uniform model (what every kernel reads but the INERTIA
// instantiations of the integrator).  TableInertials: the lane's column of the resident inertia table (saip_inertia.h) -- word k of body j is
// w[(10 j + k) stride].  `in` is a name in the scope of every traversal below, beside md.
struct ModelInertials {
	__device__ __forceinline__ double mass(const ModelDev& md, int j) const { return md.mass[j]; }
	__device__ __forceinline__ double com(const ModelDev& md, int j, int e) const { return md.com[j][e]; }
	__device__ __forceinline__ const double* inertia(const ModelDev& md, int j, double*) const { return md.inertia[j]; }
};
struct TableInertials {
	const double* w;
	long long stride;
	__device__ __forceinline__ double mass(const ModelDev&, int j) const { return w[(long long)j * 10 * stride]; }
	__device__ __forceinline__ double com(const ModelDev&, int j, int e) const { return w[((long long)j * 10 + 1 + e) * stride]; }
	__device__ __forceinline__ const double* inertia(const ModelDev&, int j, double* I6) const {
		for (int e = 0; e < 6; e++) I6[e] = w[((long long)j * 10 + 4 + e) * stride];
		return I6;
	}
};
template <bool TABLE>
struct InertialSource {
	using type = ModelInertials;
};
template <>
struct InertialSource<true> {
	using type = TableInertials;
};

template <int NMAX>
struct Chain {  // world-frame kinematics of the movable bodies of one instance
	double R[NMAX][9];
	V3 o[NMAX], z[NMAX], c[NMAX];  // joint origin, joint axis, centre of mass
};

// One joint j of the forward kinematics, expanded in place in both traversals: R, o come in as the rotation and joint origin of the parent body
// (the base: identity, zero) and leave as those of body j, which are stored in K with the world axis and the centre of mass.  md, in, q, j and K
// are names in the caller's scope.  A macro rather than a function for the reason given at SAIP_FK_JOINT_STEP (saip_fk.h): as a function,
// force-inlined or not, it changes the schedule of the chain kernels.
#define RBD_FK_JOINT_STEP \
	o = o + mulR(R, v3(md.p0[j][0], md.p0[j][1], md.p0[j][2])); \
	double Rt[9]; \
	for (int r = 0; r < 3; r++) \
		for (int c = 0; c < 3; c++) Rt[3 * r + c] = R[3 * r] * md.R0[j][c] + R[3 * r + 1] * md.R0[j][3 + c] + R[3 * r + 2] * md.R0[j][6 + c]; \
	const double ax = md.axis[j][0], ay = md.axis[j][1], az = md.axis[j][2]; \
	if (md.jtype[j] == 1) { \
		double s, c; \
		sincos(q[j], &s, &c); \
		const double v = 1.0 - c; \
		const double Rq[9] = {c + ax * ax * v,      ax * ay * v - az * s, ax * az * v + ay * s, \
							  ay * ax * v + az * s, c + ay * ay * v,      ay * az * v - ax * s, \
							  az * ax * v - ay * s, az * ay * v + ax * s, c + az * az * v}; \
		for (int r = 0; r < 3; r++) \
			for (int c2 = 0; c2 < 3; c2++) R[3 * r + c2] = Rt[3 * r] * Rq[c2] + Rt[3 * r + 1] * Rq[3 + c2] + Rt[3 * r + 2] * Rq[6 + c2]; \
	} else { \
		for (int e = 0; e < 9; e++) R[e] = Rt[e]; \
		o = o + q[j] * mulR(R, v3(ax, ay, az)); \
	} \
	for (int e = 0; e < 9; e++) K.R[j][e] = R[e]; \
	K.o[j] = o; \
	K.z[j] = mulR(R, v3(ax, ay, az)); \
	K.c[j] = o + mulR(R, v3(in.com(md, j, 0), in.com(md, j, 1), in.com(md, j, 2)));

template <int NMAX, class IN = ModelInertials>
__device__ void chain_fk(const ModelDev& md, int n, const double* q, Chain<NMAX>& K, const IN in = IN()) {
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	V3 o = v3(0, 0, 0);
#pragma unroll
	for (int j = 0; j < n; j++) {
		RBD_FK_JOINT_STEP
	}
}

// world inertia times vector: R I R^T w
__device__ __forceinline__ V3 inertia_mul(const double* R, const double* I6, V3 w) {
	const V3 l = mulRt(R, w);
	const V3 Il = v3(I6[0] * l.x + I6[3] * l.y + I6[4] * l.z, I6[3] * l.x + I6[1] * l.y + I6[5] * l.z, I6[4] * l.x + I6[5] * l.y + I6[2] * l.z);
	return mulR(R, Il);
}

// One body j of the forward pass of recursive Newton-Euler, in two statements (macros for the same reason as RBD_FK_JOINT_STEP).
// RBD_RNEA_MOTION_STEP: w, al, a (angular velocity, angular acceleration, linear acceleration of the joint origin) come in as the parent
// body's, with op its joint origin, and leave as body j's.  RBD_RNEA_FORCE_STEP: f_ = net force on body j, nn_ = net moment about its centre
// of mass rc.
#define RBD_RNEA_MOTION_STEP \
	const V3 r = K.o[j] - op; \
	a = a + cross(al, r); \
	if (with_velocity) a = a + cross(w, cross(w, r)); \
	const V3 z = K.z[j]; \
	if (md.jtype[j] == 1) { \
		if (with_velocity) al = al + dq[j] * cross(w, z); \
		al = al + ddq[j] * z; \
		if (with_velocity) w = w + dq[j] * z; \
	} else { \
		if (with_velocity) a = a + 2.0 * dq[j] * cross(w, z); \
		a = a + ddq[j] * z; \
	}
#define RBD_RNEA_FORCE_STEP(f_, nn_) \
	const V3 rc = K.c[j] - K.o[j]; \
	V3 ac = a + cross(al, rc); \
	if (with_velocity) ac = ac + cross(w, cross(w, rc)); \
	f_ = in.mass(md, j) * ac; \
	double I6s_[6]; \
	const double* const I6_ = in.inertia(md, j, I6s_); \
	nn_ = inertia_mul(K.R[j], I6_, al); \
	if (with_velocity) nn_ = nn_ + cross(w, inertia_mul(K.R[j], I6_, w));

// Recursive Newton-Euler in world coordinates: joint torques for (dq, ddq) with base acceleration a0 (= -gravity).
// with_velocity = false drops every velocity-product term (used for the columns of M).
template <int NMAX, class IN = ModelInertials>
__device__ void rnea(const ModelDev& md, int n, const Chain<NMAX>& K, const double* dq, const double* ddq, V3 a0, bool with_velocity, double* tau, const IN in = IN()) {
	V3 f[NMAX], nn[NMAX];  // net force on body j, net moment about its centre of mass
	V3 w = v3(0, 0, 0), al = v3(0, 0, 0), a = a0, op = v3(0, 0, 0);
#pragma unroll
	for (int j = 0; j < n; j++) {
		RBD_RNEA_MOTION_STEP
		RBD_RNEA_FORCE_STEP(f[j], nn[j])
		op = K.o[j];
	}
	V3 F = v3(0, 0, 0), N = v3(0, 0, 0);  // force / moment (about o_j) transmitted through joint j
#pragma unroll
	for (int jj = 0; jj < n; jj++) {
		const int j = n - 1 - jj;
		if (j < n - 1) N = N + cross(K.o[j + 1] - K.o[j], F);  // shift the child's wrench from o_{j+1} to o_j
		F = F + f[j];
		N = N + nn[j] + cross(K.c[j] - K.o[j], f[j]);
		tau[j] = md.jtype[j] == 1 ? dot(K.z[j], N) : dot(K.z[j], F);
	}
}

// kinematic tree: body j starts from its parent's frame (ModelDev::parent, the base when -1)
template <int NMAX, class IN = ModelInertials>
__device__ void chain_fk_tree(const ModelDev& md, int n, const double* q, Chain<NMAX>& K, const IN in = IN()) {
	for (int j = 0; j < n; j++) {
		const int pa = md.parent[j];
		double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		V3 o = v3(0, 0, 0);
		if (pa >= 0) {
			for (int e = 0; e < 9; e++) R[e] = K.R[pa][e];
			o = K.o[pa];
		}
		RBD_FK_JOINT_STEP
	}
}

// Recursive Newton-Euler on a kinematic tree: the forward pass keeps w, alpha, a (at the joint origin) per body and starts each body from its
// parent's; the backward pass adds each body's transmitted wrench, shifted from o_j to o_parent, into its parent.
template <int NMAX, class IN = ModelInertials>
__device__ void rnea_tree(const ModelDev& md, int n, const Chain<NMAX>& K, const double* dq, const double* ddq, V3 a0, bool with_velocity, double* tau, const IN in = IN()) {
	V3 W[NMAX], AL[NMAX], A[NMAX];  // per body: angular velocity, angular acceleration, linear acceleration of the joint origin
	V3 F[NMAX], N[NMAX];            // force / moment (about o_j) transmitted through joint j
	for (int j = 0; j < n; j++) {
		const int pa = md.parent[j];
		V3 w = v3(0, 0, 0), al = v3(0, 0, 0), a = a0, op = v3(0, 0, 0);
		if (pa >= 0) {
			w = W[pa];
			al = AL[pa];
			a = A[pa];
			op = K.o[pa];
		}
		RBD_RNEA_MOTION_STEP
		W[j] = w;
		AL[j] = al;
		A[j] = a;
		V3 f, nn;
		RBD_RNEA_FORCE_STEP(f, nn)
		F[j] = f;
		N[j] = nn + cross(rc, f);
	}
	for (int jj = 0; jj < n; jj++) {
		const int j = n - 1 - jj;  // every child of j (index > j) has already added its wrench
		tau[j] = md.jtype[j] == 1 ? dot(K.z[j], N[j]) : dot(K.z[j], F[j]);
		const int pa = md.parent[j];
		if (pa >= 0) {
			F[pa] = F[pa] + F[j];
			N[pa] = N[pa] + N[j] + cross(K.o[j] - K.o[pa], F[j]);
		}
	}
}

}  // namespace

// Joint-space inertia from composite rigid bodies in world axes (serial chain: every later body is a descendant).
// Spatial inertia of the composite j.. about the origin o_j of its own joint: mass cm, first moment ch = sum m (c - o_j), rotational inertia
// cI = sum R I R^T + m (r.r 1 - r r^T), r = c - o_j.  Going from joint j + 1 to joint j the reference point moves by d = o_{j+1} - o_j:
// cI += 2 (g.d) 1 - g d^T - d g^T with g = ch + cm d / 2, then ch += cm d.  Column j: momentum of the composite under the unit motion of joint
// j, (p, L) = Ic_j s_j with s_j = (z_j, 0) for a revolute and (0, z_j) for a prismatic joint; M_ij = s_i . (L, p) for i <= j, where joint i
// moves the point o_j with (o_i - o_j) x z_i.
// (Not about the world origin: there every entry carries a rounding of eps m |c|^2, |c| the distance from the origin, which swamps a small
// distal inertia -- the last wrist joint of a 6R arm of the PUMA layout, M_66 = 1.5e-4 at 1.5 m, was off by 3e2 n eps of its own sum.)
template <int NMAX, class IN = ModelInertials>
__device__ __forceinline__ void mass_matrix_crb(const ModelDev& md, const int n, const Chain<NMAX>& K, double (&M)[NMAX][NMAX], const IN in = IN()) {
	double cm = 0.0;
	V3 ch = v3(0, 0, 0);
	double cI[6] = {0, 0, 0, 0, 0, 0};  // xx yy zz xy xz yz
#pragma unroll
	for (int jj = 0; jj < n; jj++) {
		const int j = n - 1 - jj;
		const V3 oj = K.o[j];
		if (jj > 0) {  // the composite j + 1.. about o_j
			const V3 d = K.o[j + 1] - oj;
			const V3 g = ch + (0.5 * cm) * d;
			const double gd = dot(g, d);
			cI[0] += 2.0 * (gd - g.x * d.x);
			cI[1] += 2.0 * (gd - g.y * d.y);
			cI[2] += 2.0 * (gd - g.z * d.z);
			cI[3] -= g.x * d.y + g.y * d.x;
			cI[4] -= g.x * d.z + g.z * d.x;
			cI[5] -= g.y * d.z + g.z * d.y;
			ch = ch + cm * d;
		}
		// add body j to the composite
		const double m = in.mass(md, j);
		const V3 c = K.c[j] - oj;
		const double* R = K.R[j];
		double I6s[6];
		const double* I6 = in.inertia(md, j, I6s);
		// R I R^T
		double RI[9];
#pragma unroll
		for (int r = 0; r < 3; r++) {
			RI[3 * r + 0] = R[3 * r] * I6[0] + R[3 * r + 1] * I6[3] + R[3 * r + 2] * I6[4];
			RI[3 * r + 1] = R[3 * r] * I6[3] + R[3 * r + 1] * I6[1] + R[3 * r + 2] * I6[5];
			RI[3 * r + 2] = R[3 * r] * I6[4] + R[3 * r + 1] * I6[5] + R[3 * r + 2] * I6[2];
		}
		const double cc = dot(c, c);
		cI[0] += RI[0] * R[0] + RI[1] * R[1] + RI[2] * R[2] + m * (cc - c.x * c.x);
		cI[1] += RI[3] * R[3] + RI[4] * R[4] + RI[5] * R[5] + m * (cc - c.y * c.y);
		cI[2] += RI[6] * R[6] + RI[7] * R[7] + RI[8] * R[8] + m * (cc - c.z * c.z);
		cI[3] += RI[0] * R[3] + RI[1] * R[4] + RI[2] * R[5] - m * c.x * c.y;
		cI[4] += RI[0] * R[6] + RI[1] * R[7] + RI[2] * R[8] - m * c.x * c.z;
		cI[5] += RI[3] * R[6] + RI[4] * R[7] + RI[5] * R[8] - m * c.y * c.z;
		cm += m;
		ch = ch + m * c;
		// unit motion of joint j
		const bool rev = md.jtype[j] == 1;
		const V3 wj = rev ? K.z[j] : v3(0, 0, 0);
		const V3 vj = rev ? v3(0, 0, 0) : K.z[j];
		const V3 p = cm * vj + cross(wj, ch);
		const V3 L = v3(cI[0] * wj.x + cI[3] * wj.y + cI[4] * wj.z, cI[3] * wj.x + cI[1] * wj.y + cI[5] * wj.z, cI[4] * wj.x + cI[5] * wj.y + cI[2] * wj.z) +
					 cross(ch, vj);
#pragma unroll
		for (int i = 0; i < n; i++) {
			if (i > j) continue;
			const bool ri = md.jtype[i] == 1;
			const V3 wi = ri ? K.z[i] : v3(0, 0, 0);
			const V3 vi = ri ? cross(K.o[i] - oj, K.z[i]) : K.z[i];
			const double v = dot(wi, L) + dot(vi, p);
			M[i][j] = v;
			M[j][i] = v;
		}
	}
}

// mass_matrix_crb of a kinematic tree: the composite of body j sums its subtree (ModelDev::desc), every body about o_j, and M_ij, i < j, is
// nonzero only for i an ancestor of j (ModelDev::anc)
template <int NMAX, class IN = ModelInertials>
__device__ void mass_matrix_crb_tree(const ModelDev& md, const int n, const Chain<NMAX>& K, double (&M)[NMAX][NMAX], const IN in = IN()) {
	double bm[NMAX], bI[NMAX][6];
	for (int j = 0; j < n; j++) {  // mass of body j and its rotational inertia about its centre of mass, world axes
		const double* R = K.R[j];
		double I6s[6];
		const double* I6 = in.inertia(md, j, I6s);
		double RI[9];
		for (int r = 0; r < 3; r++) {
			RI[3 * r + 0] = R[3 * r] * I6[0] + R[3 * r + 1] * I6[3] + R[3 * r + 2] * I6[4];
			RI[3 * r + 1] = R[3 * r] * I6[3] + R[3 * r + 1] * I6[1] + R[3 * r + 2] * I6[5];
			RI[3 * r + 2] = R[3 * r] * I6[4] + R[3 * r + 1] * I6[5] + R[3 * r + 2] * I6[2];
		}
		bI[j][0] = RI[0] * R[0] + RI[1] * R[1] + RI[2] * R[2];
		bI[j][1] = RI[3] * R[3] + RI[4] * R[4] + RI[5] * R[5];
		bI[j][2] = RI[6] * R[6] + RI[7] * R[7] + RI[8] * R[8];
		bI[j][3] = RI[0] * R[3] + RI[1] * R[4] + RI[2] * R[5];
		bI[j][4] = RI[0] * R[6] + RI[1] * R[7] + RI[2] * R[8];
		bI[j][5] = RI[3] * R[6] + RI[4] * R[7] + RI[5] * R[8];
		bm[j] = in.mass(md, j);
	}
	for (int j = 0; j < n; j++) {
		double cm = 0.0, cI[6] = {0, 0, 0, 0, 0, 0};
		V3 ch = v3(0, 0, 0);
		const V3 oj = K.o[j];
		const uint32_t dm = md.desc[j];
		for (int l = j; l < n; l++) {
			if (!((dm >> l) & 1u)) continue;
			const double m = bm[l];
			const V3 c = K.c[l] - oj;
			const double cc = dot(c, c);
			cm += m;
			ch = ch + m * c;
			cI[0] += bI[l][0] + m * (cc - c.x * c.x);
			cI[1] += bI[l][1] + m * (cc - c.y * c.y);
			cI[2] += bI[l][2] + m * (cc - c.z * c.z);
			cI[3] += bI[l][3] - m * c.x * c.y;
			cI[4] += bI[l][4] - m * c.x * c.z;
			cI[5] += bI[l][5] - m * c.y * c.z;
		}
		const bool rev = md.jtype[j] == 1;
		const V3 wj = rev ? K.z[j] : v3(0, 0, 0);
		const V3 vj = rev ? v3(0, 0, 0) : K.z[j];
		const V3 p = cm * vj + cross(wj, ch);
		const V3 L = v3(cI[0] * wj.x + cI[3] * wj.y + cI[4] * wj.z, cI[3] * wj.x + cI[1] * wj.y + cI[5] * wj.z, cI[4] * wj.x + cI[5] * wj.y + cI[2] * wj.z) +
					 cross(ch, vj);
		const uint32_t am = md.anc[j];
		for (int i = 0; i <= j; i++) {
			double v = 0.0;
			if ((am >> i) & 1u) {
				const bool ri = md.jtype[i] == 1;
				const V3 wi = ri ? K.z[i] : v3(0, 0, 0);
				const V3 vi = ri ? cross(K.o[i] - oj, K.z[i]) : K.z[i];
				v = dot(wi, L) + dot(vi, p);
			}
			M[i][j] = v;
			M[j][i] = v;
		}
	}
}

}  // namespace saip
