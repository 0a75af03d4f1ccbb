// Forward kinematics of one control frame for one instance (straight walk over the chain; used by the
// re-initialisation paths only -- the cycle kernels have their own fused kinematics).
// SaiModel::positionInWorld / rotationInWorld call sites: MotionForceTask.cpp:212-216, 286-289.
#pragma once
#include "saip_device.h"

namespace saip {

// sin/cos for joint angles: Cody-Waite reduction by pi/2 (two FMA terms, exact for |x| < 1e5) + fdlibm kernel polynomials on
// [-pi/4, pi/4] (errors < 1 ulp); the rare |x| >= 1e5 takes the library path.  ~35 instructions instead of ~110.
__device__ __forceinline__ void sincos_joint(const double x, double* sn, double* cs) {
	if (!(fabs(x) < 1.0e5)) {
		sincos(x, sn, cs);
		return;
	}
	const double k = rint(x * 6.36619772367581382433e-01);
	double r = fma(-k, 1.57079632673412561417e+00, x);
	r = fma(-k, 6.07710050650619224932e-11, r);
	const double z = r * r;
	const double ps = fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06), -1.98412698298579493134e-04), 8.33333333332248946124e-03);
	const double s0 = fma(z * r, fma(z, ps, -1.66666666666666324348e-01), r);
	const double pc = z * fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07), 2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
	const double c0 = 1.0 - fma(0.5, z, -z * pc);
	const int q = (int)k & 3;
	const double sa = (q & 1) ? c0 : s0, ca = (q & 1) ? s0 : c0;
	*sn = (q & 2) ? -sa : sa;
	*cs = ((q + 1) & 2) ? -ca : ca;
}

__device__ __forceinline__ void fk_mat3_vec(const double* R, const double* v, double* o) {
	o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
	o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
	o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}

// The serial walk behind fk_control_frame, expanded in place: md, tk, q, ld, b, pos and Rc are names in the caller's scope.  The
// optional statement (__VA_ARGS__) runs for every joint j once its origin o (world) and joint frame Rt are known; the joint's world
// axis is Rt (ax, ay, az) (the joint rotation leaves its own axis fixed).  Library sin/cos on purpose: this pose seeds the OTG state,
// whose knife-edge decisions (collinearity within 2^-52) are compared against reference fixtures generated with the same arithmetic.
// A macro rather than a function so that fk_control_frame, which the general cycle kernel and the OTG inline, compiles to exactly the
// code it compiled to before the task diagnostics (saip_task_diag.hip) began to share it.
// SAIP_FK_JOINT_STEP is one joint j of that walk (R, o: rotation and origin of the body walked so last), for walks that emit several
// frames on the way (saip_model_query.hip).
#define SAIP_FK_JOINT_STEP(...)                                                                                                                 \
	double t3[3], Rn[9], Rt[9];                                                                                                                 \
	fk_mat3_vec(R, md.p0[j], t3);                                                                                                               \
	for (int e = 0; e < 3; e++) o[e] += t3[e];                                                                                                  \
	for (int r = 0; r < 3; r++)                                                                                                                 \
		for (int c = 0; c < 3; c++) Rt[3 * r + c] = R[3 * r] * md.R0[j][c] + R[3 * r + 1] * md.R0[j][3 + c] + R[3 * r + 2] * md.R0[j][6 + c];   \
	const double qj = q[(size_t)j * ld + b];                                                                                                    \
	const double ax = md.axis[j][0], ay = md.axis[j][1], az = md.axis[j][2];                                                                    \
	__VA_ARGS__                                                                                                                                 \
	if (md.jtype[j] == 1) {                                                                                                                     \
		double s, c;                                                                                                                            \
		sincos(qj, &s, &c);  /* library sin/cos on purpose: see above */                                                                        \
		const double v = 1.0 - c;                                                                                                               \
		const double Rq[9] = {c + ax * ax * v,      ax * ay * v - az * s, ax * az * v + ay * s,                                                 \
							  ay * ax * v + az * s, c + ay * ay * v,      ay * az * v - ax * s,                                                 \
							  az * ax * v - ay * s, az * ay * v + ax * s, c + az * az * v};                                                     \
		for (int r = 0; r < 3; r++)                                                                                                             \
			for (int c2 = 0; c2 < 3; c2++) Rn[3 * r + c2] = Rt[3 * r] * Rq[c2] + Rt[3 * r + 1] * Rq[3 + c2] + Rt[3 * r + 2] * Rq[6 + c2];       \
	} else {                                                                                                                                    \
		const double a[3] = {ax, ay, az};                                                                                                       \
		double d[3];                                                                                                                            \
		fk_mat3_vec(Rt, a, d);                                                                                                                  \
		for (int e = 0; e < 3; e++) o[e] += d[e] * qj;                                                                                          \
		for (int e = 0; e < 9; e++) Rn[e] = Rt[e];                                                                                              \
	}                                                                                                                                           \
	for (int e = 0; e < 9; e++) R[e] = Rn[e];
// TREE (a compile-time bool): a kinematic tree -- the same steps over the ancestors of the body only, in ascending order (a joint's origin is
// expressed in its parent body's frame, and every ancestor comes before its descendants)
#define SAIP_FK_WALK(TREE, ...)                                                                                                                 \
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};                                                                                \
	const uint32_t anc_ = TREE && tk.body >= 0 ? md.anc[tk.body] : 0u;                                                                          \
	for (int j = 0; j <= tk.body; j++) {                                                                                                        \
		if constexpr (TREE)                                                                                                                     \
			if (!((anc_ >> j) & 1u)) continue;                                                                                                  \
		SAIP_FK_JOINT_STEP(__VA_ARGS__)                                                                                                         \
	}                                                                                                                                           \
	double p[3];                                                                                                                                \
	fk_mat3_vec(R, tk.pos, p);                                                                                                                  \
	for (int e = 0; e < 3; e++) pos[e] = o[e] + p[e];                                                                                           \
	for (int r = 0; r < 3; r++)                                                                                                                 \
		for (int c = 0; c < 3; c++) Rc[3 * r + c] = R[3 * r] * tk.rot[c] + R[3 * r + 1] * tk.rot[3 + c] + R[3 * r + 2] * tk.rot[6 + c];

// world position of the control point and world rotation of the control frame of motion-force task tk; the two instantiations keep their names
__device__ inline void fk_control_frame(const ModelDev& md, const TaskDev& tk, const double* q, int ld, int b, double pos[3], double Rc[9]) {
	SAIP_FK_WALK(false)
}
__device__ inline void fk_control_frame_tree(const ModelDev& md, const TaskDev& tk, const double* q, int ld, int b, double pos[3], double Rc[9]) {
	SAIP_FK_WALK(true)
}

// compile-time choice for the templated kernels
template <bool TREE>
__device__ __forceinline__ void fk_control_frame_t(const ModelDev& md, const TaskDev& tk, const double* q, int ld, int b, double pos[3], double Rc[9]) {
	if constexpr (TREE) fk_control_frame_tree(md, tk, q, ld, b, pos, Rc);
	else fk_control_frame(md, tk, q, ld, b, pos, Rc);
}

// Statement for SAIP_FK_JOINT_STEP / SAIP_FK_WALK that accumulates the unprojected world twist of a point p carried by the body walked to
// (tv, tw, tc, dq_ and ld, b are names in the caller's scope): with aw = Rt (ax, ay, az) the world axis and o the origin of joint j, a
// revolute joint (rev) adds aw dq to tw and dq (aw x o) to tc, a prismatic joint adds aw dq to tv; at the end v = tv + tw x p - tc and
// w = tw, since sum_j dq_j aw_j x (p - o_j) = tw x p - tc.  aw and rev stay in scope for what follows (the Jacobian columns).
#define SAIP_FK_TWIST_STEP(dq_)                                                                                                                 \
	const double aj[3] = {ax, ay, az};                                                                                                          \
	const double dqj = (dq_)[(size_t)j * ld + b];                                                                                               \
	double aw[3];                                                                                                                               \
	fk_mat3_vec(Rt, aj, aw);                                                                                                                    \
	const bool rev = md.jtype[j] == 1;                                                                                                          \
	if (rev) {                                                                                                                                  \
		for (int e = 0; e < 3; e++) tw[e] += aw[e] * dqj;                                                                                       \
		tc[0] += dqj * (aw[1] * o[2] - aw[2] * o[1]);                                                                                           \
		tc[1] += dqj * (aw[2] * o[0] - aw[0] * o[2]);                                                                                           \
		tc[2] += dqj * (aw[0] * o[1] - aw[1] * o[0]);                                                                                           \
	} else {                                                                                                                                    \
		for (int e = 0; e < 3; e++) tv[e] += aw[e] * dqj;                                                                                       \
	}

}  // namespace saip
