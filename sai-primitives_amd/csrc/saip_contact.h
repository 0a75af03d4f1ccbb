// Contact planes and the simulated force sensor of the resident simulator (saip_contact.hip): the per-instance arithmetic, shared by the
// kernel and by host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_sampler.h and saip_state_snapshot.h).
//
// One contact point p = x_c + R_c r_c carried by the body of a motion-force task (x_c, R_c: control point and control frame, r_c: an offset in
// the control frame) against up to CONTACT_MAX_PLANES world-fixed half-spaces.  A plane is eight words: unit normal n (3), offset o,
// stiffness k, damping c, friction mu, slip-regularisation speed v_s.  With d = n.p - o and v the velocity of the point, a plane acts only
// when d < 0:
//   v_n = n.v    f_n = max(0, -k d - c v_n)    v_t = v - v_n n    f_t = -mu f_n v_t / max(|v_t|, v_s)
// and the force on the robot is f = sum (f_n n + f_t).
//
// Every function below rounds each product and each sum on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/contact_ref.py) reproduces it bit for bit; sqrt and the division are correctly rounded on the host and on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAIP_CT_HD __host__ __device__
#else
#define SAIP_CT_HD
#endif

namespace saip {

enum { CONTACT_MAX_PLANES = 4, CONTACT_PLANE_WORDS = 8, CONTACT_READOUT_ROWS = 8, CONTACT_SUMMARY_ROWS = 4 };
enum { CONTACT_SENSE = 0, CONTACT_APPLY = 1 };

// a . b = ((a0 b0 + a1 b1) + a2 b2)
SAIP_CT_HD inline double ct_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
	return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// a x b, every component one rounded difference of two rounded products
SAIP_CT_HD inline void ct_cross(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
	o[0] = a[1] * b[2] - a[2] * b[1];
	o[1] = a[2] * b[0] - a[0] * b[2];
	o[2] = a[0] * b[1] - a[1] * b[0];
}
// R v and R^T v of a row-major 3 x 3, rows / columns summed left to right
SAIP_CT_HD inline void ct_mat_vec(const double* R, const double* v, double* o) {
#pragma clang fp contract(off)
	for (int i = 0; i < 3; i++) o[i] = (R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2];
}
SAIP_CT_HD inline void ct_matT_vec(const double* R, const double* v, double* o) {
#pragma clang fp contract(off)
	for (int i = 0; i < 3; i++) o[i] = (R[i] * v[0] + R[3 + i] * v[1]) + R[6 + i] * v[2];
}

// the contact point p = x_c + R_c r_c
SAIP_CT_HD inline void ct_point(const double* xc, const double* Rc, const double* rc, double* p) {
#pragma clang fp contract(off)
	double t[3];
	ct_mat_vec(Rc, rc, t);
	for (int e = 0; e < 3; e++) p[e] = xc[e] + t[e];
}
// its velocity from the accumulators of SAIP_FK_TWIST_STEP (saip_fk.h): v = (tv + tw x p) - tc
SAIP_CT_HD inline void ct_velocity(const double* tv, const double* tw, const double* tc, const double* p, double* v) {
#pragma clang fp contract(off)
	double x[3];
	ct_cross(tw, p, x);
	for (int e = 0; e < 3; e++) v[e] = (tv[e] + x[e]) - tc[e];
}

struct ContactForce {
	double f[3];     // force on the robot at p, world frame
	double fn_sum;   // sum of the normal force magnitudes
	double dmin;     // smallest signed distance over the planes (negative: penetration)
	int active;      // planes with d < 0
};

// The planes of one instance.  Word w of plane k is planes[(k * CONTACT_PLANE_WORDS + w) * stride + col]: a batch-uniform table [P][8] has
// stride 1 and col 0, a per-instance table [P][8][ld] has stride ld and col = the instance.
SAIP_CT_HD inline void ct_plane_forces(const double* planes, int n_planes, long long stride, long long col, const double* p, const double* v,
										ContactForce* out) {
#pragma clang fp contract(off)
	double f[3] = {0.0, 0.0, 0.0}, fn_sum = 0.0, dmin = 0.0;
	int active = 0;
	for (int k = 0; k < n_planes; k++) {
		const double* w = planes + (long long)k * CONTACT_PLANE_WORDS * stride + col;
		const double n[3] = {w[0], w[stride], w[2 * stride]};
		const double off = w[3 * stride], ks = w[4 * stride], cd = w[5 * stride], mu = w[6 * stride], vs = w[7 * stride];
		const double d = ct_dot(n, p) - off;
		if (k == 0 || d < dmin) dmin = d;
		if (!(d < 0.0)) continue;
		active++;
		const double vn = ct_dot(n, v);
		const double fn = fmax(0.0, -ks * d - cd * vn);
		double vt[3];
		for (int e = 0; e < 3; e++) vt[e] = v[e] - vn * n[e];
		const double s = fmax(sqrt(ct_dot(vt, vt)), vs);
		const double g = mu * fn;
		for (int e = 0; e < 3; e++) {
			const double ft = -(g * vt[e]) / s;
			f[e] = f[e] + (fn * n[e] + ft);
		}
		fn_sum = fn_sum + fn;
	}
	for (int e = 0; e < 3; e++) out->f[e] = f[e];
	out->fn_sum = fn_sum;
	out->dmin = dmin;
	out->active = active;
}

// The same against moving surfaces (saip_env_schedule.h): plane k has the velocity v_p = vel[(k * 4 + e) * stride + col], e = 0..2, in the
// layout of the planes, and v_r = v - v_p (one rounding per component) takes the place of v in v_n, f_n, v_t and f_t.  With v_p = 0 these are
// the bits of ct_plane_forces.
SAIP_CT_HD inline void ct_plane_forces_moving(const double* planes, const double* vel, int n_planes, long long stride, long long col, const double* p,
											   const double* v, ContactForce* out) {
#pragma clang fp contract(off)
	double f[3] = {0.0, 0.0, 0.0}, fn_sum = 0.0, dmin = 0.0;
	int active = 0;
	for (int k = 0; k < n_planes; k++) {
		const double* w = planes + (long long)k * CONTACT_PLANE_WORDS * stride + col;
		const double* vp = vel + (long long)k * 4 * stride + col;
		const double n[3] = {w[0], w[stride], w[2 * stride]};
		const double off = w[3 * stride], ks = w[4 * stride], cd = w[5 * stride], mu = w[6 * stride], vs = w[7 * stride];
		const double d = ct_dot(n, p) - off;
		if (k == 0 || d < dmin) dmin = d;
		if (!(d < 0.0)) continue;
		active++;
		const double vr[3] = {v[0] - vp[0], v[1] - vp[stride], v[2] - vp[2 * stride]};
		const double vn = ct_dot(n, vr);
		const double fn = fmax(0.0, -ks * d - cd * vn);
		double vt[3];
		for (int e = 0; e < 3; e++) vt[e] = vr[e] - vn * n[e];
		const double s = fmax(sqrt(ct_dot(vt, vt)), vs);
		const double g = mu * fn;
		for (int e = 0; e < 3; e++) {
			const double ft = -(g * vt[e]) / s;
			f[e] = f[e] + (fn * n[e] + ft);
		}
		fn_sum = fn_sum + fn;
	}
	for (int e = 0; e < 3; e++) out->f[e] = f[e];
	out->fn_sum = fn_sum;
	out->dmin = dmin;
	out->active = active;
}

// tau_ext of one joint (column of J_v^T times f): aw the joint's world axis, oj its origin; revolute aw . ((p - oj) x f), prismatic aw . f.
// A joint that is not an ancestor of the body gets 0: the caller does not ask.
SAIP_CT_HD inline double ct_joint_torque(bool revolute, const double* aw, const double* oj, const double* p, const double* f) {
#pragma clang fp contract(off)
	if (!revolute) return ct_dot(aw, f);
	double r[3], m[3];
	for (int e = 0; e < 3; e++) r[e] = p[e] - oj[e];
	ct_cross(r, f, m);
	return ct_dot(aw, m);
}

// The simulated sensor: the exact inverse of LAW_SENSED_WRENCH (saip_law.h), in the reference's sign convention (MotionForceTask.h:538-553:
// the wrench the sensor applies to the environment).  World F = -f, m = (p - x_c) x F; control frame fc = R_c^T F, mc = R_c^T m; sensor
// frame FS = R_cs^T fc, MS = R_cs^T (mc - t_cs x fc).
SAIP_CT_HD inline void ct_sensor(const double* f, const double* p, const double* xc, const double* Rc, const double* Rcs, const double* tcs,
								  double* FS, double* MS) {
#pragma clang fp contract(off)
	double F[3], r[3], m[3], fc[3], mc[3], x[3], y[3];
	for (int e = 0; e < 3; e++) {
		F[e] = -f[e];
		r[e] = p[e] - xc[e];
	}
	ct_cross(r, F, m);
	ct_matT_vec(Rc, F, fc);
	ct_matT_vec(Rc, m, mc);
	ct_cross(tcs, fc, x);
	for (int e = 0; e < 3; e++) y[e] = mc[e] - x[e];
	ct_matT_vec(Rcs, fc, FS);
	ct_matT_vec(Rcs, y, MS);
}

// The running summaries of one instance after one APPLY substep of length dt (s: its column, rows ld apart): sum dt fn_sum, max |f|, max
// penetration, substeps in contact.
SAIP_CT_HD inline void ct_summary_advance(double* s, long long ld, double dt, const ContactForce& c) {
#pragma clang fp contract(off)
	s[0] = s[0] + dt * c.fn_sum;
	s[ld] = fmax(s[ld], sqrt(ct_dot(c.f, c.f)));
	s[2 * ld] = fmax(s[2 * ld], c.active ? -c.dmin : 0.0);
	s[3 * ld] = s[3 * ld] + (c.active ? 1.0 : 0.0);
}

// one launch of saip_contact_apply.  Passed to the kernel by value.
struct ModelDev;
struct TaskDev;
struct ContactParams {
	int B, ld, n, mode;          // mode: CONTACT_SENSE or CONTACT_APPLY
	int task, n_planes, per_instance, pad_;
	double dt;                   // length of the substep (APPLY: weight of summary row 0)
	double rc[3];                // the contact point in the control frame
	const ModelDev* model;
	const TaskDev* tasks;
	const double* q;             // [n][ld]
	const double* dq;            // [n][ld]
	const double* planes;        // [P][8] or [P][8][ld]
	double* goal;                // SENSE: the task's goal block; rows 30..35 are written
	const double* tau_cmd;       // APPLY: [n][ld] commanded torques (NaN = none)
	double* tau_sim;             // APPLY: [n][ld] commanded + contact torques
	double* readout;             // [8][ld]: f 3, p 3, smallest d, active planes
	double* summary;             // APPLY: [4][ld]
};
// ... of its MOVING instantiation: the planes have an environment schedule, which writes their velocities
struct ContactMovingParams : ContactParams {
	const double* vel;           // [P][4] or [P][4][ld]
};

}  // namespace saip
