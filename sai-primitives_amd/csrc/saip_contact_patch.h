// Contact patches of the resident simulator (saip_contact_patch.hip): the per-instance arithmetic, shared by the kernel and by host-compiled
// checks (plain C++ when no HIP compiler is reading it).  It reuses saip_contact.h unchanged.
//
// A patch is n_points (1..PATCH_MAX_POINTS) offsets r_i in the control frame of a motion-force task, carried by that task's body, against
// the patch's own n_planes (1..CONTACT_MAX_PLANES) half-spaces in the eight-word format of saip_contact.h.  Per point p_i = x_c + R_c r_i,
// v_i from the twist accumulators, c_i = ct_plane_forces(...).  An instance has PATCH_MAX_POINTS slots; slot i >= n_points holds exact zeros
// (f = 0, fn_sum = 0, active = 0, moment = 0) and is no candidate for the smallest distance.  Every sum over the slots has one shape,
//   v[i] += v[i + off]   for off = 4, 2, 1
// (the kernel's eight-lane fold), so the rounding order is part of the definition; tests/contact_patch_ref.py restates it in NumPy.
//   F = sum f_i    M = sum (p_i - x_c) x f_i (the difference rounded, then ct_cross)    fn_total = sum fn_sum_i
//   dmin = the smallest c_i.dmin over the used slots, i_deep the lowest index that attains it, n_touch = points with c_i.active > 0
// The torque of ancestor joint j is sum_i (c_i.active ? ct_joint_torque(rev_j, aw_j, o_j, p_i, f_i) : 0.0), added to the commanded torque
// only when n_touch > 0 (otherwise the torques pass through untouched), so a one-point patch gives the numbers of saip_contact_apply.
#pragma once
#include "saip_contact.h"

namespace saip {

enum { PATCH_MAX_POINTS = 8, PATCH_MAX = 2, PATCH_READOUT_ROWS = 20, PATCH_SUMMARY_ROWS = 6 };

// one slot of an instance
struct PatchSlot {
	double p[3];     // the point, world frame
	double m[3];     // (p - x_c) x f
	ContactForce c;
	double dcand;    // c.dmin of a used slot, +inf of an unused one: the candidate for the smallest distance
};

SAIP_CT_HD inline void cp_slot_unused(PatchSlot* s) {
	for (int e = 0; e < 3; e++) s->p[e] = s->m[e] = s->c.f[e] = 0.0;
	s->c.fn_sum = 0.0;
	s->c.dmin = 0.0;
	s->c.active = 0;
	s->dcand = HUGE_VAL;
}
// a used slot: the point r (control frame) at the pose xc, Rc with the twist accumulators tv, tw, tc against the planes (layout: ct_plane_forces)
SAIP_CT_HD inline void cp_slot_eval(const double* planes, int n_planes, long long stride, long long col, const double* xc, const double* Rc,
									 const double* r, const double* tv, const double* tw, const double* tc, PatchSlot* s) {
#pragma clang fp contract(off)
	double v[3], d[3];
	ct_point(xc, Rc, r, s->p);
	ct_velocity(tv, tw, tc, s->p, v);
	ct_plane_forces(planes, n_planes, stride, col, s->p, v, &s->c);
	for (int e = 0; e < 3; e++) d[e] = s->p[e] - xc[e];
	ct_cross(d, s->c.f, s->m);
	s->dcand = s->c.dmin;
}
// ... against moving surfaces: cp_slot_eval with ct_plane_forces_moving and the planes' velocity table (layout: the planes')
SAIP_CT_HD inline void cp_slot_eval_moving(const double* planes, const double* vel, int n_planes, long long stride, long long col, const double* xc,
											const double* Rc, const double* r, const double* tv, const double* tw, const double* tc, PatchSlot* s) {
#pragma clang fp contract(off)
	double v[3], d[3];
	ct_point(xc, Rc, r, s->p);
	ct_velocity(tv, tw, tc, s->p, v);
	ct_plane_forces_moving(planes, vel, n_planes, stride, col, s->p, v, &s->c);
	for (int e = 0; e < 3; e++) d[e] = s->p[e] - xc[e];
	ct_cross(d, s->c.f, s->m);
	s->dcand = s->c.dmin;
}
// the order of the smallest-distance fold: candidate (db, ib) replaces (da, ia) when it is deeper, or as deep with the lower index
SAIP_CT_HD inline bool cp_deeper(double db, int ib, double da, int ia) { return db < da || (db == da && ib < ia); }

struct PatchNet {
	double F[3], M[3], fn_total, dmin;
	int n_touch, i_deep;
};

// The folds over the eight slots as plain loops: what the kernel does with cross-lane moves (lane 0's result).
inline void cp_fold_sum(double* v) {
	for (int off = PATCH_MAX_POINTS / 2; off > 0; off >>= 1)
		for (int i = 0; i < off; i++) v[i] = v[i] + v[i + off];
}
inline void cp_net(const PatchSlot* s, PatchNet* out) {
	double v[PATCH_MAX_POINTS], d[PATCH_MAX_POINTS];
	int ix[PATCH_MAX_POINTS];
	for (int e = 0; e < 3; e++) {
		for (int i = 0; i < PATCH_MAX_POINTS; i++) v[i] = s[i].c.f[e];
		cp_fold_sum(v);
		out->F[e] = v[0];
		for (int i = 0; i < PATCH_MAX_POINTS; i++) v[i] = s[i].m[e];
		cp_fold_sum(v);
		out->M[e] = v[0];
	}
	for (int i = 0; i < PATCH_MAX_POINTS; i++) v[i] = s[i].c.fn_sum;
	cp_fold_sum(v);
	out->fn_total = v[0];
	out->n_touch = 0;
	for (int i = 0; i < PATCH_MAX_POINTS; i++) {
		out->n_touch += s[i].c.active > 0 ? 1 : 0;
		d[i] = s[i].dcand;
		ix[i] = i;
	}
	for (int off = PATCH_MAX_POINTS / 2; off > 0; off >>= 1)
		for (int i = 0; i < off; i++)
			if (cp_deeper(d[i + off], ix[i + off], d[i], ix[i])) {
				d[i] = d[i + off];
				ix[i] = ix[i + off];
			}
	out->dmin = d[0];
	out->i_deep = ix[0];
}
// the torque of one ancestor joint from the eight slots
inline double cp_joint_torque(bool revolute, const double* aw, const double* oj, const PatchSlot* s) {
	double v[PATCH_MAX_POINTS];
	for (int i = 0; i < PATCH_MAX_POINTS; i++) v[i] = s[i].c.active ? ct_joint_torque(revolute, aw, oj, s[i].p, s[i].c.f) : 0.0;
	cp_fold_sum(v);
	return v[0];
}

// The simulated sensor of a patch: world F_w = -F, m_w = -M; control frame fc = R_c^T F_w, mc = R_c^T m_w; the tail of ct_sensor:
// FS = R_cs^T fc, MS = R_cs^T (mc - t_cs x fc).  For one point these are the bits of ct_sensor (negation commutes with every product and
// difference there).
SAIP_CT_HD inline void cp_sensor(const double* F, const double* M, const double* Rc, const double* Rcs, const double* tcs, double* FS, double* MS) {
#pragma clang fp contract(off)
	double Fw[3], mw[3], fc[3], mc[3], x[3], y[3];
	for (int e = 0; e < 3; e++) {
		Fw[e] = -F[e];
		mw[e] = -M[e];
	}
	ct_matT_vec(Rc, Fw, fc);
	ct_matT_vec(Rc, mw, mc);
	ct_cross(tcs, fc, x);
	for (int e = 0; e < 3; e++) y[e] = mc[e] - x[e];
	ct_matT_vec(Rcs, fc, FS);
	ct_matT_vec(Rcs, y, MS);
}

// The running summaries of one instance after one APPLY substep of length dt (s: its column, rows ld apart): sum dt fn_total, max |F|, max
// penetration, substeps with a point touching, max |M|, substeps in full contact (every point touching).
SAIP_CT_HD inline void cp_summary_advance(double* s, long long ld, double dt, const double* F, const double* M, double fn_total, double dmin,
										   int n_touch, int n_points) {
#pragma clang fp contract(off)
	s[0] = s[0] + dt * fn_total;
	s[ld] = fmax(s[ld], sqrt(ct_dot(F, F)));
	s[2 * ld] = fmax(s[2 * ld], n_touch > 0 ? -dmin : 0.0);
	s[3 * ld] = s[3 * ld] + (n_touch > 0 ? 1.0 : 0.0);
	s[4 * ld] = fmax(s[4 * ld], sqrt(ct_dot(M, M)));
	s[5 * ld] = s[5 * ld] + (n_touch == n_points ? 1.0 : 0.0);
}

// one patch of a launch
struct PatchDev {
	int task, n_points, n_planes, per_instance, sensor, pad_;
	double r[PATCH_MAX_POINTS][3];  // the points in the control frame
	const double* planes;           // [P][8] or [P][8][ld]
	double* goal;                   // SENSE: the task's goal block; rows 30..35 are written when `sensor`
	double* readout;                // [20][ld]
	double* summary;                // APPLY: [6][ld]
};
// one launch of saip_contact_patch_apply.  Passed to the kernel by value.
struct ContactPatchParams {
	int B, ld, n, mode;             // mode: CONTACT_SENSE (patches with the sensor only) or CONTACT_APPLY (all)
	int n_patches, pad_;
	double dt;                      // length of the substep (APPLY: weight of summary row 0)
	const ModelDev* model;
	const TaskDev* tasks;
	const double* q;                // [n][ld]
	const double* dq;               // [n][ld]
	const double* tau_cmd;          // APPLY: [n][ld] commanded torques (NaN = none)
	double* tau_sim;                // APPLY: [n][ld] (commanded + patch 0) + patch 1
	PatchDev patch[PATCH_MAX];
};
// ... of its MOVING instantiation: the planes of at least one patch have an environment schedule
struct ContactPatchMovingParams : ContactPatchParams {
	const double* vel[PATCH_MAX];   // per patch [P][4] or [P][4][ld]; nullptr: the planes of that patch stand still
};

}  // namespace saip
