// The pushed object of the resident simulator: an optional second stage of link contact (saip_link_contact.h).  One free rigid body per
// instance, made of P spheres, that the robot's link spheres push and that the link-contact obstacles hold up.  The per-instance
// arithmetic, shared by the kernel (saip_link_contact.hip) and by host-compiled checks (plain C++ when no HIP compiler is reading it).
//
// State x[13] = { p[3], quat (w, x, y, z) body to world, v[3], omega[3] (world frame) }, inertial words { m, Ix, Iy, Iz } (principal moments
// in body axes), shape: P spheres { r[3], radius } in the body frame, one material { k, c, mu, v_s } for robot-object contact.
//
// One substep of length dt, at the state of that substep:
//   1  R = lo_rotation(quat); object sphere p: c_p = p + R r_p (cl_centre), a_p = c_p - p, v_p = v + omega x a_p (lo_sphere).
//   2  robot sphere (sorted position i) x object sphere p: lc_item on the 8-word obstacle { capsule, c_p, c_p, radius_p } with the object's
//      material and the velocity v_s - v_p.  f acts on the robot sphere, nf = -f on the object at c_p with the moment a_p x nf.
//      F_s = (the world-obstacle items in ascending order, as lc_lane sums them) then + the object items p = 0 .. P-1.  The link-contact
//      partial (its readout and summaries) is formed from the world-obstacle items alone, exactly as lc_lane forms it: the object never
//      shows in the link-contact readout.  The flag of a sphere is "has an active item of either kind".
//   3  object sphere p x obstacle o = 0 .. O-1 with obstacle o's material: lc_item with c_p, v_p, radius_p; f acts on the object at c_p.
//   4  the work split: lane l keeps the reaction partial (rf, rm, smallest distance, its item, sum f_n, active items) over the sorted robot
//      spheres l, l + 8, ... it owns, each over p = 0 .. P-1, in that order; lane l < P keeps the world partial (wf, wm, largest
//      penetration) of object sphere l over the obstacles in ascending order.  The eight partials fold as v[l] (+)= v[l + off], off = 4, 2, 1
//      (lo_fold).  Net force F = (m g + wf) + rf, net moment about p T = wm + rf's partner rm: T = wm + rm.
//   5  semi-implicit Euler (lo_integrate): v' = v + dt (F / m); with t_b = R^T T, w_b = R^T omega, the gyroscopic term in Euler's form
//      y = ((Iz - Iy) w_b1 w_b2, (Ix - Iz) w_b2 w_b0, (Iy - Ix) w_b0 w_b1), d_b = dt ((t_b - y) / I), omega' = omega + R d_b (the increment
//      form of omega_b' = omega_b + d_b, omega' = R omega_b': a torque-free body with equal moments keeps omega bit for bit);
//      p' = p + dt v'; quat' = (quat + (dt / 2) ((0, omega') (x) quat)) / |.|.
// An instance with a robot sphere centre or an object state word that is not finite is invalid: tau_sim = u0, the state is not written, the
// object readout is NaN.  The torque loop of the robot runs iff the instance is valid and a world or an object item is active.
//
// Every function rounds each product and each sum on its own (no contraction), in the order written, so that tests/link_object_ref.py
// reproduces it bit for bit; sqrt and the division are correctly rounded on the host and on the device.
#pragma once
#include "saip_link_contact.h"

namespace saip {

enum { LINK_OBJECT_MAX_SPHERES = 8, LINK_OBJECT_STATE_ROWS = 13, LINK_OBJECT_INERTIAL_WORDS = 4, LINK_OBJECT_READOUT_ROWS = 12, LINK_OBJECT_SUMMARY_ROWS = 4 };
// a vector per object sphere of the eight instances of one block: component e of sphere p of group g
enum { LINK_OBJECT_VEC_WORDS = LINK_OBJECT_MAX_SPHERES * 3 * LINK_CONTACT_GROUPS };
SAIP_LC_HD inline int lo_index(int p, int e, int g) { return (p * 3 + e) * LINK_CONTACT_GROUPS + g; }

// the shape, batch-uniform, as the device keeps it
struct LinkObjectGeom {
	int P, pad_;
	double r[LINK_OBJECT_MAX_SPHERES][3];
	double radius[LINK_OBJECT_MAX_SPHERES];
	double mat[LINK_CONTACT_MATERIAL_WORDS];
};

SAIP_LC_HD inline void lo_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
	c[0] = a[1] * b[2] - a[2] * b[1];
	c[1] = a[2] * b[0] - a[0] * b[2];
	c[2] = a[0] * b[1] - a[1] * b[0];
}
// row-major R of the unit quaternion (w, x, y, z)
SAIP_LC_HD inline void lo_rotation(const double* q, double* R) {
#pragma clang fp contract(off)
	const double w = q[0], x = q[1], y = q[2], z = q[3];
	const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
	R[0] = 1.0 - 2.0 * (yy + zz);
	R[1] = 2.0 * (xy - wz);
	R[2] = 2.0 * (xz + wy);
	R[3] = 2.0 * (xy + wz);
	R[4] = 1.0 - 2.0 * (xx + zz);
	R[5] = 2.0 * (yz - wx);
	R[6] = 2.0 * (xz - wy);
	R[7] = 2.0 * (yz + wx);
	R[8] = 1.0 - 2.0 * (xx + yy);
}
// centre and velocity of the object sphere at r (body frame): x the state, R its rotation
SAIP_LC_HD inline void lo_sphere(const double* x, const double* R, const double* r, double* c, double* v) {
#pragma clang fp contract(off)
	double a[3], wa[3];
	cl_centre(x, R, r, c);
	for (int e = 0; e < 3; e++) a[e] = c[e] - x[e];
	lo_cross(x + 10, a, wa);
	for (int e = 0; e < 3; e++) v[e] = x[7 + e] + wa[e];
}
SAIP_LC_HD inline bool lo_state_finite(const double* x) {
	bool ok = true;
	for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) ok = ok && cl_finite(x[r]);
	return ok;
}

// what one lane keeps of the object, and what the fold leaves in lane 0
struct LinkObjectPartial {
	double rf[3], rm[3];  // robot on object: force, moment about p
	double wf[3], wm[3];  // world on object
	double dmin;          // smallest robot-object distance (+inf: no item)
	double fn_sum;        // sum of f_n over the robot-object items
	double wpen;          // largest object-world penetration max(0, -d)
	int k;                // item s P + p of dmin in the caller's sphere numbering (-1: none); the lowest among equals
	int active;           // active robot-object items
};
SAIP_LC_HD inline void lo_partial_clear(LinkObjectPartial* q) {
	for (int e = 0; e < 3; e++) q->rf[e] = q->rm[e] = q->wf[e] = q->wm[e] = 0.0;
	q->dmin = INFINITY;
	q->fn_sum = 0.0;
	q->wpen = 0.0;
	q->k = -1;
	q->active = 0;
}

// Lane `lane` of the instance in group g over the robot spheres it owns: lc_lane with the object items behind the world items of every
// sphere.  OC, OV: centres and velocities of the object spheres (lo_index), pos: the body origin p.  *out is what lc_lane would leave (world
// items only), *obj receives the reaction partial (its world part is left as it is).
SAIP_LC_HD inline void lo_lane(const LinkContactView& W, const LinkObjectGeom& OG, const double* C, const double* V, const double* OC, const double* OV,
								const double* pos, double* F, int* A, int g, int lane, LinkContactPartial* out, LinkObjectPartial* obj) {
#pragma clang fp contract(off)
	LinkContactPartial p = {{0.0, 0.0, 0.0}, INFINITY, 0.0, 0.0, -1, 0, 0};
	LinkObjectPartial q = *obj;
	for (int i = lane; i < W.S; i += LINK_CONTACT_LANES) {
		const double c[3] = {C[cl_centre_index(i, 0, g)], C[cl_centre_index(i, 1, g)], C[cl_centre_index(i, 2, g)]};
		const double v[3] = {V[cl_centre_index(i, 0, g)], V[cl_centre_index(i, 1, g)], V[cl_centre_index(i, 2, g)]};
		for (int e = 0; e < 3; e++)
			if (!cl_finite(c[e])) p.bad = 1;
		double Fs[3] = {0.0, 0.0, 0.0};
		int act = lc_sphere_items(W, i, c, v, p, Fs);
		for (int e = 0; e < 3; e++) p.f[e] = p.f[e] + Fs[e];  // the link-contact readout: the world items alone
		p.active += act;
		for (int s = 0; s < OG.P; s++) {
			const double cp[3] = {OC[lo_index(s, 0, g)], OC[lo_index(s, 1, g)], OC[lo_index(s, 2, g)]};
			const double w[LINK_CONTACT_OBSTACLE_WORDS] = {(double)CLEARANCE_CAPSULE, cp[0], cp[1], cp[2], cp[0], cp[1], cp[2], OG.radius[s]};
			double vr[3];
			for (int e = 0; e < 3; e++) vr[e] = v[e] - OV[lo_index(s, e, g)];
			LinkContactItem it;
			lc_item(w, 1, OG.mat, c, vr, W.radius[i], &it);
			const int k = W.slot[i] * OG.P + s;
			if (it.d < q.dmin || (it.d == q.dmin && k < q.k)) {
				q.dmin = it.d;
				q.k = k;
			}
			if (!it.active) continue;
			act++;
			q.active++;
			double nf[3], a[3], m[3];
			for (int e = 0; e < 3; e++) {
				Fs[e] = Fs[e] + it.f[e];
				nf[e] = -it.f[e];
				a[e] = cp[e] - pos[e];
			}
			lo_cross(a, nf, m);
			for (int e = 0; e < 3; e++) {
				q.rf[e] = q.rf[e] + nf[e];
				q.rm[e] = q.rm[e] + m[e];
			}
			q.fn_sum = q.fn_sum + it.fn;
		}
		for (int e = 0; e < 3; e++) F[cl_centre_index(i, e, g)] = Fs[e];
		A[lc_flag_index(i, g)] = act > 0 ? 1 : 0;
	}
	*out = p;
	*obj = q;
}
// object sphere s against the obstacles of the attachment, each with its own material: the world part of *obj
SAIP_LC_HD inline void lo_world(const LinkContactView& W, const LinkObjectGeom& OG, const double* OC, const double* OV, const double* pos, int g, int s,
								 LinkObjectPartial* obj) {
#pragma clang fp contract(off)
	const double cp[3] = {OC[lo_index(s, 0, g)], OC[lo_index(s, 1, g)], OC[lo_index(s, 2, g)]};
	const double vp[3] = {OV[lo_index(s, 0, g)], OV[lo_index(s, 1, g)], OV[lo_index(s, 2, g)]};
	double a[3];
	for (int e = 0; e < 3; e++) a[e] = cp[e] - pos[e];
	for (int o = 0; o < W.O; o++) {
		LinkContactItem it;
		lc_item(W.obst + (long long)o * LINK_CONTACT_OBSTACLE_WORDS * W.stride + W.col, W.stride, W.mat + LINK_CONTACT_MATERIAL_WORDS * o, cp, vp, OG.radius[s], &it);
		obj->wpen = lc_max(obj->wpen, lc_max(0.0, -it.d));
		if (!it.active) continue;
		double m[3];
		lo_cross(a, it.f, m);
		for (int e = 0; e < 3; e++) {
			obj->wf[e] = obj->wf[e] + it.f[e];
			obj->wm[e] = obj->wm[e] + m[e];
		}
	}
}
SAIP_LC_HD inline void lo_fold(LinkObjectPartial* v, const LinkObjectPartial& w) {
#pragma clang fp contract(off)
	for (int e = 0; e < 3; e++) {
		v->rf[e] = v->rf[e] + w.rf[e];
		v->rm[e] = v->rm[e] + w.rm[e];
		v->wf[e] = v->wf[e] + w.wf[e];
		v->wm[e] = v->wm[e] + w.wm[e];
	}
	v->fn_sum = v->fn_sum + w.fn_sum;
	v->wpen = lc_max(v->wpen, w.wpen);
	v->active = v->active + w.active;
	if (w.dmin < v->dmin || (w.dmin == v->dmin && w.k < v->k)) {
		v->dmin = w.dmin;
		v->k = w.k;
	}
}
// the readout of one instance: robot on object force 3 and moment 3, world on object force 3, smallest robot-object distance, its item,
// active robot-object items.  An invalid instance: NaN in every row.
SAIP_LC_HD inline void lo_readout(const LinkObjectPartial& v, bool bad, double* ro) {
	for (int e = 0; e < 3; e++) {
		ro[e] = bad ? (double)NAN : v.rf[e];
		ro[3 + e] = bad ? (double)NAN : v.rm[e];
		ro[6 + e] = bad ? (double)NAN : v.wf[e];
	}
	ro[9] = bad ? (double)NAN : v.dmin;
	ro[10] = bad ? (double)NAN : (double)v.k;
	ro[11] = bad ? (double)NAN : (double)v.active;
}
// The running summaries after one APPLY substep: sum dt sum f_n over the robot-object items (NaN is sticky), the largest robot-object
// penetration, the largest object-world penetration, substeps with an active robot-object item.  An invalid substep leaves rows 1 - 3.
SAIP_LC_HD inline void lo_summary_advance(double* s, long long ld, double dt, const LinkObjectPartial& v, bool bad) {
#pragma clang fp contract(off)
	s[0] = s[0] + dt * (bad ? (double)NAN : v.fn_sum);
	if (bad) return;
	s[ld] = lc_max(s[ld], lc_max(0.0, -v.dmin));
	s[2 * ld] = lc_max(s[2 * ld], v.wpen);
	s[3 * ld] = s[3 * ld] + (v.active > 0 ? 1.0 : 0.0);
}
// step 5: x (the 13 state words), in = { m, Ix, Iy, Iz }, grav the simulation's gravity, v the folded partial -> xn
SAIP_LC_HD inline void lo_integrate(const double* x, const double* in, const double* grav, double dt, const LinkObjectPartial& v, double* xn) {
#pragma clang fp contract(off)
	double R[9], T[3], tb[3], wb[3], y[3], db[3];
	lo_rotation(x + 3, R);
	for (int e = 0; e < 3; e++) {
		const double F = (in[0] * grav[e] + v.wf[e]) + v.rf[e];
		T[e] = v.wm[e] + v.rm[e];
		xn[7 + e] = x[7 + e] + dt * (F / in[0]);
	}
	const double* om = x + 10;
	for (int i = 0; i < 3; i++) {
		tb[i] = (R[i] * T[0] + R[3 + i] * T[1]) + R[6 + i] * T[2];
		wb[i] = (R[i] * om[0] + R[3 + i] * om[1]) + R[6 + i] * om[2];
	}
	y[0] = (in[3] - in[2]) * (wb[1] * wb[2]);
	y[1] = (in[1] - in[3]) * (wb[2] * wb[0]);
	y[2] = (in[2] - in[1]) * (wb[0] * wb[1]);
	for (int i = 0; i < 3; i++) db[i] = dt * ((tb[i] - y[i]) / in[1 + i]);
	for (int i = 0; i < 3; i++) xn[10 + i] = om[i] + ((R[3 * i] * db[0] + R[3 * i + 1] * db[1]) + R[3 * i + 2] * db[2]);
	for (int e = 0; e < 3; e++) xn[e] = x[e] + dt * xn[7 + e];
	const double qw = x[3], qx = x[4], qy = x[5], qz = x[6], ox = xn[10], oy = xn[11], oz = xn[12];
	const double d[4] = {-((ox * qx + oy * qy) + oz * qz), (ox * qw + oy * qz) - oz * qy, (oy * qw + oz * qx) - ox * qz, (oz * qw + ox * qy) - oy * qx};
	const double h = 0.5 * dt;
	double u[4];
	for (int i = 0; i < 4; i++) u[i] = x[3 + i] + h * d[i];
	const double len = sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]);
	for (int i = 0; i < 4; i++) xn[3 + i] = u[i] / len;
}
// cost + (w_pos |p - t|^2 + w_ori (1 - (q . qt)^2)), the orientation term only when has_quat; a state that is not finite: +inf
SAIP_LC_HD inline double lo_add_cost(double cost, const double* x, const double* tp, double w_pos, const double* tq, bool has_quat, double w_ori) {
#pragma clang fp contract(off)
	if (!lo_state_finite(x)) return (double)INFINITY;
	const double d[3] = {x[0] - tp[0], x[1] - tp[1], x[2] - tp[2]};
	double c = w_pos * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
	if (has_quat) {
		const double s = ((x[3] * tq[0] + x[4] * tq[1]) + x[5] * tq[2]) + x[6] * tq[3];
		c = c + w_ori * (1.0 - s * s);
	}
	return cost + c;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host form of one substep of one instance (group 0), in the kernel's shape: the eight lanes one after the other, the fold, the
// readouts, the new state.  C, V, F, A as lc_evaluate_host takes them; OC, OV: LINK_OBJECT_VEC_WORDS doubles of scratch.  ro_lc [8], ro_lo [12];
// xn receives the new state when *valid (else it is left alone).  Returns whether the robot's torque loop runs.
inline bool lo_step_host(const LinkContactView& W, const LinkObjectGeom& OG, const double* x, const double* in, const double* grav, double dt, const double* C,
						 const double* V, double* F, int* A, double* OC, double* OV, double* ro_lc, double* ro_lo, LinkObjectPartial* folded, double* xn, bool* valid) {
	double R[9];
	lo_rotation(x + 3, R);
	for (int s = 0; s < OG.P; s++) {
		double c[3], v[3];
		lo_sphere(x, R, OG.r[s], c, v);
		for (int e = 0; e < 3; e++) {
			OC[lo_index(s, e, 0)] = c[e];
			OV[lo_index(s, e, 0)] = v[e];
		}
	}
	LinkContactPartial v[LINK_CONTACT_LANES];
	LinkObjectPartial q[LINK_CONTACT_LANES];
	for (int l = 0; l < LINK_CONTACT_LANES; l++) {
		lo_partial_clear(&q[l]);
		lo_lane(W, OG, C, V, OC, OV, x, F, A, 0, l, &v[l], &q[l]);
		if (l < OG.P) lo_world(W, OG, OC, OV, x, 0, l, &q[l]);
	}
	for (int off = LINK_CONTACT_LANES / 2; off >= 1; off >>= 1)
		for (int l = 0; l < off; l++) {
			lc_fold(&v[l], v[l + off]);
			lo_fold(&q[l], q[l + off]);
		}
	lc_readout(v[0], ro_lc);
	const bool bad = v[0].bad || !lo_state_finite(x);
	lo_readout(q[0], bad, ro_lo);
	*folded = q[0];
	*valid = !bad;
	if (!bad) lo_integrate(x, in, grav, dt, q[0], xn);
	return !bad && v[0].active + q[0].active > 0;
}
#endif

// one launch of saip_link_object_apply: the link-contact launch it replaces, and the object's arrays.  Passed to the kernel by value.
struct LinkObjectParams {
	LinkContactParams lc;
	const LinkObjectGeom* geom;
	const double* inertial;      // [4] or [4][ld]
	int inertial_per_instance, pad_;
	double gravity[3];
	double* state;               // [13][ld]; APPLY advances it
	double* readout;             // [12][ld]
	double* summary;             // APPLY: [4][ld]
};

}  // namespace saip
