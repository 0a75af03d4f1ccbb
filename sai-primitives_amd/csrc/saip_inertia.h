// The resident inertia table of the simulator (saip_inertia.hip): the inertial parameters the integrators (saip_dynamics.hip,
// saip_dynamics_oct.hip) read in place of the model's when the simulated robot is not the controller's model -- link masses off by a factor,
// centres of mass displaced, a payload in the hand.  The per-instance arithmetic that composes a row from scaled links and payloads, shared
// by the kernel and by host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_plant.h).
//
// A row is INERTIA_ROW_WORDS words per movable body, in ModelDev's order: { m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz }, the centre of mass
// in the body frame, the inertia about it in body axes.  A body's parts are INERTIA_BODY_WORDS words { s, dx, dy, dz }:
//   m' = s m,  I' = s I,  c' = c + d                        (m, c, I the model's own)
// A payload is INERTIA_PAYLOAD_WORDS words { m_p, c_p (3), hx, hy, hz }: a uniform box of half-extents h, aligned with the frame of its site
// link, its centre at c_p in that frame; I_p = m_p / 3 diag(hy^2 + hz^2, hx^2 + hz^2, hx^2 + hy^2).  With (p_f, R_f) the site link's frame in
// its movable body and PA(d) = (d.d) 1 - d d^T, the body's row is
//   m = m' + sum m_p,  c = (m' c' + sum m_p (p_f + R_f c_p)) / m,  I = I' + m' PA(c' - c) + sum (R_f I_p R_f^T + m_p PA(p_f + R_f c_p - c))
// summed over the payloads with m_p > 0 on that body, in table order.  A body without such a payload takes m', c', I' as they are -- no
// sum, no division -- so s = 1, d = 0 returns the model's words bit for bit.
//
// Every function below rounds each product, sum and quotient on its own (no contraction into FMAs), in the order written, so that a NumPy
// restatement (tests/inertia_ref.py) reproduces it bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_sampler.h"

#if defined(__HIPCC__)
#define SAIP_IN_HD __host__ __device__
#else
#define SAIP_IN_HD
#endif

namespace saip {

enum { INERTIA_ROW_WORDS = 10, INERTIA_BODY_WORDS = 4, INERTIA_PAYLOAD_WORDS = 7, INERTIA_MAX_PAYLOADS = 2 };
enum { INERTIA_TABLE_BODIES = 2, INERTIA_TABLE_PAYLOADS = 3 };  // the table id inside the random-number counter (the plant's are 0 and 1)

// where a payload sits: the movable body of its site link and the link's frame in that body
struct InertiaSite {
	int body, pad_;
	double pos[3], rot[9];
};

// PA(d) as six words xx yy zz xy xz yz
SAIP_IN_HD inline void in_parallel_axis(const double* d, double* pa) {
#pragma clang fp contract(off)
	const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
	const double dd = (xx + yy) + zz;
	pa[0] = dd - xx;
	pa[1] = dd - yy;
	pa[2] = dd - zz;
	pa[3] = -(d[0] * d[1]);
	pa[4] = -(d[0] * d[2]);
	pa[5] = -(d[1] * d[2]);
}

// One row.  mdl: the model's ten words of body j, contiguous.  bw: the body's four words, bw[k * bstride].  pw: the first word of payload 0,
// word e of payload p at pw[(7 p + e) * pstride].  out: word k at out[k * ostride].
SAIP_IN_HD inline void in_compose_row(const double* mdl, const double* bw, long long bstride, int j, int n_payloads, const InertiaSite* site, const double* pw,
									   long long pstride, double* out, long long ostride) {
#pragma clang fp contract(off)
	const double s = bw[0];
	const double m1 = s * mdl[0];
	double c1[3], I1[6];
	for (int e = 0; e < 3; e++) c1[e] = mdl[1 + e] + bw[(1 + e) * bstride];
	for (int e = 0; e < 6; e++) I1[e] = s * mdl[4 + e];
	double mp[INERTIA_MAX_PAYLOADS], cp[INERTIA_MAX_PAYLOADS][3], Ip[INERTIA_MAX_PAYLOADS][6];
	int np = 0;
	for (int p = 0; p < n_payloads; p++) {
		const double* w = pw + (long long)p * INERTIA_PAYLOAD_WORDS * pstride;
		const double m = w[0];
		if (site[p].body != j || !(m > 0.0)) continue;
		const double* R = site[p].rot;
		const double cl[3] = {w[pstride], w[2 * pstride], w[3 * pstride]};
		const double hx = w[4 * pstride], hy = w[5 * pstride], hz = w[6 * pstride];
		for (int i = 0; i < 3; i++) cp[np][i] = site[p].pos[i] + ((R[3 * i] * cl[0] + R[3 * i + 1] * cl[1]) + R[3 * i + 2] * cl[2]);
		const double a = m / 3.0, xx = hx * hx, yy = hy * hy, zz = hz * hz;
		const double D[3] = {a * (yy + zz), a * (xx + zz), a * (xx + yy)};
		// R_f diag(D) R_f^T
		const int ri[6] = {0, 1, 2, 0, 0, 1}, rk[6] = {0, 1, 2, 1, 2, 2};
		for (int e = 0; e < 6; e++) {
			const double *a_ = R + 3 * ri[e], *b_ = R + 3 * rk[e];
			Ip[np][e] = ((a_[0] * D[0]) * b_[0] + (a_[1] * D[1]) * b_[1]) + (a_[2] * D[2]) * b_[2];
		}
		mp[np] = m;
		np++;
	}
	if (np == 0) {
		out[0] = m1;
		for (int e = 0; e < 3; e++) out[(1 + e) * ostride] = c1[e];
		for (int e = 0; e < 6; e++) out[(4 + e) * ostride] = I1[e];
		return;
	}
	double m = m1;
	for (int p = 0; p < np; p++) m = m + mp[p];
	double c[3];
	for (int e = 0; e < 3; e++) {
		double h = m1 * c1[e];
		for (int p = 0; p < np; p++) h = h + mp[p] * cp[p][e];
		c[e] = h / m;
	}
	double I[6], d[3], pa[6];
	for (int e = 0; e < 3; e++) d[e] = c1[e] - c[e];
	in_parallel_axis(d, pa);
	for (int e = 0; e < 6; e++) I[e] = I1[e] + m1 * pa[e];
	for (int p = 0; p < np; p++) {
		for (int e = 0; e < 3; e++) d[e] = cp[p][e] - c[e];
		in_parallel_axis(d, pa);
		for (int e = 0; e < 6; e++) I[e] = I[e] + (Ip[p][e] + mp[p] * pa[e]);
	}
	out[0] = m;
	for (int e = 0; e < 3; e++) out[(1 + e) * ostride] = c[e];
	for (int e = 0; e < 6; e++) out[(4 + e) * ostride] = I[e];
}

// The random draw of word `word` (its index inside the whole table: body j word k is 4 j + k, payload p word e is 7 p + e) of instance i:
// lo + u (hi - lo), u the first uniform of Philox counter (i, word, table id, round) under the 64-bit seed, clamped to the interval; lo == hi
// gives lo exactly (nothing is drawn).  The plant's scheme (pl_draw) under table ids of its own.
SAIP_IN_HD inline double in_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int table, int i, int word, double lo, double hi) {
#pragma clang fp contract(off)
	double v = lo;
	if (!(lo == hi)) {
		const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)word, (uint32_t)table, round}, key[2] = {seed_lo, seed_hi};
		uint32_t x[4];
		samp_philox4x32_10(ctr, key, x);
		const double u = samp_uniform(x[0], x[1]);
		v = lo + u * (hi - lo);
		const double a = lo < hi ? lo : hi, b = lo < hi ? hi : lo;
		v = v < a ? a : v;
		v = b < v ? b : v;
	}
	return v;
}

// one launch of saip_inertia_compose.  Passed to the kernel by value.  The words come from the part tables (draw = 0) or are drawn between
// the bound tables (draw = 1); either way the composition is in_compose_row.
struct ModelDev;
struct InertiaComposeParams {
	int cols, ld, n, n_payloads;     // cols: the columns to fill (B of a per-instance table, 1 of a batch-uniform one)
	int per_instance_bodies, per_instance_payloads, draw, pad_;
	uint32_t seed_lo, seed_hi, round, pad2_;
	long long stride;                // of `rows`: ld (per instance) or 1
	const ModelDev* model;
	const double* bodies;            // [n][4] or [n][4][ld]; draw: lower bounds [n][4]
	const double* bodies_hi;         // draw: upper bounds [n][4]
	const double* payloads;          // [P][7] or [P][7][ld]; draw: lower bounds [P][7]
	const double* payloads_hi;       // draw: upper bounds [P][7]
	double* rows;                    // [n][10] or [n][10][ld]
	InertiaSite site[INERTIA_MAX_PAYLOADS];
};

}  // namespace saip
