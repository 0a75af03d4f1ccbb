// The per-instance arithmetic of the pushed object (csrc/saip_link_object.h) compiled for the host as a stand-alone program: N instances,
// one APPLY substep each, read from / written to raw binary files.  Built and run by tests/test_link_object_cpu.py (once more with
// -fsanitize=address,undefined).
//
// in:  int32[7] { N, S, O, n, per_instance (obstacles), P, per_instance (inertial) }, int32 order[S], uint32 anc[S], int32 jtype[n], then
//      doubles: dt, gravity[3], w_pos, w_ori, has_quat, target_p[3], target_quat[4], centres[N][S][3], velocities[N][S][3], radii[S],
//      obstacles ([O][8][N] per instance, else [O][8]), materials[O][4], aw[N][n][3], oj[N][n][3], tau_cmd[N][n], link-contact summary[4][N],
//      object summary[4][N], cost[N], shape r[P][3], shape radius[P], object material[4], inertial ([4][N] per instance, else [4]),
//      state[13][N]
// out: doubles link-contact readout[N][8], object readout[N][12], F[N][S][3] (by sphere), tau_sim[N][n], link-contact summary[4][N] and
//      object summary[4][N] (advanced once), state[13][N] (advanced once where valid), cost[N] (add_cost on the new state)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_link_object.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[7];
	if (fread(h, 4, 7, f) != 7) return 3;
	const int N = h[0], S = h[1], O = h[2], nj = h[3], per = h[4], P = h[5], per_in = h[6];
	if (N < 1 || S < 1 || S > LINK_CONTACT_MAX_SPHERES || O < 1 || O > LINK_CONTACT_MAX_OBSTACLES || nj < 1 || nj > LINK_CONTACT_MAX_JOINTS || P < 1 ||
		P > LINK_OBJECT_MAX_SPHERES)
		return 3;
	std::vector<int32_t> order(S), jtype(nj);
	std::vector<uint32_t> anc(S);
	if (fread(order.data(), 4, S, f) != (size_t)S || fread(anc.data(), 4, S, f) != (size_t)S || fread(jtype.data(), 4, nj, f) != (size_t)nj) return 3;
	double sc[14];
	if (fread(sc, 8, 14, f) != 14) return 3;
	const double dt = sc[0], *grav = sc + 1, w_pos = sc[4], w_ori = sc[5], *tp = sc + 7, *tq = sc + 10;
	const bool has_quat = sc[6] != 0.0;
	const size_t n = N;
	std::vector<double> centres(n * S * 3), vels(n * S * 3), radii(S), obst((size_t)O * LINK_CONTACT_OBSTACLE_WORDS * (per ? n : 1)), mat((size_t)O * LINK_CONTACT_MATERIAL_WORDS),
		aw(n * nj * 3), oj(n * nj * 3), tau_cmd(n * nj), summary(LINK_CONTACT_SUMMARY_ROWS * n), osummary(LINK_OBJECT_SUMMARY_ROWS * n), cost(n), shape_r((size_t)P * 3),
		shape_radius(P), omat(LINK_CONTACT_MATERIAL_WORDS), inertial((size_t)LINK_OBJECT_INERTIAL_WORDS * (per_in ? n : 1)), state(LINK_OBJECT_STATE_ROWS * n);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	const bool ok = rd(centres) && rd(vels) && rd(radii) && rd(obst) && rd(mat) && rd(aw) && rd(oj) && rd(tau_cmd) && rd(summary) && rd(osummary) && rd(cost) &&
					rd(shape_r) && rd(shape_radius) && rd(omat) && rd(inertial) && rd(state);
	fclose(f);
	if (!ok) return 4;
	int slot[LINK_CONTACT_MAX_SPHERES];
	double radius[LINK_CONTACT_MAX_SPHERES];
	for (int i = 0; i < S; i++) {
		if (order[i] < 0 || order[i] >= S) return 3;
		slot[i] = order[i];
		radius[i] = radii[order[i]];
	}
	LinkObjectGeom OG;
	memset(&OG, 0, sizeof(OG));
	OG.P = P;
	for (int s = 0; s < P; s++) {
		for (int e = 0; e < 3; e++) OG.r[s][e] = shape_r[3 * s + e];
		OG.radius[s] = shape_radius[s];
	}
	for (int k = 0; k < LINK_CONTACT_MATERIAL_WORDS; k++) OG.mat[k] = omat[k];
	std::vector<double> readout(LINK_CONTACT_READOUT_ROWS * n), oreadout(LINK_OBJECT_READOUT_ROWS * n), Fout(n * S * 3), tau(n * nj), C(LINK_CONTACT_VEC_WORDS),
		V(LINK_CONTACT_VEC_WORDS), F(LINK_CONTACT_VEC_WORDS), OC(LINK_OBJECT_VEC_WORDS), OV(LINK_OBJECT_VEC_WORDS);
	std::vector<int> A(LINK_CONTACT_FLAG_WORDS);
	for (size_t b = 0; b < n; b++) {
		for (int i = 0; i < S; i++)
			for (int e = 0; e < 3; e++) {
				C[cl_centre_index(i, e, 0)] = centres[(b * S + slot[i]) * 3 + e];
				V[cl_centre_index(i, e, 0)] = vels[(b * S + slot[i]) * 3 + e];
			}
		LinkContactView W;
		W.S = S;
		W.O = O;
		W.slot = slot;
		W.radius = radius;
		W.obst = obst.data();
		W.stride = per ? (long long)n : 1;
		W.col = per ? (long long)b : 0;
		W.mat = mat.data();
		double x[LINK_OBJECT_STATE_ROWS], xn[LINK_OBJECT_STATE_ROWS], in[LINK_OBJECT_INERTIAL_WORDS];
		for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) x[r] = state[r * n + b];
		for (int r = 0; r < LINK_OBJECT_INERTIAL_WORDS; r++) in[r] = per_in ? inertial[r * n + b] : inertial[r];
		double* ro = &readout[LINK_CONTACT_READOUT_ROWS * b];
		LinkObjectPartial q;
		bool valid = false;
		const bool run = lo_step_host(W, OG, x, in, grav, dt, C.data(), V.data(), F.data(), A.data(), OC.data(), OV.data(), ro, &oreadout[LINK_OBJECT_READOUT_ROWS * b], &q, xn, &valid);
		for (int i = 0; i < S; i++)
			for (int e = 0; e < 3; e++) Fout[(b * S + slot[i]) * 3 + e] = F[cl_centre_index(i, e, 0)];
		for (int j = 0; j < nj; j++) {
			const double u0 = lc_u0(tau_cmd[b * nj + j]);
			tau[b * nj + j] = run ? lc_tau(u0, lc_joint_sum(S, anc.data(), j, jtype[j], &aw[(b * nj + j) * 3], &oj[(b * nj + j) * 3], C.data(), F.data(), A.data(), 0)) : u0;
		}
		lc_summary_advance(&summary[b], (long long)n, dt, ro);
		lo_summary_advance(&osummary[b], (long long)n, dt, q, !valid);
		if (valid)
			for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) state[r * n + b] = xn[r];
		for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) x[r] = state[r * n + b];
		cost[b] = lo_add_cost(cost[b], x, tp, w_pos, tq, has_quat, w_ori);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(readout) && wr(oreadout) && wr(Fout) && wr(tau) && wr(summary) && wr(osummary) && wr(state) && wr(cost);
	fclose(f);
	return okw ? 0 : 6;
}
