// The per-instance arithmetic of link contact (csrc/saip_link_contact.h) compiled for the host as a stand-alone program: N instances read
// from / written to raw binary files.  Built and run by tests/test_link_contact_cpu.py (once more with -fsanitize=address,undefined).
//
// in:  int32[5] { N, S, O, n, per_instance }, int32 order[S] (sorted position -> sphere), uint32 anc[S] (by sorted position), int32 jtype[n],
//      then doubles: dt, w_impulse, w_peak, centres[N][S][3], velocities[N][S][3], radii[S] (by sphere), obstacles ([O][8][N] per instance,
//      else [O][8]), materials[O][4], aw[N][n][3], oj[N][n][3], tau_cmd[N][n], summary[4][N], cost[N]
// out: doubles readout[N][8], F[N][S][3] (by sphere), tau_sim[N][n], summary[4][N] (advanced once), cost[N] (after add_cost on the
//      advanced summaries)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_link_contact.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[5];
	if (fread(h, 4, 5, f) != 5) return 3;
	const int N = h[0], S = h[1], O = h[2], nj = h[3], per = h[4];
	if (N < 1 || S < 1 || S > LINK_CONTACT_MAX_SPHERES || O < 1 || O > LINK_CONTACT_MAX_OBSTACLES || nj < 1 || nj > LINK_CONTACT_MAX_JOINTS) return 3;
	std::vector<int32_t> order(S), jtype(nj);
	std::vector<uint32_t> anc(S);
	if (fread(order.data(), 4, S, f) != (size_t)S || fread(anc.data(), 4, S, f) != (size_t)S || fread(jtype.data(), 4, nj, f) != (size_t)nj) return 3;
	double sc[3];
	if (fread(sc, 8, 3, f) != 3) return 3;
	const double dt = sc[0], w_impulse = sc[1], w_peak = sc[2];
	const size_t n = N;
	std::vector<double> centres(n * S * 3), vels(n * S * 3), radii(S), obst((size_t)O * LINK_CONTACT_OBSTACLE_WORDS * (per ? n : 1)), mat((size_t)O * LINK_CONTACT_MATERIAL_WORDS),
		aw(n * nj * 3), oj(n * nj * 3), tau_cmd(n * nj), summary(LINK_CONTACT_SUMMARY_ROWS * n), cost(n);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	const bool ok = rd(centres) && rd(vels) && rd(radii) && rd(obst) && rd(mat) && rd(aw) && rd(oj) && rd(tau_cmd) && rd(summary) && rd(cost);
	fclose(f);
	if (!ok) return 4;
	int slot[LINK_CONTACT_MAX_SPHERES];
	double radius[LINK_CONTACT_MAX_SPHERES];
	for (int i = 0; i < S; i++) {
		if (order[i] < 0 || order[i] >= S) return 3;
		slot[i] = order[i];
		radius[i] = radii[order[i]];
	}
	std::vector<double> readout(LINK_CONTACT_READOUT_ROWS * n), Fout(n * S * 3), tau(n * nj), C(LINK_CONTACT_VEC_WORDS), V(LINK_CONTACT_VEC_WORDS), F(LINK_CONTACT_VEC_WORDS);
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
		double* ro = &readout[LINK_CONTACT_READOUT_ROWS * b];
		const bool run = lc_evaluate_host(W, C.data(), V.data(), F.data(), A.data(), ro);
		for (int i = 0; i < S; i++)
			for (int e = 0; e < 3; e++) Fout[(b * S + slot[i]) * 3 + e] = F[cl_centre_index(i, e, 0)];
		for (int j = 0; j < nj; j++) {
			const double u0 = lc_u0(tau_cmd[b * nj + j]);
			tau[b * nj + j] = run ? lc_tau(u0, lc_joint_sum(S, anc.data(), j, jtype[j], &aw[(b * nj + j) * 3], &oj[(b * nj + j) * 3], C.data(), F.data(), A.data(), 0)) : u0;
		}
		lc_summary_advance(&summary[b], (long long)n, dt, ro);
		cost[b] = lc_add_cost(cost[b], summary[b], summary[n + b], w_impulse, w_peak);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(readout) && wr(Fout) && wr(tau) && wr(summary) && wr(cost);
	fclose(f);
	return okw ? 0 : 6;
}
