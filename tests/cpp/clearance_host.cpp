// The per-instance arithmetic of the clearance monitor (csrc/saip_clearance.h) compiled for the host as a stand-alone program: N instances
// read from / written to raw binary files.  Built and run by tests/test_clearance_cpu.py (once more with -fsanitize=address,undefined).
//
// in:  int32[5] { N, S, O, P, per_instance }, int32 pairs[P][2], then doubles: margin, dt, period, w_penalty, w_collision, d_safe,
//      centres[N][S][3], radii[S], obstacles ([O][8][N] per instance, else [O][8]), summary[4][N], cost[N], o[N][3], R[N][9], r[N][3]
// out: doubles readout[N][8], summary[4][N] (advanced once with rows 0 and 2 of the readout), cost[N] (after add_cost on the advanced
//      summaries), c[N][3] = o + R r
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_clearance.h"

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
	const int N = h[0], S = h[1], O = h[2], P = h[3], per = h[4];
	if (N < 1 || S < 1 || S > CLEARANCE_MAX_SPHERES || O < 0 || O > CLEARANCE_MAX_OBSTACLES || P < 0 || P > CLEARANCE_MAX_PAIRS) return 3;
	std::vector<int32_t> pairs(2 * (size_t)P);
	if (P && fread(pairs.data(), 4, pairs.size(), f) != pairs.size()) return 3;
	double sc[6];
	if (fread(sc, 8, 6, f) != 6) return 3;
	const double margin = sc[0], dt = sc[1], period = sc[2], w_penalty = sc[3], w_collision = sc[4], d_safe = sc[5];
	const size_t n = N;
	std::vector<double> centres(n * S * 3), radii(S), obst((size_t)O * CLEARANCE_OBSTACLE_WORDS * (per ? n : 1)), summary(CLEARANCE_SUMMARY_ROWS * n), cost(n),
		o(3 * n), R(9 * n), r(3 * n);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	const bool ok = rd(centres) && rd(radii) && rd(obst) && rd(summary) && rd(cost) && rd(o) && rd(R) && rd(r);
	fclose(f);
	if (!ok) return 4;
	ClearanceGeom G;
	memset(&G, 0, sizeof(G));
	G.S = S;
	G.O = O;
	G.P = P;
	for (int s = 0; s < S; s++) {
		G.slot[s] = s;
		G.radius[s] = radii[s];
	}
	for (int p = 0; p < P; p++) {
		if (pairs[2 * p] < 0 || pairs[2 * p] >= S || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= S) return 3;
		G.pair[p][0] = (uint8_t)pairs[2 * p];
		G.pair[p][1] = (uint8_t)pairs[2 * p + 1];
	}
	std::vector<double> readout(CLEARANCE_READOUT_ROWS * n), c(3 * n), C(CLEARANCE_CENTRE_WORDS);
	for (size_t i = 0; i < n; i++) {
		for (int s = 0; s < S; s++)
			for (int e = 0; e < 3; e++) C[cl_centre_index(s, e, 0)] = centres[(i * S + s) * 3 + e];
		double* ro = &readout[CLEARANCE_READOUT_ROWS * i];
		cl_evaluate_host(G, obst.data(), per ? (long long)n : 1, per ? (long long)i : 0, margin, C.data(), ro);
		cl_summary_advance(&summary[i], (long long)n, dt, ro[0], ro[2], period);
		cost[i] = cl_add_cost(cost[i], summary[i], summary[n + i], w_penalty, w_collision, d_safe);
		cl_centre(&o[3 * i], &R[9 * i], &r[3 * i], &c[3 * i]);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(readout) && wr(summary) && wr(cost) && wr(c);
	fclose(f);
	return okw ? 0 : 6;
}
