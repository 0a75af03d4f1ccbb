// What a lane of the resident guards decides (csrc/saip_guard.h) compiled for the host as a stand-alone program: K evaluations of N
// instances through gd_step, the state kept in the device's layout ([rows][N], one column per instance), read from / written to raw binary
// files.  Built and run by tests/test_guard_cpu.py (once more with -fsanitize=address,undefined).
//
// in:  int32[8] { N, G, P, per_instance, K, have_pose, 0, 0 }, then doubles: guards ([G][8][N] per instance, else [G][8]), phases [P][4],
//      the goal rows [24][N] before the first evaluation, then per evaluation f[3][N], m[3][N], pos[3][N], ep[N], eo[N], speed[N], pose[12][N];
//      then cost[N], w_time, w_miss and int32 phase, 0 for one gd_cost
// out: doubles, per evaluation phase[N], since[N], clock[N], run[G][N], entry[P][N], fires[G][N] (as doubles), latch[12][N], goal[24][N];
//      then the cost [N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_guard.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[8];
	if (fread(h, 4, 8, f) != 8) return 3;
	const int N = h[0], G = h[1], P = h[2], per = h[3], K = h[4], have_pose = h[5];
	if (N < 1 || G < 1 || G > GUARD_MAX_GUARDS || P < 1 || P > GUARD_MAX_PHASES || K < 0) return 3;
	const size_t n = N;
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	// exactly the sizes the engine allocates: an access past a row is an access past the vector for the last row
	std::vector<double> guards((size_t)G * GUARD_WORDS * (per ? n : 1)), phases((size_t)P * GUARD_PHASE_WORDS), goal(24 * n), latch(GUARD_LATCH_ROWS * n, 0.0);
	if (!(rd(guards) && rd(phases) && rd(goal))) return 4;
	std::vector<int> phase(n, 0), since(n, 0), clock(n, 0), run((size_t)G * n, 0), entry((size_t)P * n, -1), fires((size_t)G * n, 0);
	for (size_t i = 0; i < n; i++) entry[i] = 0;
	std::vector<double> in(24 * n), out;
	const long long gstride = per ? (long long)n : 1;
	for (int k = 0; k < K; k++) {
		if (!rd(in)) return 4;
		for (size_t i = 0; i < n; i++) {
			GuardSignals S;
			double pose[GUARD_LATCH_ROWS];
			for (int e = 0; e < 3; e++) {
				S.f[e] = in[(size_t)e * n + i];
				S.m[e] = in[(size_t)(3 + e) * n + i];
				S.pos[e] = in[(size_t)(6 + e) * n + i];
			}
			S.ep = in[9 * n + i];
			S.eo = in[10 * n + i];
			S.speed = in[11 * n + i];
			for (int e = 0; e < GUARD_LATCH_ROWS; e++) pose[e] = in[(size_t)(12 + e) * n + i];
			gd_step(guards.data() + (per ? i : 0), gstride, G, phases.data(), P, S, pose, have_pose != 0, &phase[i], &since[i], &clock[i], &run[i], &entry[i], &fires[i],
					&latch[i], (long long)n, &goal[i], (long long)n);
		}
		for (const std::vector<int>* a : {&phase, &since, &clock, &run, &entry, &fires}) out.insert(out.end(), a->begin(), a->end());
		out.insert(out.end(), latch.begin(), latch.end());
		out.insert(out.end(), goal.begin(), goal.end());
	}
	std::vector<double> cost(n), w(2);
	int32_t cp[2];
	if (!(rd(cost) && rd(w)) || fread(cp, 4, 2, f) != 2 || cp[0] < 0 || cp[0] >= P) return 4;
	fclose(f);
	for (size_t i = 0; i < n; i++) out.push_back(gd_cost(cost[i], entry[(size_t)cp[0] * n + i], w[0], w[1]));
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	const bool okw = out.empty() || fwrite(out.data(), 8, out.size(), f) == out.size();
	fclose(f);
	return okw ? 0 : 6;
}
