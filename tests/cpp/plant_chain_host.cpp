// The per-element arithmetic of the actuation chain (csrc/saip_plant_chain.h) compiled for the host as a stand-alone program: P periods of
// S substeps of N instances x J joints through pc_step, the state kept in the device's layout ([rows][N], one column per instance), then one
// random draw of the per-instance table, read from / written to raw binary files.  Built and run by tests/test_plant_chain_cpu.py (once
// more with -fsanitize=address,undefined).
//
// in:  int32[6] { N, J, depth, per_instance, P, S }, then doubles: table ([J][3][N] per instance, else [J][3]), dt[S] (the substeps'
//      lengths) and per period the command t[J][N]; then uint64 draw seed, uint32 round, uint32 0, doubles lo[J][3], hi[J][3]
// out: doubles, per period and substep what pl_joint gets, [J][N]; then the final state taps[J][depth][N], filt[J][3][N], primed[J][N] (as
//      doubles); then the drawn table [J][3][N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_plant_chain.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[6];
	if (fread(h, 4, 6, f) != 6) return 3;
	const int N = h[0], J = h[1], depth = h[2], per = h[3], P = h[4], S = h[5];
	if (N < 1 || J < 1 || J > 32 || depth < 0 || depth > PLANT_CHAIN_MAX_DEPTH || P < 0 || S < 1 || S > 16) return 3;
	const size_t n = N;
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	std::vector<double> table((size_t)J * PLANT_CHAIN_WORDS * (per ? n : 1)), dts(S);
	if (!(rd(table) && rd(dts))) return 4;
	// exactly the sizes the engine allocates: an access past a row's taps is an access past the vector for the last joint
	std::vector<double> taps((size_t)J * depth * n, 0.0), filt((size_t)J * PLANT_CHAIN_FILT_ROWS * n, 0.0), t(J * n), out((size_t)P * S * J * n);
	std::vector<int> primed((size_t)J * n, 0);
	const long long cs = per ? (long long)n : 1;
	for (int k = 0; k < P; k++) {
		if (!rd(t)) return 4;
		for (int s = 0; s < S; s++) {
			double* o = out.data() + ((size_t)k * S + s) * J * n;
			for (int j = 0; j < J; j++)
				for (size_t i = 0; i < n; i++)
					o[j * n + i] = pc_step(table.data() + (long long)j * PLANT_CHAIN_WORDS * cs + (per ? (long long)i : 0), cs, depth, depth > 0 ? taps.data() + (size_t)j * depth * n + i : nullptr,
										   filt.data() + (size_t)j * PLANT_CHAIN_FILT_ROWS * n + i, &primed[j * n + i], (long long)n, t[j * n + i], dts[s], s == 0);
		}
	}
	uint64_t dseed;
	uint32_t rnd[2];
	std::vector<double> lo(J * PLANT_CHAIN_WORDS), hi(lo.size());
	if (fread(&dseed, 8, 1, f) != 1 || fread(rnd, 4, 2, f) != 2 || !(rd(lo) && rd(hi))) return 4;
	fclose(f);
	std::vector<double> drawn(lo.size() * n), pr(primed.begin(), primed.end());
	for (size_t i = 0; i < n; i++)
		for (size_t w = 0; w < lo.size(); w++) drawn[w * n + i] = pc_draw((uint32_t)dseed, (uint32_t)(dseed >> 32), rnd[0], (int)i, (int)w, lo[w], hi[w], depth);
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(out) && wr(taps) && wr(filt) && wr(pr) && wr(drawn);
	fclose(f);
	return okw ? 0 : 6;
}
