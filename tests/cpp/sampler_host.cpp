// The per-element code of the resident rollout sampler (csrc/saip_sampler.h) compiled for the host as a stand-alone program: the Philox
// known answers, the uniforms of one counter, and one perturb -> cost -> update -> shift pass over small arrays read from / written to
// raw binary files.  Built and run by tests/test_sampler_cpu.py (once more with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_sampler.h"

using namespace saip;

static int philox() {
	const uint32_t ctr[3][4] = {{0, 0, 0, 0}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
	const uint32_t key[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
	for (int t = 0; t < 3; t++) {
		uint32_t w[4];
		samp_philox4x32_10(ctr[t], key[t], w);
		printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
	}
	return 0;
}
// words and uniforms (as bit patterns) of counter (i, k, (task << 16) | p, round)
static int uniforms(char** a) {
	const unsigned long long seed = strtoull(a[0], nullptr, 0);
	const uint32_t round = (uint32_t)strtoul(a[1], nullptr, 0);
	const int task = atoi(a[2]), i = atoi(a[3]), k = atoi(a[4]), p = atoi(a[5]);
	const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)k, ((uint32_t)task << 16) | (uint32_t)p, round}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
	uint32_t w[4];
	samp_philox4x32_10(ctr, key, w);
	double u[2];
	samp_uniforms(key[0], key[1], round, task, i, k, p, u);
	uint64_t bits[2];
	memcpy(bits, u, sizeof(bits));
	printf("%08x %08x %08x %08x %016llx %016llx\n", w[0], w[1], w[2], w[3], (unsigned long long)bits[0], (unsigned long long)bits[1]);
	return 0;
}

// in:  int32[16] { B, ld, K, count, rot, r_rot, task, exempt, round, capacity, first_slot, n_samples, rows, pose_row0, has_target,
//      has_summary } uint64 seed, double temperature, w[8], target[3], w_path, w_final, int32 shift, int32 pad,
//      nominal[K][count], sigma[d], summary[8][ld], log[capacity][rows][ld], cost_in[B]
// out: key[K][count][ld] (perturbed; padding columns keep the sentinel), cost[ld] (the cost kernel's), weights[ld], best_map[ld] (as
//      doubles), result { best, n_valid, min_cost, sum_w, ess } (as doubles), nominal after the update [K][count], after the shift
static int run(const char* in_path, const char* out_path) {
	FILE* f = fopen(in_path, "rb");
	if (!f) return 2;
	int32_t h[16];
	unsigned long long seed;
	double temperature, wts[8], target[3], w_path, w_final;
	int32_t shift[2];
	bool ok = fread(h, 4, 16, f) == 16 && fread(&seed, 8, 1, f) == 1 && fread(&temperature, 8, 1, f) == 1 && fread(wts, 8, 8, f) == 8 &&
			  fread(target, 8, 3, f) == 3 && fread(&w_path, 8, 1, f) == 1 && fread(&w_final, 8, 1, f) == 1 && fread(shift, 4, 2, f) == 2;
	if (!ok) return 3;
	const int B = h[0], ld = h[1], K = h[2], count = h[3], rot = h[4], r_rot = h[5];
	const int d = rot ? count - 6 : count;
	const double SENTINEL = 6.02214076e23;
	std::vector<double> nominal((size_t)K * count), sigma(d), summary((size_t)8 * ld), log((size_t)h[9] * h[12] * ld), cost_in(B);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	ok = rd(nominal) && rd(sigma) && rd(summary) && rd(log) && rd(cost_in);
	fclose(f);
	if (!ok) return 4;
	std::vector<double> key((size_t)K * count * ld, SENTINEL), cost(ld, SENTINEL), w(ld, SENTINEL), map_d(ld, SENTINEL);
	std::vector<int> best_map(ld, 0);
	SamplerEntry E;
	memset(&E, 0, sizeof(E));
	E.key = key.data();
	E.nominal = nominal.data();
	E.sigma = sigma.data();
	E.count = count;
	E.K = K;
	E.d = d;
	E.rot = rot;
	E.r_rot = r_rot;
	E.task = h[6];
	E.exempt = h[7];
	for (int i = 0; i < B; i++) samp_perturb_instance(E, ld, i, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)h[8]);
	SamplerCostParams P;
	memset(&P, 0, sizeof(P));
	P.B = B;
	P.ld = ld;
	P.summary = h[15] ? summary.data() : nullptr;
	P.log = log.data();
	P.rows = h[12];
	P.pose_row0 = h[13];
	P.capacity = h[9];
	P.first_slot = h[10];
	P.n_samples = h[11];
	P.has_target = h[14];
	for (int r = 0; r < 8; r++) P.w[r] = wts[r];
	for (int e = 0; e < 3; e++) P.target[e] = target[e];
	P.w_path = w_path;
	P.w_final = w_final;
	P.cost = cost.data();
	for (int i = 0; i < B; i++) cost[i] = samp_cost_instance(P, i);
	SamplerResult res;
	samp_host_weights(cost_in.data(), B, temperature, w.data(), &res, best_map.data());
	for (int i = 0; i < B; i++) map_d[i] = best_map[i];
	const std::vector<double> perturbed = key;
	samp_host_update(E, ld, B, w.data(), res);
	const std::vector<double> updated = nominal;
	for (int c = 0; c < count && shift[0] > 0; c++) samp_shift_column(nominal.data(), K, count, shift[0], c);
	f = fopen(out_path, "wb");
	if (!f) return 5;
	const double r5[5] = {(double)res.best, (double)res.n_valid, res.min_cost, res.sum_w, res.ess};
	auto wr = [&](const std::vector<double>& v) { return v.empty() || fwrite(v.data(), 8, v.size(), f) == v.size(); };
	ok = wr(perturbed) && wr(cost) && wr(w) && wr(map_d) && fwrite(r5, 8, 5, f) == 5 && wr(updated) && wr(nominal);
	fclose(f);
	return ok ? 0 : 6;
}

int main(int argc, char** argv) {
	if (argc == 2 && !strcmp(argv[1], "philox")) return philox();
	if (argc == 8 && !strcmp(argv[1], "uniforms")) return uniforms(argv + 2);
	if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
	fprintf(stderr, "usage: %s philox | uniforms seed round task i k p | run in.bin out.bin\n", argv[0]);
	return 1;
}
