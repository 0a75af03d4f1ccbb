// The scenario groups of the resident rollout sampler (csrc/saip_sampler.h) compiled for the host as a stand-alone program: one grouped
// perturb -> group cost -> weights -> best map -> update pass over small arrays read from / written to raw binary files, in the order
// and with the arguments saip_batch_sampler_perturb / _update use.  Built and run by tests/test_sampler_scenarios_cpu.py (once more with
// -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_sampler.h"

using namespace saip;

// in:  int32[12] { C, M, ld, K, count, rot, r_rot, task, exempt, round, risk, tail } uint64 seed, double temperature,
//      nominal[K][count], sigma[d], cost_in[C M]
// out: key[K][count][ld] (perturbed; padding columns keep the sentinel), group[ld] (C entries written; with M = 1 the costs themselves, as
//      the engine takes them), weights[ld] (C entries written), best_map[ld] (as doubles, C M entries written), result { best, n_valid,
//      min_cost, sum_w, ess } (as doubles), nominal after the update [K][count]
static int run(const char* in_path, const char* out_path) {
	FILE* f = fopen(in_path, "rb");
	if (!f) return 2;
	int32_t h[12];
	unsigned long long seed;
	double temperature;
	bool ok = fread(h, 4, 12, f) == 12 && fread(&seed, 8, 1, f) == 1 && fread(&temperature, 8, 1, f) == 1;
	if (!ok) return 3;
	const int C = h[0], M = h[1], ld = h[2], K = h[3], count = h[4], rot = h[5], r_rot = h[6], risk = h[10], tail = h[11];
	const int B = C * M, d = rot ? count - 6 : count;
	if (C < 1 || M < 1 || M > SAMP_MAX_SCENARIOS || ld < B || count > SAMP_MAX_ROWS) return 3;
	const double SENTINEL = 6.02214076e23;
	std::vector<double> nominal((size_t)K * count), sigma(d), cost_in(B);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	ok = rd(nominal) && rd(sigma) && rd(cost_in);
	fclose(f);
	if (!ok) return 4;
	std::vector<double> key((size_t)K * count * ld, SENTINEL), group(ld, SENTINEL), w(ld, SENTINEL), map_d(ld, SENTINEL);
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
	E.task = h[7];
	E.exempt = h[8];
	samp_host_perturb_grouped(E, ld, B, C, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)h[9]);
	if (M == 1)
		for (int c = 0; c < C; c++) group[c] = cost_in[c];
	else samp_host_group_cost(cost_in.data(), C, M, risk, tail, group.data());
	SamplerResult res;
	samp_host_weights(group.data(), C, temperature, w.data(), &res, best_map.data());
	if (M > 1) samp_host_group_map(B, C, res.best, best_map.data());
	for (int i = 0; i < B; i++) map_d[i] = best_map[i];
	const std::vector<double> perturbed = key;
	samp_host_update(E, ld, C, w.data(), res);
	f = fopen(out_path, "wb");
	if (!f) return 5;
	const double r5[5] = {(double)res.best, (double)res.n_valid, res.min_cost, res.sum_w, res.ess};
	auto wr = [&](const std::vector<double>& v) { return v.empty() || fwrite(v.data(), 8, v.size(), f) == v.size(); };
	ok = wr(perturbed) && wr(group) && wr(w) && wr(map_d) && fwrite(r5, 8, 5, f) == 5 && wr(nominal);
	fclose(f);
	return ok ? 0 : 6;
}

int main(int argc, char** argv) {
	if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
	fprintf(stderr, "usage: %s run in.bin out.bin\n", argv[0]);
	return 1;
}
