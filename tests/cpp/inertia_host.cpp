// The per-instance arithmetic of the resident inertia table (csrc/saip_inertia.h) compiled for the host as a stand-alone program: the rows of
// N instances composed from part tables, then the parts drawn between bound tables and composed again, read from / written to raw binary
// files.  Built and run by tests/test_inertia_cpu.py (once more with -fsanitize=address,undefined).  The model's rows and the payload sites
// are inputs: on the device they come from ModelDev and from the engine's link table.
//
// in:  int32[5] { N, J, P, per_instance_bodies, per_instance_payloads }, int32 site_body[P], then doubles: model rows [J][10], site pos
//      [P][3], site rot [P][9], bodies ([J][4][N] per instance, else [J][4]), payloads ([P][7][N] or [P][7]); then uint64 seed, uint32 round,
//      uint32 0, doubles body_lo[J][4], body_hi[J][4], payload_lo[P][7], payload_hi[P][7]
// out: doubles rows[J][10][N] from the tables, drawn bodies [J][4][N], drawn payloads [P][7][N], rows[J][10][N] from the draw
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_inertia.h"

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
	const int N = h[0], J = h[1], P = h[2], perb = h[3], perp = h[4];
	if (N < 1 || J < 1 || J > 32 || P < 0 || P > INERTIA_MAX_PAYLOADS) return 3;
	const size_t n = N;
	int32_t body[INERTIA_MAX_PAYLOADS] = {0, 0};
	if (P && fread(body, 4, P, f) != (size_t)P) return 4;
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	std::vector<double> mdl((size_t)J * INERTIA_ROW_WORDS), pos(3 * P), rot(9 * P), bodies((size_t)J * INERTIA_BODY_WORDS * (perb ? n : 1)),
		payloads((size_t)P * INERTIA_PAYLOAD_WORDS * (perp ? n : 1));
	if (!(rd(mdl) && rd(pos) && rd(rot) && rd(bodies) && rd(payloads))) return 4;
	InertiaSite site[INERTIA_MAX_PAYLOADS] = {};
	for (int p = 0; p < P; p++) {
		site[p].body = body[p];
		for (int e = 0; e < 3; e++) site[p].pos[e] = pos[3 * p + e];
		for (int e = 0; e < 9; e++) site[p].rot[e] = rot[9 * p + e];
	}
	uint64_t seed;
	uint32_t rnd[2];
	std::vector<double> blo((size_t)J * INERTIA_BODY_WORDS), bhi(blo.size()), plo((size_t)P * INERTIA_PAYLOAD_WORDS), phi(plo.size());
	if (fread(&seed, 8, 1, f) != 1 || fread(rnd, 4, 2, f) != 2 || !(rd(blo) && rd(bhi) && rd(plo) && rd(phi))) return 4;
	fclose(f);
	std::vector<double> rows((size_t)J * INERTIA_ROW_WORDS * n), rows2(rows.size()), db(blo.size() * n), dp(plo.size() * n);
	const long long bs = perb ? (long long)n : 1, ps = perp ? (long long)n : 1;
	for (size_t i = 0; i < n; i++) {
		for (int j = 0; j < J; j++)
			in_compose_row(mdl.data() + j * INERTIA_ROW_WORDS, bodies.data() + (long long)j * INERTIA_BODY_WORDS * bs + (perb ? (long long)i : 0), bs, j, P, site,
						   payloads.data() + (perp ? (long long)i : 0), ps, rows.data() + (size_t)j * INERTIA_ROW_WORDS * n + i, (long long)n);
		// the draw, as the kernel does it: the words of the instance into local arrays, then the same composition
		double pw[INERTIA_MAX_PAYLOADS * INERTIA_PAYLOAD_WORDS] = {};
		for (size_t w = 0; w < plo.size(); w++) dp[w * n + i] = pw[w] = in_draw((uint32_t)seed, (uint32_t)(seed >> 32), rnd[0], INERTIA_TABLE_PAYLOADS, (int)i, (int)w, plo[w], phi[w]);
		for (int j = 0; j < J; j++) {
			double bw[INERTIA_BODY_WORDS];
			for (int k = 0; k < INERTIA_BODY_WORDS; k++) {
				const int w = INERTIA_BODY_WORDS * j + k;
				db[w * n + i] = bw[k] = in_draw((uint32_t)seed, (uint32_t)(seed >> 32), rnd[0], INERTIA_TABLE_BODIES, (int)i, w, blo[w], bhi[w]);
			}
			in_compose_row(mdl.data() + j * INERTIA_ROW_WORDS, bw, 1, j, P, site, pw, 1, rows2.data() + (size_t)j * INERTIA_ROW_WORDS * n + i, (long long)n);
		}
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(rows) && wr(db) && wr(dp) && wr(rows2);
	fclose(f);
	return okw ? 0 : 6;
}
