// The per-element arithmetic of the sensing model (csrc/saip_sense.h) compiled for the host as a stand-alone program: P periods of N
// instances (joint measurements and the wrenches of S slots), the raw normals of the joint rows, then one random draw of the per-instance
// tables, read from / written to raw binary files.  Built and run by tests/test_sensing_cpu.py (once more with
// -fsanitize=address,undefined).  Period k of the input belongs to period p0 + k of the noise counter.
//
// in:  int32[6] { N, J, S, per_instance_joints, per_instance_wrenches, P }, uint32 p0, uint32 0, uint64 seed, then doubles: joints
//      ([J][6][N] per instance, else [J][6]), wrenches ([S][6][3][N] or [S][6][3]), and per period q[J][N], dq[J][N], f[S][6][N];
//      then uint64 draw seed, uint32 round, uint32 0, doubles joint_lo[J][6], joint_hi[J][6], wrench_lo[S][18], wrench_hi[S][18]
// out: doubles, per period q_meas[J][N], dq_meas[J][N], f_meas[S][6][N]; then z[P][J][2][N] (the normals of the joint rows, drawn whatever
//      the sigmas); then the drawn joints [J][6][N] and wrenches [S][18][N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_sense.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[6];
	uint32_t p0[2];
	uint64_t seed;
	if (fread(h, 4, 6, f) != 6 || fread(p0, 4, 2, f) != 2 || fread(&seed, 8, 1, f) != 1) return 3;
	const int N = h[0], J = h[1], S = h[2], perj = h[3], perw = h[4], P = h[5];
	if (N < 1 || J < 1 || J > 32 || S < 0 || S > SENSE_MAX_WRENCH_TASKS || P < 0) return 3;
	const size_t n = N;
	const uint32_t slo = (uint32_t)seed, shi = (uint32_t)(seed >> 32);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	std::vector<double> joints((size_t)J * SENSE_JOINT_WORDS * (perj ? n : 1)), wrenches((size_t)S * SENSE_WRENCH_WORDS * (perw ? n : 1));
	if (!(rd(joints) && rd(wrenches))) return 4;
	const size_t per_period = (size_t)(2 * J + 6 * S) * n;
	std::vector<double> out(per_period * P), z((size_t)P * J * 2 * n), q(J * n), dq(J * n), fw(6 * S * n);
	const long long js = perj ? (long long)n : 1, ws = perw ? (long long)n : 1;
	for (int k = 0; k < P; k++) {
		if (!(rd(q) && rd(dq) && rd(fw))) return 4;
		double* qm = out.data() + per_period * k;
		double* dqm = qm + (size_t)J * n;
		double* fm = dqm + (size_t)J * n;
		const uint32_t period = p0[0] + (uint32_t)k;
		for (size_t i = 0; i < n; i++) {
			for (int j = 0; j < J; j++) {
				se_joint(joints.data() + (long long)j * SENSE_JOINT_WORDS * js + (perj ? (long long)i : 0), js, slo, shi, period, (int)i, j, q[j * n + i], dq[j * n + i],
						 &qm[j * n + i], &dqm[j * n + i]);
				double zz[2];
				samp_normals(slo, shi, period, SENSE_TABLE_JOINT_NOISE, (int)i, j, 0, zz);
				z[(((size_t)k * J + j) * 2) * n + i] = zz[0];
				z[(((size_t)k * J + j) * 2 + 1) * n + i] = zz[1];
			}
			for (int s = 0; s < S; s++)
				for (int pair = 0; pair < 3; pair++) {
					const size_t r0 = ((size_t)6 * s + 2 * pair) * n + i, r1 = r0 + n;
					fm[r0] = fw[r0];
					fm[r1] = fw[r1];
					se_wrench_pair(wrenches.data() + (long long)s * SENSE_WRENCH_WORDS * ws + (perw ? (long long)i : 0), ws, slo, shi, period, (int)i, s, pair, &fm[r0], &fm[r1]);
				}
		}
	}
	uint64_t dseed;
	uint32_t rnd[2];
	std::vector<double> jlo(J * SENSE_JOINT_WORDS), jhi(jlo.size()), wlo(S * SENSE_WRENCH_WORDS), whi(wlo.size());
	if (fread(&dseed, 8, 1, f) != 1 || fread(rnd, 4, 2, f) != 2 || !(rd(jlo) && rd(jhi) && rd(wlo) && rd(whi))) return 4;
	fclose(f);
	std::vector<double> dj(jlo.size() * n), dw(wlo.size() * n);
	for (size_t i = 0; i < n; i++) {
		for (size_t w = 0; w < jlo.size(); w++) dj[w * n + i] = se_draw((uint32_t)dseed, (uint32_t)(dseed >> 32), rnd[0], SENSE_TABLE_JOINTS, (int)i, (int)w, jlo[w], jhi[w]);
		for (size_t w = 0; w < wlo.size(); w++) dw[w * n + i] = se_draw((uint32_t)dseed, (uint32_t)(dseed >> 32), rnd[0], SENSE_TABLE_WRENCHES, (int)i, (int)w, wlo[w], whi[w]);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(out) && wr(z) && wr(dj) && wr(dw);
	fclose(f);
	return okw ? 0 : 6;
}
