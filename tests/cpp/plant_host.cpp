// The per-instance arithmetic of the plant model (csrc/saip_plant.h) compiled for the host as a stand-alone program: S substeps of N
// instances, then one random draw, read from / written to raw binary files.  Built and run by tests/test_plant_cpu.py (once more with
// -fsanitize=address,undefined).  The kinematics a wrench needs (joint axes and origins, the application point, the link's rotation) are
// inputs: on the device they come from the walk of saip_fk.h.  Substep s belongs to period p0 + s.
//
// in:  int32[6] { N, J, W, per_instance_joints, per_instance_wrenches, S }, int64 p0, double dt, int32 rev[J] (0 / 1), int32 frame[W],
//      uint32 anc[W] (bit j: joint j is an ancestor of the wrench's link), then doubles: joints ([J][10][N] per instance, else [J][10]),
//      wrenches ([W][8][N] or [W][8]), summary[4][N], and per substep t[J][N], q[J][N], dq[J][N], aw[J][3][N], oj[J][3][N], p[W][3][N], Rl[W][9][N];
//      then uint64 seed, uint32 round, uint32 0, doubles joint_lo[J][10], joint_hi[J][10], wrench_lo[W][8], wrench_hi[W][8]
// out: doubles tau_act[S][J][N], summary[4][N], drawn joints [J][10][N], drawn wrenches [W][8][N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_plant.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[6];
	int64_t p0;
	double dt;
	if (fread(h, 4, 6, f) != 6 || fread(&p0, 8, 1, f) != 1 || fread(&dt, 8, 1, f) != 1) return 3;
	const int N = h[0], J = h[1], W = h[2], perj = h[3], perw = h[4], S = h[5];
	if (N < 1 || J < 1 || J > 32 || W < 0 || W > PLANT_MAX_WRENCHES || S < 0) return 3;
	const size_t n = N;
	std::vector<int32_t> rev(J), frame(W);
	std::vector<uint32_t> anc(W);
	if (fread(rev.data(), 4, J, f) != (size_t)J || (W && (fread(frame.data(), 4, W, f) != (size_t)W || fread(anc.data(), 4, W, f) != (size_t)W))) return 4;
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	std::vector<double> joints((size_t)J * PLANT_JOINT_WORDS * (perj ? n : 1)), wrenches((size_t)W * PLANT_WRENCH_WORDS * (perw ? n : 1)), summary(PLANT_SUMMARY_ROWS * n);
	if (!(rd(joints) && rd(wrenches) && rd(summary))) return 4;
	std::vector<double> tau_act((size_t)S * J * n), t(J * n), q(J * n), dq(J * n), aw(3 * J * n), oj(3 * J * n), p(3 * W * n), Rl(9 * W * n);
	const long long js = perj ? (long long)n : 1, ws = perw ? (long long)n : 1;
	for (int s = 0; s < S; s++) {
		if (!(rd(t) && rd(q) && rd(dq) && rd(aw) && rd(oj) && rd(p) && rd(Rl))) return 4;
		double* out = tau_act.data() + (size_t)s * J * n;
		for (size_t i = 0; i < n; i++) {
			PlantFold fold;
			pl_fold_init(&fold);
			for (int j = 0; j < J; j++) {
				PlantJointOut o;
				pl_joint(joints.data() + (long long)j * PLANT_JOINT_WORDS * js + (perj ? (long long)i : 0), js, t[j * n + i], q[j * n + i], dq[j * n + i], &o);
				out[j * n + i] = o.tau;
				pl_fold_joint(&fold, o, dq[j * n + i]);
			}
			double work_ext = 0.0;
			for (int w = 0; w < W; w++) {
				const double* ww = wrenches.data() + (long long)w * PLANT_WRENCH_WORDS * ws + (perw ? (long long)i : 0);
				if (anc[w] == 0 || !pl_wrench_acts(ww, ws, (long long)p0 + s)) continue;
				double R[9], pw[3], F[3], M[3];
				for (int e = 0; e < 9; e++) R[e] = Rl[(9 * w + e) * n + i];
				for (int e = 0; e < 3; e++) pw[e] = p[(3 * w + e) * n + i];
				pl_wrench_world(ww, ws, frame[w], R, F, M);
				for (int j = 0; j < J; j++) {
					if (!((anc[w] >> j) & 1u)) continue;
					const double a[3] = {aw[(3 * j) * n + i], aw[(3 * j + 1) * n + i], aw[(3 * j + 2) * n + i]};
					const double o[3] = {oj[(3 * j) * n + i], oj[(3 * j + 1) * n + i], oj[(3 * j + 2) * n + i]};
					const double x = pl_wrench_torque(rev[j] != 0, a, o, pw, F, M);
					out[j * n + i] = out[j * n + i] + x;
					work_ext = pl_work_add(work_ext, x, dq[j * n + i]);
				}
			}
			pl_summary_advance(&summary[i], (long long)n, dt, fold, work_ext);
		}
	}
	uint64_t seed;
	uint32_t rnd[2];
	std::vector<double> jlo(J * PLANT_JOINT_WORDS), jhi(jlo.size()), wlo(W * PLANT_WRENCH_WORDS), whi(wlo.size());
	if (fread(&seed, 8, 1, f) != 1 || fread(rnd, 4, 2, f) != 2 || !(rd(jlo) && rd(jhi) && rd(wlo) && rd(whi))) return 4;
	fclose(f);
	std::vector<double> dj(jlo.size() * n), dw(wlo.size() * n);
	for (size_t i = 0; i < n; i++) {
		for (size_t w = 0; w < jlo.size(); w++)
			dj[w * n + i] = pl_draw((uint32_t)seed, (uint32_t)(seed >> 32), rnd[0], PLANT_TABLE_JOINTS, (int)i, (int)w, jlo[w], jhi[w], false);
		for (size_t w = 0; w < wlo.size(); w++)
			dw[w * n + i] = pl_draw((uint32_t)seed, (uint32_t)(seed >> 32), rnd[0], PLANT_TABLE_WRENCHES, (int)i, (int)w, wlo[w], whi[w], w % PLANT_WRENCH_WORDS >= 6);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(tau_act) && wr(summary) && wr(dj) && wr(dw);
	fclose(f);
	return okw ? 0 : 6;
}
