// The per-instance arithmetic of the contact planes and the simulated sensor (csrc/saip_contact.h) compiled for the host as a stand-alone
// program: N cases read from / written to raw binary files.  Built and run by tests/test_contact_cpu.py (once more with
// -fsanitize=address,undefined).
//
// in:  int32[4] { N, P, J, per_instance }, double dt, then doubles: planes ([P][8][N] per instance, else [P][8]), xc[N][3], Rc[N][9], rc[N][3],
//      tv[N][3], tw[N][3], tc[N][3], Rcs[N][9], tcs[N][3], rev[N][J] (0 / 1), aw[N][J][3], oj[N][J][3], summary[4][N]
// out: doubles p[N][3], v[N][3], f[N][3], fn_sum[N], dmin[N], active[N], tau[N][J], FS[N][3], MS[N][3], summary[4][N] (advanced once)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_contact.h"

using namespace saip;

int main(int argc, char** argv) {
	if (argc != 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 1;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[4];
	double dt;
	if (fread(h, 4, 4, f) != 4 || fread(&dt, 8, 1, f) != 1) return 3;
	const int N = h[0], P = h[1], J = h[2], per = h[3];
	if (N < 1 || P < 1 || P > CONTACT_MAX_PLANES || J < 0) return 3;
	const size_t n = N;
	std::vector<double> planes((size_t)P * CONTACT_PLANE_WORDS * (per ? n : 1)), xc(3 * n), Rc(9 * n), rc(3 * n), tv(3 * n), tw(3 * n), tc(3 * n),
		Rcs(9 * n), tcs(3 * n), rev(n * J), aw(3 * n * J), oj(3 * n * J), summary(CONTACT_SUMMARY_ROWS * n);
	auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); };
	const bool ok = rd(planes) && rd(xc) && rd(Rc) && rd(rc) && rd(tv) && rd(tw) && rd(tc) && rd(Rcs) && rd(tcs) && rd(rev) && rd(aw) && rd(oj) && rd(summary);
	fclose(f);
	if (!ok) return 4;
	std::vector<double> p(3 * n), v(3 * n), fo(3 * n), fn_sum(n), dmin(n), active(n), tau(n * J), FS(3 * n), MS(3 * n);
	for (size_t i = 0; i < n; i++) {
		ct_point(&xc[3 * i], &Rc[9 * i], &rc[3 * i], &p[3 * i]);
		ct_velocity(&tv[3 * i], &tw[3 * i], &tc[3 * i], &p[3 * i], &v[3 * i]);
		ContactForce c;
		ct_plane_forces(planes.data(), P, per ? (long long)n : 1, per ? (long long)i : 0, &p[3 * i], &v[3 * i], &c);
		for (int e = 0; e < 3; e++) fo[3 * i + e] = c.f[e];
		fn_sum[i] = c.fn_sum;
		dmin[i] = c.dmin;
		active[i] = c.active;
		for (int j = 0; j < J; j++) tau[i * J + j] = ct_joint_torque(rev[i * J + j] != 0.0, &aw[3 * (i * J + j)], &oj[3 * (i * J + j)], &p[3 * i], c.f);
		ct_sensor(c.f, &p[3 * i], &xc[3 * i], &Rc[9 * i], &Rcs[9 * i], &tcs[3 * i], &FS[3 * i], &MS[3 * i]);
		ct_summary_advance(&summary[i], (long long)n, dt, c);
	}
	f = fopen(argv[2], "wb");
	if (!f) return 5;
	auto wr = [&](const std::vector<double>& a) { return a.empty() || fwrite(a.data(), 8, a.size(), f) == a.size(); };
	const bool okw = wr(p) && wr(v) && wr(fo) && wr(fn_sum) && wr(dmin) && wr(active) && wr(tau) && wr(FS) && wr(MS) && wr(summary);
	fclose(f);
	return okw ? 0 : 6;
}
