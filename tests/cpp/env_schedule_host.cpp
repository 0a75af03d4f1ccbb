// The environment schedules (csrc/saip_env_schedule.h) and the moving-surface contact arithmetic (csrc/saip_contact.h,
// csrc/saip_contact_patch.h) compiled for the host as a stand-alone program over raw binary files.  Built and run by
// tests/test_env_schedule_cpu.py (once more with -fsanitize=address,undefined).
//
// env_schedule_host schedule in.bin out.bin
//   in:  int32[9] { planes, K, n_items, B (0: batch-uniform), first, items (of the whole table), stride, mode, periods }, double T, double
//        sentinel, then the keyframes [K][n_items][W] or [K][n_items][W][B]
//   out: per rollout period c = 0 .. periods - 1: the table [items][8] or [items][8][B], then for planes the velocity table [items][4] or
//        [items][4][B], each filled with the sentinel and then written the way the kernel writes it (env_period_index, env_timing,
//        env_entry_item per item and column)
// env_schedule_host forces in.bin out.bin
//   in:  int32[4] { N, P, per_instance, n_points (0: single point) }, then doubles: planes ([P][8][N] per instance, else [P][8]), vel ([P][4][N] or
//        [P][4]), xc[N][3], Rc[N][9], r[max(n_points, 1)][3], tv[N][3], tw[N][3], tc[N][3]
//   out: single point: for ct_plane_forces_moving and then for ct_plane_forces: f[N][3], fn_sum[N], dmin[N], active[N]
//        patch: for cp_slot_eval_moving and then for cp_slot_eval: p[N][8][3], f[N][8][3], m[N][8][3], fn_sum[N][8], dcand[N][8], active[N][8],
//        F[N][3], M[N][3]
// env_schedule_host check in.bin
//   in:  int32[5] { planes, K, n_items, cols, mode }, then the keyframes; prints "ok" or what env_check_keyframes refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai-primitives_amd/csrc/saip_contact_patch.h"
#include "../../sai-primitives_amd/csrc/saip_env_schedule.h"

using namespace saip;

static bool rd(FILE* f, std::vector<double>& v) { return v.empty() || fread(v.data(), 8, v.size(), f) == v.size(); }
static bool wr(FILE* f, const std::vector<double>& v) { return v.empty() || fwrite(v.data(), 8, v.size(), f) == v.size(); }

static int run_schedule(FILE* in, FILE* out) {
	int32_t h[9];
	double T, sentinel;
	if (fread(h, 4, 9, in) != 9 || fread(&T, 8, 1, in) != 1 || fread(&sentinel, 8, 1, in) != 1) return 3;
	const int planes = h[0], K = h[1], n_items = h[2], B = h[3], first = h[4], items = h[5], stride = h[6], mode = h[7], periods = h[8];
	if (K < 1 || n_items < 1 || first < 0 || first + n_items > items || stride < 1 || B < 0 || periods < 1) return 3;
	const size_t W = planes ? ENV_PLANE_WORDS : ENV_OBSTACLE_WORDS, cols = B ? B : 1;
	std::vector<double> key((size_t)K * n_items * W * cols);
	if (!rd(in, key)) return 4;
	for (int c = 0; c < periods; c++) {
		std::vector<double> table((size_t)items * ENV_TABLE_WORDS * cols, sentinel), vel(planes ? (size_t)items * ENV_VELOCITY_WORDS * cols : 0, sentinel);
		EnvEntry E;
		memset(&E, 0, sizeof(E));
		E.table = table.data();
		E.vel = planes ? vel.data() : nullptr;
		E.key = key.data();
		E.planes = planes;
		E.per_instance = B ? 1 : 0;
		E.first = first;
		E.n_items = n_items;
		env_timing(env_period_index(c, planes), K, stride, mode, &E.i, &E.s, &E.moving);
		E.span = (double)stride * T;
		for (int item = 0; item < n_items; item++)
			for (size_t col = 0; col < cols; col++) env_entry_item(E, item, B ? (long long)cols : 1, B ? (long long)col : 0);
		if (!wr(out, table) || !wr(out, vel)) return 6;
	}
	return 0;
}

static int run_forces(FILE* in, FILE* out) {
	int32_t h[4];
	if (fread(h, 4, 4, in) != 4) return 3;
	const int N = h[0], P = h[1], per = h[2], n_points = h[3];
	if (N < 1 || P < 1 || P > CONTACT_MAX_PLANES || n_points < 0 || n_points > PATCH_MAX_POINTS) return 3;
	const size_t n = N, np = n_points ? n_points : 1;
	std::vector<double> planes((size_t)P * CONTACT_PLANE_WORDS * (per ? n : 1)), vel((size_t)P * 4 * (per ? n : 1)), xc(3 * n), Rc(9 * n), r(3 * np), tv(3 * n),
		tw(3 * n), tc(3 * n);
	if (!(rd(in, planes) && rd(in, vel) && rd(in, xc) && rd(in, Rc) && rd(in, r) && rd(in, tv) && rd(in, tw) && rd(in, tc))) return 4;
	const long long stride = per ? (long long)n : 1;
	for (int moving = 1; moving >= 0; moving--) {
		if (n_points == 0) {
			std::vector<double> fo(3 * n), fn_sum(n), dmin(n), active(n);
			for (size_t i = 0; i < n; i++) {
				double p[3], v[3];
				ContactForce c;
				ct_point(&xc[3 * i], &Rc[9 * i], &r[0], p);
				ct_velocity(&tv[3 * i], &tw[3 * i], &tc[3 * i], p, v);
				if (moving) ct_plane_forces_moving(planes.data(), vel.data(), P, stride, per ? (long long)i : 0, p, v, &c);
				else ct_plane_forces(planes.data(), P, stride, per ? (long long)i : 0, p, v, &c);
				for (int e = 0; e < 3; e++) fo[3 * i + e] = c.f[e];
				fn_sum[i] = c.fn_sum;
				dmin[i] = c.dmin;
				active[i] = c.active;
			}
			if (!(wr(out, fo) && wr(out, fn_sum) && wr(out, dmin) && wr(out, active))) return 6;
			continue;
		}
		std::vector<double> p(24 * n), fo(24 * n), m(24 * n), fn_sum(8 * n), dcand(8 * n), active(8 * n), F(3 * n), M(3 * n);
		for (size_t i = 0; i < n; i++) {
			PatchSlot s[PATCH_MAX_POINTS];
			for (int l = 0; l < PATCH_MAX_POINTS; l++) {
				if (l >= n_points) cp_slot_unused(&s[l]);
				else if (moving)
					cp_slot_eval_moving(planes.data(), vel.data(), P, stride, per ? (long long)i : 0, &xc[3 * i], &Rc[9 * i], &r[3 * l], &tv[3 * i], &tw[3 * i], &tc[3 * i],
										&s[l]);
				else cp_slot_eval(planes.data(), P, stride, per ? (long long)i : 0, &xc[3 * i], &Rc[9 * i], &r[3 * l], &tv[3 * i], &tw[3 * i], &tc[3 * i], &s[l]);
				for (int e = 0; e < 3; e++) {
					p[(i * 8 + l) * 3 + e] = s[l].p[e];
					fo[(i * 8 + l) * 3 + e] = s[l].c.f[e];
					m[(i * 8 + l) * 3 + e] = s[l].m[e];
				}
				fn_sum[i * 8 + l] = s[l].c.fn_sum;
				dcand[i * 8 + l] = s[l].dcand;
				active[i * 8 + l] = s[l].c.active;
			}
			PatchNet nt;
			cp_net(s, &nt);
			for (int e = 0; e < 3; e++) {
				F[3 * i + e] = nt.F[e];
				M[3 * i + e] = nt.M[e];
			}
		}
		if (!(wr(out, p) && wr(out, fo) && wr(out, m) && wr(out, fn_sum) && wr(out, dcand) && wr(out, active) && wr(out, F) && wr(out, M))) return 6;
	}
	return 0;
}

static int run_check(FILE* in) {
	int32_t h[5];
	if (fread(h, 4, 5, in) != 5) return 3;
	const int planes = h[0], K = h[1], n_items = h[2], cols = h[3], mode = h[4];
	if (K < 1 || n_items < 1 || cols < 1) return 3;
	std::vector<double> key((size_t)K * n_items * (planes ? ENV_PLANE_WORDS : ENV_OBSTACLE_WORDS) * cols);
	if (!rd(in, key)) return 4;
	char msg[200];
	if (env_check_keyframes(key.data(), planes, K, n_items, (size_t)cols, mode, msg, sizeof(msg))) puts("ok");
	else puts(msg);
	return 0;
}

int main(int argc, char** argv) {
	const bool check = argc == 3 && !strcmp(argv[1], "check");
	if (!check && !(argc == 4 && (!strcmp(argv[1], "schedule") || !strcmp(argv[1], "forces")))) {
		fprintf(stderr, "usage: %s schedule|forces in.bin out.bin | check in.bin\n", argv[0]);
		return 1;
	}
	FILE* in = fopen(argv[2], "rb");
	if (!in) return 2;
	int rc;
	if (check) {
		rc = run_check(in);
	} else {
		FILE* out = fopen(argv[3], "wb");
		if (!out) {
			fclose(in);
			return 5;
		}
		rc = !strcmp(argv[1], "schedule") ? run_schedule(in, out) : run_forces(in, out);
		if (fclose(out) != 0 && rc == 0) rc = 6;
	}
	fclose(in);
	return rc;
}
