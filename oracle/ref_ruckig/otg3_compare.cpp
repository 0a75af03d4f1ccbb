// TEST INFRASTRUCTURE ONLY.  Function-level check of the product's jerk-limited OTG core (sai-primitives_amd/csrc/saip_otg3.h, compiled
// here for the host, unchanged) against the REAL vendored Ruckig 0.10.1 of the reference, compiled from /root/reference/ruckig where it
// lies (oracle/Makefile, target _ref/otg3_compare): brake pre-trajectory, step 1 (extremal profiles + blocked intervals), step 2
// (profile of a given duration), on random inputs of the kinds the wrappers produce.  Prints the worst deviations; exit code 0 = all
// decisions equal and all numbers within 1e-9.
#include <ruckig/ruckig.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "saip_otg3.h"

using namespace ruckig;
namespace o3 = saip::otg3;

static double worst = 0.0;
static long mismatches = 0, cases1 = 0, cases2 = 0, found1 = 0, found2 = 0, nbr = 0;
static void cmp(double a, double b, const char* what) {
	if (std::isnan(a) && std::isnan(b)) return;
	const double d = std::abs(a - b) / std::max(1.0, std::abs(b));
	if (!(d <= 1e-9)) {
		if (mismatches < 20) printf("MISMATCH %s: %.17g vs %.17g\n", what, a, b);
		mismatches++;
	}
	if (d > worst) worst = d;
}

// `otg3_compare --record N`: N seeded cases and the reference's answers on them, as raw doubles on stdout, case (12) then record (173) per
// case in the layout of tests/cpp/otg3_vectors.cpp -- what tests/golden/make_otg3_golden.py stores as tests/golden/otg3_core_vectors.npz, so
// that the product's core is checked against the reference where the reference is not present.  The step-2 durations are chosen like below.
static int record(long N) {
	const double nan = std::nan("");
	std::mt19937_64 rng(24680);
	std::uniform_real_distribution<double> U(-1.0, 1.0);
	for (long it = 0; it < N; it++) {
		const double vMax = 0.2 + 3.0 * std::abs(U(rng)), aMax = 0.5 + 8.0 * std::abs(U(rng)), jMax = 1.0 + 40.0 * std::abs(U(rng));
		const double vMin = -vMax, aMin = -aMax;
		const int kind = (int)(it % 8);
		double p0 = 2 * U(rng), pf = 2 * U(rng), v0 = 0, a0 = 0, vf = 0, af = 0;
		if (kind >= 1) v0 = 0.95 * vMax * U(rng);
		if (kind >= 2) a0 = 0.9 * aMax * U(rng);
		if (kind == 3 || kind == 6) vf = 0.8 * vMax * U(rng);
		if (kind == 4) pf = p0 + 1e-3 * U(rng);
		if (kind == 5) { v0 = 1.4 * vMax * U(rng); a0 = 1.3 * aMax * U(rng); }
		if (kind == 6) af = 0.5 * aMax * U(rng);
		if (kind == 7) pf = p0;
		double c[12] = {p0, v0, a0, pf, vf, af, vMax, aMax, jMax, nan, nan, nan};
		double r[173];
		for (double& x : r) x = nan;
		Profile in;
		in.brake.get_position_brake_trajectory(v0, a0, vMax, vMin, aMax, aMin, jMax);
		in.set_boundary(p0, v0, a0, pf, vf, af);
		in.brake.finalize(in.p[0], in.v[0], in.a[0]);
		r[0] = in.brake.duration, r[1] = in.p[0], r[2] = in.v[0], r[3] = in.a[0];
		Block block;
		PositionThirdOrderStep1 s1{in.p[0], in.v[0], in.a[0], in.pf, in.vf, in.af, vMax, vMin, aMax, aMin, jMax};
		const bool f1 = s1.get_profile(in, block);
		double* q = r + 4;
		q[0] = f1;
		if (f1) {
			q[1] = block.t_min, q[2] = (bool)block.a, q[3] = (bool)block.b;
			if (block.a) { q[4] = block.a->left, q[5] = block.a->right; for (int i = 0; i < 7; i++) q[8 + i] = block.a->profile.t[i]; }
			if (block.b) { q[6] = block.b->left, q[7] = block.b->right; for (int i = 0; i < 7; i++) q[15 + i] = block.b->profile.t[i]; }
			for (int i = 0; i < 7; i++) q[22 + i] = block.p_min.t[i], q[29 + i] = block.p_min.j[i];
			for (int i = 0; i < 8; i++) q[36 + i] = block.p_min.a[i];
			q[44] = (int)block.p_min.direction, q[45] = (int)block.p_min.control_signs;
			for (int k = 0; k < 3; k++) {
				const double tf = (block.t_min - in.brake.duration) * (1.0 + (k == 0 ? 0.05 : (k == 1 ? 0.6 : 3.0)) * std::abs(U(rng))) + (k == 2 ? 0.5 : 0.0);
				if (tf <= 0 || block.is_blocked(tf + in.brake.duration)) continue;
				c[9 + k] = tf;
				double* s = r + 50 + 41 * k;
				Profile pr = in;
				PositionThirdOrderStep2 s2{tf, in.p[0], in.v[0], in.a[0], in.pf, in.vf, in.af, vMax, vMin, aMax, aMin, jMax};
				const bool f2 = s2.get_profile(pr);
				s[0] = f2;
				if (!f2) continue;
				for (int i = 0; i < 7; i++) s[1 + i] = pr.t[i], s[8 + i] = pr.j[i];
				for (int i = 0; i < 8; i++) s[15 + i] = pr.a[i], s[23 + i] = pr.v[i], s[31 + i] = pr.p[i];
				s[39] = (int)pr.control_signs, s[40] = (int)pr.limits;
			}
		}
		fwrite(c, sizeof(double), 12, stdout);
		fwrite(r, sizeof(double), 173, stdout);
	}
	return 0;
}

int main(int argc, char** argv) {
	if (argc > 2 && std::string(argv[1]) == "--record") return record(atol(argv[2]));
	const long N = argc > 1 ? atol(argv[1]) : 200000;
	std::mt19937_64 rng(12345);
	std::uniform_real_distribution<double> U(-1.0, 1.0);
	for (long it = 0; it < N; it++) {
		const double vMax = 0.2 + 3.0 * std::abs(U(rng)), aMax = 0.5 + 8.0 * std::abs(U(rng)), jMax = 1.0 + 40.0 * std::abs(U(rng));
		const double vMin = -vMax, aMin = -aMax;
		const int kind = (int)(it % 8);
		double p0 = 2 * U(rng), pf = 2 * U(rng), v0 = 0, a0 = 0, vf = 0, af = 0;
		if (kind >= 1) v0 = 0.95 * vMax * U(rng);
		if (kind >= 2) a0 = 0.9 * aMax * U(rng);
		if (kind == 3 || kind == 6) vf = 0.8 * vMax * U(rng);
		if (kind == 4) pf = p0 + 1e-3 * U(rng);
		if (kind == 5) { v0 = 1.4 * vMax * U(rng); a0 = 1.3 * aMax * U(rng); }   // beyond the limits: brake pre-trajectory
		if (kind == 6) af = 0.5 * aMax * U(rng);
		if (kind == 7) pf = p0;
		// ---- brake
		Profile in;
		in.brake.get_position_brake_trajectory(v0, a0, vMax, vMin, aMax, aMin, jMax);
		in.set_boundary(p0, v0, a0, pf, vf, af);
		in.brake.finalize(in.p[0], in.v[0], in.a[0]);
		o3::Brake3 br;
		double ps = p0, vs = v0, as = a0;
		o3::o3_brake(br, ps, vs, as, vMax, vMin, aMax, aMin, jMax);
		cmp(br.duration, in.brake.duration, "brake duration");
		cmp(ps, in.p[0], "brake p");
		cmp(vs, in.v[0], "brake v");
		cmp(as, in.a[0], "brake a");
		if (in.brake.duration > 0) nbr++;
		// ---- step 1
		Block block;
		PositionThirdOrderStep1 s1{in.p[0], in.v[0], in.a[0], in.pf, in.vf, in.af, vMax, vMin, aMax, aMin, jMax};
		const bool f1 = s1.get_profile(in, block);
		o3::O3Step1 m1;
		o3::Block3 mb;
		m1.init(ps, vs, as, pf, vf, af, vMax, vMin, aMax, aMin, jMax);
		const bool g1 = m1.run(mb, br.duration);
		cases1++;
		if (f1 != g1) {
			if (mismatches < 20) printf("MISMATCH step1 found %d vs %d (kind %d)\n", (int)g1, (int)f1, kind);
			mismatches++;
			continue;
		}
		if (!f1) continue;
		found1++;
		cmp(mb.t_min, block.t_min, "t_min");
		if (mb.has_a != (bool)block.a || mb.has_b != (bool)block.b) {
			if (mismatches < 20) printf("MISMATCH intervals a %d/%d b %d/%d\n", (int)mb.has_a, (int)(bool)block.a, (int)mb.has_b, (int)(bool)block.b);
			mismatches++;
			continue;
		}
		if (block.a) { cmp(mb.a_left, block.a->left, "a.left"); cmp(mb.a_right, block.a->right, "a.right"); for (int i = 0; i < 7; i++) cmp(mb.pa.t[i], block.a->profile.t[i], "a.profile.t"); }
		if (block.b) { cmp(mb.b_left, block.b->left, "b.left"); cmp(mb.b_right, block.b->right, "b.right"); for (int i = 0; i < 7; i++) cmp(mb.pb.t[i], block.b->profile.t[i], "b.profile.t"); }
		for (int i = 0; i < 7; i++) { cmp(mb.pmin.t[i], block.p_min.t[i], "p_min.t"); cmp(mb.pmin.j[i], block.p_min.j[i], "p_min.j"); }
		for (int i = 0; i < 8; i++) cmp(mb.pmin.a[i], block.p_min.a[i], "p_min.a");
		if ((int)block.p_min.direction != mb.pmin.dir || (int)block.p_min.control_signs != mb.pmin.cs) { mismatches++; if (mismatches < 20) printf("MISMATCH dir / control signs\n"); }
		// ---- step 2 at durations beyond the minimum (outside the blocked intervals), and at sampling
		for (int k = 0; k < 3; k++) {
			const double tf = (block.t_min - in.brake.duration) * (1.0 + (k == 0 ? 0.05 : (k == 1 ? 0.6 : 3.0)) * std::abs(U(rng))) + (k == 2 ? 0.5 : 0.0);
			if (tf <= 0) continue;
			const double tabs = tf + in.brake.duration;
			if (block.is_blocked(tabs)) continue;
			Profile pr = in;
			PositionThirdOrderStep2 s2{tf, in.p[0], in.v[0], in.a[0], in.pf, in.vf, in.af, vMax, vMin, aMax, aMin, jMax};
			const bool f2 = s2.get_profile(pr);
			o3::O3Step2 m2;
			o3::P3 w = m1.w;
			m2.init(tf, ps, vs, as, pf, vf, af, vMax, vMin, aMax, aMin, jMax);
			const bool g2 = m2.run(w);
			cases2++;
			if (f2 != g2) {
				if (mismatches < 20) printf("MISMATCH step2 found %d vs %d (kind %d, tf %.6g, t_min %.6g)\n", (int)g2, (int)f2, kind, tf, block.t_min);
				mismatches++;
				continue;
			}
			if (!f2) continue;
			found2++;
			for (int i = 0; i < 7; i++) { cmp(w.t[i], pr.t[i], "step2 t"); cmp(w.j[i], pr.j[i], "step2 j"); }
			for (int i = 0; i < 8; i++) { cmp(w.a[i], pr.a[i], "step2 a"); cmp(w.v[i], pr.v[i], "step2 v"); cmp(w.p[i], pr.p[i], "step2 p"); }
			if ((int)pr.control_signs != w.cs || (int)pr.limits != w.lim) { mismatches++; if (mismatches < 20) printf("MISMATCH step2 signs / limits\n"); }
		}
	}
	printf("step 1: %ld cases, %ld with a profile; step 2: %ld cases, %ld with a profile; %ld with a brake pre-trajectory\n", cases1, found1, cases2, found2, nbr);
	printf("worst relative deviation %.3e, mismatches %ld\n", worst, mismatches);
	return mismatches == 0 ? 0 : 1;
}
