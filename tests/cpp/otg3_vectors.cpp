// The product's jerk-limited OTG core (sai-primitives_amd/csrc/saip_otg3.h, compiled for the host, unchanged) on stored cases:
// reads cases from stdin, writes one record per case to stdout, both as raw doubles.  tests/test_otg_reference.py compares the
// records with the reference's (tests/golden/otg3_core_vectors.npz, recorded by `oracle/_ref/otg3_compare --record`, same layout).
//   case   (12): p0 v0 a0 pf vf af vMax aMax jMax tf0 tf1 tf2      (vMin = -vMax, aMin = -aMax; tf = NaN: no step 2 at that duration)
//   record (173): brake {duration, p, v, a}
//                 step 1 {found, t_min, has_a, has_b, a_left, a_right, b_left, b_right, a.t[7], b.t[7], p_min.t[7], p_min.j[7], p_min.a[8],
//                         direction, control_signs}
//                 3 x step 2 {found, t[7], j[7], a[8], v[8], p[8], control_signs, limits}
// Entries that do not apply (no profile found, interval absent, no step 2) are NaN.
#include <cmath>
#include <cstdio>
#include <vector>

#include "saip_otg3.h"

namespace o3 = saip::otg3;

int main() {
	const double nan = std::nan("");
	double c[12];
	while (fread(c, sizeof(double), 12, stdin) == 12) {
		std::vector<double> r(173, nan);
		const double p0 = c[0], v0 = c[1], a0 = c[2], pf = c[3], vf = c[4], af = c[5], vMax = c[6], aMax = c[7], jMax = c[8];
		const double vMin = -vMax, aMin = -aMax;
		o3::Brake3 br;
		double ps = p0, vs = v0, as = a0;
		o3::o3_brake(br, ps, vs, as, vMax, vMin, aMax, aMin, jMax);
		r[0] = br.duration, r[1] = ps, r[2] = vs, r[3] = as;
		o3::O3Step1 m1;
		o3::Block3 mb;
		m1.init(ps, vs, as, pf, vf, af, vMax, vMin, aMax, aMin, jMax);
		const bool g1 = m1.run(mb, br.duration);
		double* s1 = &r[4];
		s1[0] = g1;
		if (g1) {
			s1[1] = mb.t_min, s1[2] = mb.has_a, s1[3] = mb.has_b;
			if (mb.has_a) { s1[4] = mb.a_left, s1[5] = mb.a_right; for (int i = 0; i < 7; i++) s1[8 + i] = mb.pa.t[i]; }
			if (mb.has_b) { s1[6] = mb.b_left, s1[7] = mb.b_right; for (int i = 0; i < 7; i++) s1[15 + i] = mb.pb.t[i]; }
			for (int i = 0; i < 7; i++) s1[22 + i] = mb.pmin.t[i], s1[29 + i] = mb.pmin.j[i];
			for (int i = 0; i < 8; i++) s1[36 + i] = mb.pmin.a[i];
			s1[44] = mb.pmin.dir, s1[45] = mb.pmin.cs;
			for (int k = 0; k < 3; k++) {
				const double tf = c[9 + k];
				if (std::isnan(tf)) continue;
				double* s2 = &r[50 + 41 * k];
				o3::O3Step2 m2;
				o3::P3 w = m1.w;
				m2.init(tf, ps, vs, as, pf, vf, af, vMax, vMin, aMax, aMin, jMax);
				const bool g2 = m2.run(w);
				s2[0] = g2;
				if (!g2) continue;
				for (int i = 0; i < 7; i++) s2[1 + i] = w.t[i], s2[8 + i] = w.j[i];
				for (int i = 0; i < 8; i++) s2[15 + i] = w.a[i], s2[23 + i] = w.v[i], s2[31 + i] = w.p[i];
				s2[39] = w.cs, s2[40] = w.lim;
			}
		}
		fwrite(r.data(), sizeof(double), r.size(), stdout);
	}
	return 0;
}
