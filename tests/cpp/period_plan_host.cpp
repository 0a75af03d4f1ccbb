// Host build of csrc/saip_period_plan.h (g++, no HIP): plan_sim over every combination of facts, one line per combination for
// tests/test_period_plan_cpu.py, which holds the invariants.  Columns: planes patches plant link_contact inertia sensing goals_written any_otg
// tree n, then per_substep link_contact_in contact_in integrator_in offer_cycle_sim may_fuse_next_otg; a TauBuf prints as its position in
// the chain (0 commanded, 1 plant, 2 link contact, 3 planes, 4 patches).
#include <cstdio>

#include "../../sai-primitives_amd/csrc/saip_period_plan.h"

static int pos(saip::TauBuf t) {
	switch (t) {
		case saip::TauBuf::Commanded: return 0;
		case saip::TauBuf::Plant: return 1;
		case saip::TauBuf::LinkContact: return 2;
		case saip::TauBuf::Planes: return 3;
		case saip::TauBuf::Patches: return 4;
	}
	return -1;
}

int main() {
	int lines = 0;
	for (int bits = 0; bits < (1 << 9); bits++) {
		saip::SimFacts f;
		f.planes = bits & 1;
		f.patches = bits & 2;
		if (f.planes && f.patches) continue;  // never both attached
		f.plant = bits & 4;
		f.link_contact = bits & 8;
		f.inertia = bits & 16;
		f.sensing = bits & 32;
		f.goals_written = bits & 64;
		f.any_otg = bits & 128;
		f.tree = bits & 256;
		for (int n = 6; n <= 8; n++) {
			f.n = n;
			const saip::SimPlan p = saip::plan_sim(f);
			std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", f.planes, f.patches, f.plant, f.link_contact, f.inertia, f.sensing, f.goals_written,
						f.any_otg, f.tree, f.n, p.per_substep, pos(p.link_contact_in), pos(p.contact_in), pos(p.integrator_in), p.offer_cycle_sim, p.may_fuse_next_otg);
			lines++;
		}
	}
	return lines == 3 * 128 * 3 ? 0 : 1;
}
