// Host-only: what the resident simulator decides about one period before it enqueues anything (saip_engine_rollout.cpp carries it out).
// Plain C++17, nothing from HIP: tests/cpp/period_plan_host.cpp compiles it alone.  DESIGN.md 4.7.2 says the same in prose.
//
// A period of saip_batch_rollout_async is, in this order: goal schedules, environment schedules, the simulated sensors (SENSE), the sensing
// model, the guards, the OTG step, the cycle, then per integration substep { plant, link contact, contact planes or patches, integrate },
// then the clearance monitor and the recorder.  The order is straight-line code there; the three questions with more than one answer
// are answered here, once, from the attach flags.
#pragma once

namespace saip {

struct SimFacts {  // everything the decisions depend on, and nothing else
	bool planes = false, patches = false, plant = false, link_contact = false, inertia = false, sensing = false;  // attached (planes and patches never both)
	bool goals_written = false;  // a goal schedule or the guards write goals in front of the period's OTG step
	bool any_otg = false;        // some task has its internal OTG on
	bool tree = false;
	int n = 0;                   // dof
};

enum class TauBuf { Commanded, Plant, LinkContact, Planes, Patches };  // the commanded torques, or the buffer that stage writes

struct SimPlan {
	bool per_substep;        // a stage stands in front of every substep: substeps are separate launches, no fused form
	TauBuf link_contact_in, contact_in, integrator_in;  // whose torques link contact, the contact planes or patches, and the integrator read
	bool offer_cycle_sim;    // rollouts: hand the SimRequest to the cycle launch (plan_cycle keeps the last word)
	bool may_fuse_next_otg;  // rollouts: integrate + the next period's OTG pair in one launch, if another period follows and otg_pair_ready()
};

inline SimPlan plan_sim(const SimFacts& f) {
	SimPlan p;
	// The substep stages.  Plant, link contact and the contact planes or patches are evaluated at the state of the substep they stand in front
	// of (a penalty force held over a control period is unstable at useful stiffness), so with any of them attached every substep is a
	// launch sequence of its own and no single launch can integrate the period.
	p.per_substep = f.planes || f.patches || f.plant || f.link_contact;
	// The torque chain: commanded -> plant -> link contact -> contact planes or patches -> integrator.  Every stage reads the buffer of the
	// nearest attached stage in front of it and writes its own; the commanded torques are never written.
	p.link_contact_in = f.plant ? TauBuf::Plant : TauBuf::Commanded;
	p.contact_in = f.link_contact ? TauBuf::LinkContact : p.link_contact_in;
	p.integrator_in = f.patches ? TauBuf::Patches : f.planes ? TauBuf::Planes : p.contact_in;
	// Both fused forms integrate the whole period in one launch, from the commanded torques, with the model's own inertial parameters, and
	// read the state the controller reads.  So neither is possible with a substep stage, an inertia table (the simulated robot is not the
	// model) or a sensing model (the controller reads a measured copy, and the next period's OTG step belongs behind the next
	// measurement).  Both exist for the 7-dof eight-lane kernels only.
	const bool fusable = !p.per_substep && !f.inertia && !f.sensing && f.n == 7;
	// The cycle launch integrates the state itself: only when no OTG step stands in front of the cycle.  Goals written in front of the
	// period do not bar it (the launch that writes them precedes the cycle either way), nor does a tree: plan_cycle refuses what its
	// kernel does not cover.
	p.offer_cycle_sim = fusable && !f.any_otg;
	// Integrate + the next period's OTG pair: the pair would read the next period's goal before the schedule or the guards have written
	// it, and the fused launch is chain-only.
	p.may_fuse_next_otg = fusable && !f.goals_written && !f.tree;
	return p;
}

}  // namespace saip
