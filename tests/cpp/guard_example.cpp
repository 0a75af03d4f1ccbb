// Resident guards through the C++ facade: a timed stop and retract of a Panda's tool inside a rollout.
//   guard_example <robot.txt> cfgonly               no device: the argument and order errors
//   guard_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from the postures q ([dof][B] doubles), at rest; the example checks itself:
//       guards "since >= 4 in phase 0 -> HOLD" and "since >= 2 in HOLD -> OFFSET(+z 2 cm)"; after 8 of the K >= 9 rollout periods every
//       instance is in phase 2, the entry periods are 4 and 7 and the goal is the latch with z + 0.02; after the rest nothing has left phase
//       2 and the readout position of a host-driven evaluation is the pose getter's; the reset; the detach
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../include/saip/SaiPrimitivesBatched.hpp"

using namespace SaiPrimitivesBatched;

static std::vector<saip_link_desc> read_robot(const char* path) {
	std::ifstream f(path);
	int n;
	f >> n;
	std::vector<saip_link_desc> links(n);
	for (auto& l : links) {
		std::string name;
		memset(&l, 0, sizeof(l));
		f >> name >> l.joint_type;
		strncpy(l.name, name.c_str(), SAIP_NAME_LEN - 1);
		for (double& v : l.origin_xyz) f >> v;
		for (double& v : l.origin_rpy) f >> v;
		for (double& v : l.axis) f >> v;
		f >> l.mass;
		for (double& v : l.com) f >> v;
		for (double& v : l.inertia) f >> v;
		f >> l.q_lower >> l.q_upper >> l.velocity_limit >> l.effort_limit;
	}
	if (!f) throw std::runtime_error("bad robot file");
	return links;
}

template <typename E, typename F>
static bool throws(F f) {
	try {
		f();
	} catch (const E&) {
		return true;
	} catch (...) {
	}
	return false;
}

struct Stack {
	std::shared_ptr<SaiModel> robot;
	std::shared_ptr<MotionForceTask> motion_force_task;
	std::shared_ptr<JointTask> joint_task;
	std::unique_ptr<RobotController> robot_controller;
	Stack(const std::vector<saip_link_desc>& links, int B, int device) {
		const double pos_in_link[3] = {0.0, 0.0, 0.07};
		robot = std::make_shared<SaiModel>(links, B, device);
		motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		joint_task = std::make_shared<JointTask>(robot);
		motion_force_task->disableInternalOtg();
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		robot_controller = std::make_unique<RobotController>(robot, task_list);
	}
};

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	using G = MotionForceTask::Guard;
	using Ph = MotionForceTask::GuardPhase;
	const std::vector<G> guards = {{0, 1, SAIP_GUARD_PERIODS, 0, SAIP_GUARD_GE, 4.0, 1, 0}, {1, 2, SAIP_GUARD_PERIODS, 0, SAIP_GUARD_GE, 2.0, 1, 0}};
	const std::vector<Ph> phases = {{SAIP_GUARD_FREE, {0, 0, 0}}, {SAIP_GUARD_HOLD, {0, 0, 0}}, {SAIP_GUARD_OFFSET, {0.0, 0.0, 0.02}}};
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		auto& t = *s.motion_force_task;
		int ok = 1;
		auto with = [&](int g, auto set) {
			std::vector<G> v = guards;
			set(v[g]);
			return v;
		};
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(std::vector<G>{}, phases); });                                      // 0 guards
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(guards, std::vector<Ph>{}); });                                     // 0 phases
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(std::vector<G>(9, guards[0]), phases); });                          // above the maximum
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(0, [](G& g) { g.to = 3; }), phases); });                       // outside the phases
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(1, [](G& g) { g.signal = 7; }), phases); });                   // unknown signal
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(1, [](G& g) { g.signal = SAIP_GUARD_POSITION, g.axis = 3; }), phases); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(0, [](G& g) { g.cmp = 2; }), phases); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(0, [](G& g) { g.threshold = NAN; }), phases); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(0, [](G& g) { g.hold = 0; }), phases); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(with(0, [](G& g) { g.blank = -1; }), phases); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(guards, {{SAIP_GUARD_HOLD, {0, 0, 0}}, phases[1], phases[2]}); });  // phase 0 not FREE
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(guards, {phases[0], phases[1], {3, {0, 0, 0}}}); });                // unknown mode
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(guards, {phases[0], phases[1], {SAIP_GUARD_OFFSET, {0, INFINITY, 0}}}); });
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(std::vector<double>(15, 0.0), 2, std::vector<double>(12, 0.0), 3); });  // shape
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(std::vector<double>(16, 0.0), 2, std::vector<double>(12, 0.0), 3, true); });  // [G][8][B] expected
		ok &= throws<std::invalid_argument>([&] { t.attachGuards(std::vector<double>(16, 0.5), 2, std::vector<double>(12, 0.0), 3); });  // words that are no integers
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { t.attachGuards(guards, phases); });
		ok &= throws<std::runtime_error>([&] { t.detachGuards(); });
		ok &= throws<std::runtime_error>([&] { c.guardInfo(); });
		ok &= throws<std::runtime_error>([&] { c.evaluateGuards(); });
		ok &= throws<std::runtime_error>([&] { c.resetGuards(); });
		ok &= throws<std::runtime_error>([&] { c.guardState(); });
		ok &= throws<std::runtime_error>([&] { c.guardReadout(); });
		ok &= throws<std::runtime_error>([&] { c.guardCost(1, 1.0); });
		ok &= c.guardTableDevice() == nullptr && saip_batch_guard_readout_device(c.handle()) == nullptr;
		std::cout << (ok ? "GUARD_CFG_OK" : "GUARD_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		if (K < 9) return 2;
		Stack s(links, B, 0);
		auto& c = *s.robot_controller;
		auto& t = *s.motion_force_task;
		const int n = s.robot->dof();
		std::vector<double> q((size_t)n * B);
		std::ifstream f(argv[5], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		if (!f) return 3;
		s.robot->setQ(q);
		s.robot->setDq(std::vector<double>((size_t)n * B, 0.0));
		s.robot->updateModel();
		c.reinitializeTasks();
		c.updateControllerTaskModels();
		int ok = 1;
		t.attachGuards(guards, phases);
		const RobotController::GuardInfo info = c.guardInfo();
		ok &= info.task == 0 && info.n_guards == 2 && info.n_phases == 3 && !info.per_instance && info.needs_pose;
		ok &= c.guardTableDevice() != nullptr;
		ok &= throws<std::runtime_error>([&] { t.attachGuards(guards, phases); });  // a second attach
		RobotController::GuardState st = c.guardState();
		for (int b = 0; b < B; b++) ok &= st.phase[b] == 0 && st.clock[b] == 0 && st.entry[b] == 0 && st.entry[(size_t)B + b] == -1 && st.entry[(size_t)2 * B + b] == -1;
		// 1. 8 periods: the evaluation of period 4 fires the first guard, that of period 7 the second
		c.rolloutAsync(8, 1e-3);
		st = c.guardState();
		for (int b = 0; b < B; b++) {
			ok &= st.phase[b] == 2 && st.clock[b] == 8 && st.since[b] == 0;
			ok &= st.entry[(size_t)B + b] == 4 && st.entry[(size_t)2 * B + b] == 7;
			ok &= st.fires[b] == 1 && st.fires[(size_t)B + b] == 1;
		}
		// the goal of the OFFSET phase: the latch, z + 0.02 rounded once; the velocity and acceleration goals are 0
		const std::vector<double> gp = t.getGoalPosition(), go = t.getGoalOrientation(), gv = t.getGoalLinearVelocity();
		for (int b = 0; b < B; b++) {
			ok &= gp[b] == st.latch[b] && gp[(size_t)B + b] == st.latch[(size_t)B + b] && gp[(size_t)2 * B + b] == st.latch[(size_t)2 * B + b] + 0.02;
			for (int e = 0; e < 9; e++) ok &= go[(size_t)e * B + b] == st.latch[(size_t)(3 + e) * B + b];
			for (int e = 0; e < 3; e++) ok &= gv[(size_t)e * B + b] == 0.0;
		}
		// 2. the rest of the K periods: no guard leaves phase 2; the readout position is the pose of the state the last evaluation saw
		c.rolloutAsync(K - 8, 1e-3);
		st = c.guardState();
		for (int b = 0; b < B; b++) ok &= st.phase[b] == 2 && st.clock[b] == K && st.since[b] == K - 8 && st.entry[(size_t)2 * B + b] == 7;
		c.evaluateGuards();
		const std::vector<double> ro = c.guardReadout(), pos = t.getCurrentPosition();
		for (int b = 0; b < B; b++) {
			for (int e = 0; e < 3; e++) ok &= ro[(size_t)(5 + e) * B + b] == pos[(size_t)e * B + b];
			ok &= std::isnan(ro[b]) && std::isnan(ro[(size_t)4 * B + b]);  // no guard asked for the force or the joint speed
		}
		// 3. the reset, the detach
		c.resetGuards();
		st = c.guardState();
		for (int b = 0; b < B; b++) ok &= st.phase[b] == 0 && st.clock[b] == 0 && st.entry[(size_t)2 * B + b] == -1 && st.fires[b] == 0 && st.latch[b] == 0.0;
		t.detachGuards();
		ok &= throws<std::runtime_error>([&] { c.guardReadout(); }) && c.guardTableDevice() == nullptr;
		std::cout << (ok ? "GUARD_RUN_OK" : "GUARD_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
