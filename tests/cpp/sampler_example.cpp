// A full planning round of a sampling MPC through the C++ facade: the resident rollout sampler on a Panda stack.
//   sampler_example <robot.txt> cfgonly               no device: the error behaviour of the facade
//   sampler_example <robot.txt> run <B> <R> <q.bin>   on GPU 0 from q ([dof][B] doubles, instance 0 is the measured state): save; R rounds of
//       { restore instance 0 into all, rewind, reset the recorder, perturb, 40 periods, cost = squared distance of the last logged position
//       to a target, take the best }; instance 0 runs the best plan of the round before (same cost, 1e-5 relative); the minimum never rises
//       and ends below the cost of staying; the best instance's state into all
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
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		int ok = 1;
		// without a schedule there is no sampler, and without a sampler every entry is an order error
		ok &= throws<std::runtime_error>([&] { s.motion_force_task->attachSampler({0.1, 0.1, 0.1}); });
		ok &= throws<std::runtime_error>([&] { s.motion_force_task->detachSampler(); });
		ok &= throws<std::runtime_error>([&] { s.joint_task->samplerNominal(); });
		ok &= throws<std::runtime_error>([&] { c.seedSampler(1); });
		ok &= throws<std::runtime_error>([&] { c.perturbGoalSchedules(); });
		ok &= throws<std::runtime_error>([&] { c.updateSampler(1.0); });
		ok &= throws<std::runtime_error>([&] { c.shiftSampler(1); });
		ok &= throws<std::runtime_error>([&] { c.samplerResult(); });
		ok &= throws<std::runtime_error>([&] { c.getRolloutCost(); });
		ok &= throws<std::runtime_error>([&] { c.restoreStateBest(RobotController::StateSnapshot()); });
		// the facade's own shape checks
		ok &= throws<std::invalid_argument>([&] { c.rolloutCost({1.0, 2.0}); });
		ok &= throws<std::invalid_argument>([&] { c.rolloutCost({}, {0.0, 0.0}); });
		ok &= throws<std::invalid_argument>([&] { c.setRolloutCost(std::vector<double>(5, 0.0)); });
		ok &= saip_batch_sampler_cost_device(c.handle()) == nullptr && saip_batch_sampler_best_map_device(c.handle()) == nullptr;
		ok &= saip_batch_sampler_attach(c.handle(), 0, nullptr, nullptr, 1) == SAIP_ERR_INVALID_ARGUMENT;
		const double sigma[3] = {0.1, 0.1, 0.1};
		ok &= saip_batch_sampler_attach(c.handle(), 0, sigma, nullptr, 5) == SAIP_ERR_INVALID_ARGUMENT;
		ok &= saip_batch_sampler_attach(c.handle(), 0, sigma, nullptr, 1) == SAIP_ERR_ORDER;
		std::cout << (ok ? "SAMPLER_CFG_OK" : "SAMPLER_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), R = atoi(argv[4]), K = 4, STRIDE = 10, PERIODS = 40;
		Stack s(links, B, 0);
		auto& c = *s.robot_controller;
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
		const std::vector<double> pos = s.motion_force_task->getCurrentPosition();  // [3][B]
		const double p0[3] = {pos[0], pos[(size_t)B], pos[(size_t)2 * B]};
		const std::vector<double> target = {p0[0] + 0.03, p0[1] - 0.02, p0[2] + 0.04};
		// the nominal plan is "stay"; every instance starts from it
		std::vector<double> stay((size_t)K * 3), keys((size_t)K * 3 * B);
		for (int k = 0; k < K; k++)
			for (int e = 0; e < 3; e++) {
				stay[(size_t)k * 3 + e] = p0[e];
				for (int b = 0; b < B; b++) keys[((size_t)k * 3 + e) * B + b] = p0[e];
			}
		s.motion_force_task->setGoalSchedule("position", keys, K, STRIDE, SAIP_SCHEDULE_LINEAR);
		s.motion_force_task->attachSampler({0.02, 0.02, 0.02}, stay, 1);
		c.recordRollouts(4, STRIDE, SAIP_RECORD_POSE, s.motion_force_task);
		c.seedSampler(2026);
		RobotController::StateSnapshot snap = c.saveState();
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		int ok = 1;
		double first_cost0 = 0.0, last_min = 0.0, worst = 0.0;
		RobotController::SamplerResult res;
		for (int r = 0; r < R; r++) {
			c.restoreState(snap, 0);
			c.rewindGoalSchedules();
			c.resetRolloutRecorder();
			c.perturbGoalSchedules();
			c.rolloutAsync(PERIODS, 5e-4, 2, no_gravity);
			c.rolloutCost({}, target, 0.0, 1.0);
			const std::vector<double> cost = c.getRolloutCost();
			c.updateSampler(1e-300);
			res = c.samplerResult();
			int arg = 0;
			for (int b = 1; b < B; b++)
				if (cost[b] < cost[arg]) arg = b;
			ok &= res.best == arg && res.min_cost == cost[arg] && res.n_valid == B && res.sum_w >= 1.0;
			if (r == 0) {
				first_cost0 = cost[0];
			} else {
				const double rel = std::fabs(cost[0] - last_min) / last_min;
				worst = std::max(worst, rel);
				ok &= rel <= 1e-5 && res.min_cost <= last_min * (1 + 1e-5);
			}
			last_min = res.min_cost;
		}
		ok &= last_min < first_cost0;
		// the nominal plan is the best instance's keyframes; shifting it repeats the last keyframe
		const std::vector<double> nominal = s.motion_force_task->samplerNominal();
		c.shiftSampler(1);
		const std::vector<double> shifted = s.motion_force_task->samplerNominal();
		for (int k = 0; k < K; k++)
			for (int e = 0; e < 3; e++) ok &= shifted[(size_t)k * 3 + e] == nominal[(size_t)std::min(k + 1, K - 1) * 3 + e];
		c.restoreStateBest(snap);
		c.synchronize();
		c.pullState();
		const std::vector<double> qb = s.robot->q();
		for (int j = 0; j < n; j++)
			for (int b = 0; b < B; b++) ok &= qb[(size_t)j * B + b] == q[(size_t)j * B + res.best];
		s.motion_force_task->clearGoalSchedule();  // takes the sampler along
		ok &= throws<std::runtime_error>([&] { c.perturbGoalSchedules(); });
		std::cout << (ok ? "SAMPLER_RUN_OK" : "SAMPLER_RUN_FAIL") << " first " << first_cost0 << " last minimum " << last_min << " round-to-round worst " << worst << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
