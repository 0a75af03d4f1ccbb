// The clearance monitor through the C++ facade: link spheres of a Panda against a floor, a post and each other, inside rollouts.
//   clearance_example <robot.txt> cfgonly               no device: the argument and order errors
//   clearance_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from the postures q ([dof][B] doubles); the example checks itself: the
//       readout of an evaluation against a recomputation from the model queries (1e-12 m, the same item); one sampling round of K
//       periods with the clearance cost as a hard constraint: the instances that went through the floor have an infinite cost, are
//       not counted as valid and are not the best; the reset of the summaries
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

static double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// signed distance of a sphere (c, rs) to obstacle row w = { kind, a[3], b[3], r }
static double obstacle_distance(const double* w, const double* c, double rs) {
	if (w[0] == SAIP_CLEARANCE_HALF_SPACE) return dot3(w + 1, c) - w[4] - rs;
	double e[3], d[3], u[3];
	for (int i = 0; i < 3; i++) {
		e[i] = w[4 + i] - w[1 + i];
		d[i] = c[i] - w[1 + i];
	}
	const double L2 = dot3(e, e);
	const double t = L2 > 0 ? std::fmin(std::fmax(dot3(d, e) / L2, 0.0), 1.0) : 0.0;
	for (int i = 0; i < 3; i++) u[i] = d[i] - t * e[i];
	return std::sqrt(dot3(u, u)) - (rs + w[7]);
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const std::vector<RobotController::ClearanceSphere> spheres = {
		{"link4", {0.0, 0.0, 0.0}, 0.06}, {"link6", {0.0, 0.0, 0.0}, 0.05}, {"end-effector", {0.0, 0.0, 0.03}, 0.04}};
	const std::vector<double> obstacles = {1, 0.0, 0.0, 1.0, 0.05, 0, 0, 0,        // the floor z >= 0.05
										   0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02};  // a horizontal post
	const std::vector<std::array<int, 2>> pairs = {{0, 2}};
	const double margin = 0.05;
	const int S = 3, O = 2;
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		int ok = 1;
		using Sph = std::vector<RobotController::ClearanceSphere>;
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, {1, 0, 0, 1, 0.05, 0, 0}); });                       // shape
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, obstacles, pairs, margin, true); });                // [O][8][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(Sph{{"no-such-link", {0, 0, 0}, 0.1}}, obstacles); });
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(Sph{}, obstacles); });                                        // 0 spheres
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres); });                                                // nothing to measure against
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(Sph{{"link4", {0, 0, 0}, -0.1}}, obstacles); });              // radius below 0
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(Sph{{"link4", {0, NAN, 0}, 0.1}}, obstacles); });
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, {2, 0, 0, 1, 0.05, 0, 0, 0}); });                    // unknown kind
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, {1, 0, 0, 1.001, 0.05, 0, 0, 0}); });                // not a unit normal
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, {0, 0, 0, 1, 0, 0, 1, -0.01}); });                   // capsule radius below 0
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, obstacles, {{0, 3}}); });                            // sphere index
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, obstacles, {{1, 1}}); });                            // a sphere against itself
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(spheres, obstacles, pairs, -0.01); });                        // margin
		ok &= throws<std::invalid_argument>([&] { c.attachClearance(Sph(33, spheres[0]), obstacles); });                          // above the maximum
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { c.attachClearance(spheres, obstacles, pairs, margin, false, true); });
		ok &= throws<std::runtime_error>([&] { c.attachClearance(spheres, {}, pairs); });
		ok &= throws<std::runtime_error>([&] { c.detachClearance(); });
		ok &= throws<std::runtime_error>([&] { c.clearanceInfo(); });
		ok &= throws<std::runtime_error>([&] { c.setClearanceObstacles(obstacles); });
		ok &= throws<std::runtime_error>([&] { c.evaluateClearance(); });
		ok &= throws<std::runtime_error>([&] { c.clearanceReadout(); });
		ok &= throws<std::runtime_error>([&] { c.clearanceSummary(); });
		ok &= throws<std::runtime_error>([&] { c.resetClearanceSummary(); });
		ok &= throws<std::runtime_error>([&] { c.clearanceCost(1.0); });
		ok &= c.clearanceObstaclesDevice() == nullptr && c.clearanceCentresDevice() == nullptr;
		ok &= saip_batch_clearance_readout_device(c.handle()) == nullptr && saip_batch_clearance_summary_device(c.handle()) == nullptr;
		std::cout << (ok ? "CLEARANCE_CFG_OK" : "CLEARANCE_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
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
		int ok = 1;
		c.attachClearance(spheres, obstacles, pairs, margin);
		const RobotController::ClearanceInfo info = c.clearanceInfo();
		ok &= info.n_spheres == S && info.n_obstacles == O && info.n_pairs == 1 && info.margin == margin && !info.per_instance && !info.keep_centres;
		ok &= c.clearanceCentresDevice() == nullptr && c.clearanceObstaclesDevice() != nullptr;
		// 1. an evaluation against the model queries
		c.evaluateClearance();
		const std::vector<double> ro = c.clearanceReadout();
		std::vector<std::vector<double>> centre;  // [S] of [3][B]
		for (const auto& sp : spheres) centre.push_back(s.robot->position(sp.link, sp.centre.data()));
		double worst = 0.0;
		int compared = 0;
		for (int b = 0; b < B; b++) {
			double d[7], cs[3][3];
			for (int i = 0; i < S; i++)
				for (int e = 0; e < 3; e++) cs[i][e] = centre[i][(size_t)e * B + b];
			for (int i = 0; i < S; i++)
				for (int o = 0; o < O; o++) d[i * O + o] = obstacle_distance(&obstacles[8 * o], cs[i], spheres[i].radius);
			const double u[3] = {cs[0][0] - cs[2][0], cs[0][1] - cs[2][1], cs[0][2] - cs[2][2]};
			d[S * O] = std::sqrt(dot3(u, u)) - (spheres[0].radius + spheres[2].radius);
			int k = 0, under = 0;
			for (int i = 1; i < 7; i++)
				if (d[i] < d[k]) k = i;
			double second = 1e300;
			for (int i = 0; i < 7; i++) {
				if (i != k) second = std::fmin(second, d[i]);
				under += d[i] < margin - 1e-9;
			}
			worst = std::fmax(worst, std::fabs(ro[b] - d[k]));
			ok &= std::fabs(ro[(size_t)7 * B + b] - d[S * O]) <= 1e-12 && ro[(size_t)3 * B + b] >= under;
			if (second - d[k] > 1e-9) {  // the item can only be compared where the minimum is not a near-tie
				ok &= ro[(size_t)B + b] == (double)k;
				compared++;
			}
		}
		ok &= worst <= 1e-12 && compared > B / 2;
		// 2. one sampling round with the clearance as a hard constraint
		const std::vector<double> pos = s.motion_force_task->getCurrentPosition();  // [3][B]
		const double p0[3] = {pos[0], pos[(size_t)B], pos[(size_t)2 * B]};
		std::vector<double> stay(2 * 3), keys((size_t)2 * 3 * B);
		for (int k = 0; k < 2; k++)
			for (int e = 0; e < 3; e++) {
				stay[(size_t)k * 3 + e] = p0[e];
				for (int b = 0; b < B; b++) keys[((size_t)k * 3 + e) * B + b] = p0[e];
			}
		s.motion_force_task->setGoalSchedule("position", keys, 2, 4, SAIP_SCHEDULE_LINEAR);
		s.motion_force_task->attachSampler({0.01, 0.01, 0.01}, stay, 0);
		c.recordRollouts(K, 1, SAIP_RECORD_POSE, s.motion_force_task);
		c.seedSampler(11);
		c.resetClearanceSummary();
		c.perturbGoalSchedules();
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		c.rolloutAsync(K, 5e-4, 2, no_gravity);
		c.rolloutCost({}, {p0[0], p0[1], p0[2]}, 0.0, 1.0);
		const std::vector<double> cost0 = c.getRolloutCost();
		c.clearanceCost(2.0);
		const std::vector<double> cost1 = c.getRolloutCost(), sm = c.clearanceSummary();
		ok &= c.clearanceInfo().period == K;
		int hits = 0, arg = -1;
		for (int b = 0; b < B; b++) {
			const bool hit = sm[b] < 0.0;
			hits += hit;
			ok &= hit == (sm[(size_t)2 * B + b] > 0.0) && hit == (sm[(size_t)3 * B + b] >= 0.0);
			if (hit) {
				ok &= std::isinf(cost1[b]) && cost1[b] > 0;
			} else {
				const double add = 2.0 * sm[(size_t)B + b];
				ok &= cost1[b] == cost0[b] + add;
				if (arg < 0 || cost1[b] < cost1[arg]) arg = b;
			}
		}
		ok &= hits > 0 && hits < B;
		c.updateSampler(1e-3);
		const RobotController::SamplerResult res = c.samplerResult();
		ok &= res.n_valid == B - hits && res.best == arg && res.min_cost == cost1[arg];
		// 3. the reset, the detach
		c.resetClearanceSummary();
		const std::vector<double> z = c.clearanceSummary();
		for (int b = 0; b < B; b++) ok &= std::isinf(z[b]) && z[b] > 0 && z[(size_t)B + b] == 0.0 && z[(size_t)2 * B + b] == 0.0 && z[(size_t)3 * B + b] == -1.0;
		ok &= c.clearanceInfo().period == 0;
		c.detachClearance();
		ok &= throws<std::runtime_error>([&] { c.clearanceReadout(); }) && c.clearanceObstaclesDevice() == nullptr;
		printf("worst |dmin - recomputation| %.3e m, items compared in %d of %d instances, %d of %d instances went through the floor\n", worst, compared, B, hits, B);
		std::cout << (ok ? "CLEARANCE_RUN_OK" : "CLEARANCE_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
