// Environment schedules through the C++ facade: a table that rises under the tool of a Panda and a floor that jumps up under its link
// spheres, inside rollouts.
//   env_schedule_example <robot.txt> cfgonly               no device: the argument and order errors
//   env_schedule_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from the postures q ([dof][B] doubles); the example checks itself: in
//       even instances the table rises 2 cm through the tool point over 4 periods and touches, in odd ones it stops 1 cm short and does
//       not; the belt velocity u drags the touching tools along +x; the floor of the clearance monitor jumps at keyframe 1, which the
//       monitor sees one period early (it looks at the end of the period); a rewind replays the same summaries; the rules of the tables
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
	const std::vector<RobotController::ClearanceSphere> spheres = {{"link4", {0.0, 0.0, 0.0}, 0.06}, {"end-effector", {0.0, 0.0, 0.03}, 0.04}};
	const std::vector<double> floor_low = {1, 0.0, 0.0, 1.0, -1.0, 0, 0, 0}, floor_high = {1, 0.0, 0.0, 1.0, 10.0, 0, 0, 0};
	std::vector<double> floor_keys = floor_low;
	floor_keys.insert(floor_keys.end(), floor_high.begin(), floor_high.end());
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		auto& t = *s.motion_force_task;
		int ok = 1;
		// nothing can be attached without a device, so every schedule entry refuses by order; the facade's own shape checks come first
		ok &= throws<std::runtime_error>([&] { c.setObstacleSchedule(floor_keys, 2); });
		ok &= throws<std::runtime_error>([&] { c.clearObstacleSchedule(); });
		ok &= throws<std::runtime_error>([&] { c.obstacleScheduleInfo(); });
		ok &= throws<std::runtime_error>([&] { t.setContactSchedule(std::vector<double>(24, 0.0), 2); });
		ok &= throws<std::runtime_error>([&] { t.clearContactSchedule(); });
		ok &= throws<std::runtime_error>([&] { t.contactScheduleInfo(); });
		ok &= throws<std::runtime_error>([&] { t.contactVelocityDevice(); });
		ok &= throws<std::invalid_argument>([&] { c.rewindEnvironment(-1); });
		ok &= throws<std::invalid_argument>([&] { check(saip_batch_env_schedule_attach(c.handle(), 7, 0, 0, 1, floor_keys.data(), 2, 1, SAIP_ENV_HOLD)); });
		ok &= throws<std::invalid_argument>([&] { check(saip_batch_env_schedule_attach(c.handle(), SAIP_ENV_TARGET_OBSTACLES, 0, 0, 1, floor_keys.data(), 2, 1, 2)); });
		ok &= throws<std::invalid_argument>([&] { check(saip_batch_env_schedule_attach(c.handle(), SAIP_ENV_TARGET_OBSTACLES, 0, 0, 1, floor_keys.data(), 0, 1, 0)); });
		ok &= throws<std::invalid_argument>([&] { check(saip_batch_env_schedule_attach(c.handle(), SAIP_ENV_TARGET_OBSTACLES, 0, 0, 1, floor_keys.data(), 2, 0, 0)); });
		ok &= throws<std::invalid_argument>([&] { check(saip_batch_env_schedule_attach(c.handle(), SAIP_ENV_TARGET_OBSTACLES, 0, 0, 1, nullptr, 2, 1, 0)); });
		c.rewindEnvironment(5);
		c.clearEnvironmentSchedules();  // all of none
		ok &= saip_batch_env_schedule_keyframes_device(c.handle(), SAIP_ENV_TARGET_PLANES, -1) == nullptr;
		ok &= saip_batch_env_schedule_velocity_device(c.handle(), SAIP_ENV_TARGET_PATCH, -1) == nullptr;
		std::cout << (ok ? "ENV_SCHEDULE_CFG_OK" : "ENV_SCHEDULE_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		if (B < 2 || K < 6) return 2;
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
		// 1. a table under the tool: 1 cm (even instances) or 3 cm (odd) below the tool point, rising 2 cm over 4 periods on a belt that runs along +x
		const std::vector<double> pos = t.getCurrentPosition();  // [3][B]
		std::vector<double> planes((size_t)8 * B), keys((size_t)2 * 12 * B, 0.0);
		const double row[8] = {0, 0, 1, 0, 5e3, 10.0, 0.2, 1e-3};
		for (int b = 0; b < B; b++) {
			for (int w = 0; w < 8; w++) planes[(size_t)w * B + b] = row[w];
			planes[(size_t)3 * B + b] = pos[(size_t)2 * B + b] - (b % 2 == 0 ? 0.01 : 0.03);
			for (int k = 0; k < 2; k++) {
				for (int w = 0; w < 8; w++) keys[((size_t)k * 12 + w) * B + b] = planes[(size_t)w * B + b];
				keys[((size_t)k * 12 + 3) * B + b] += 0.02 * k;
				keys[((size_t)k * 12 + 8) * B + b] = 0.05;
			}
		}
		t.attachContactPlanes(planes, 1, {0.0, 0.0, 0.0}, true, true);
		ok &= throws<std::invalid_argument>([&] { t.setContactSchedule(std::vector<double>(24, 0.0), 2); });  // [K][n][12][B] expected
		t.setContactSchedule(keys, 2, 4, SAIP_ENV_LINEAR);
		ok &= throws<std::runtime_error>([&] { t.setContactSchedule(keys, 2, 4, SAIP_ENV_LINEAR); });        // one schedule per table
		ok &= throws<std::runtime_error>([&] { t.setContactPlanes(planes); });                               // the schedule writes the table
		TemplateTask::EnvScheduleInfo ci = t.contactScheduleInfo();
		ok &= ci.first == 0 && ci.n_items == 1 && ci.n_keyframes == 2 && ci.stride == 4 && ci.mode == SAIP_ENV_LINEAR && ci.per_instance == 1 && ci.period == 0;
		ok &= t.contactVelocityDevice() != nullptr;
		// 2. a floor far below the robot that jumps above it at keyframe 1 (stride 3): the monitor of period c sees period index c + 1
		c.attachClearance(spheres, floor_low, {}, 0.05);
		c.setObstacleSchedule(floor_keys, 2, 3, SAIP_ENV_HOLD);
		ok &= throws<std::runtime_error>([&] { c.setClearanceObstacles(floor_low); });
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		c.rolloutAsync(K, 5e-4, 2, no_gravity);
		const std::vector<double> sm = t.contactSummary(), ro = t.contactReadout(), cs = c.clearanceSummary();
		int touching = 0;
		for (int b = 0; b < B; b++) {
			const bool even = b % 2 == 0;
			ok &= even ? sm[(size_t)3 * B + b] > 0.0 : sm[(size_t)3 * B + b] == 0.0;
			if (even) ok &= ro[b] > 0.0 && ro[(size_t)2 * B + b] > 0.0;  // dragged along +x, pushed up
			touching += sm[(size_t)3 * B + b] > 0.0;
			ok &= cs[(size_t)2 * B + b] == (double)(K - 2) && cs[(size_t)3 * B + b] == 2.0;  // periods 2 .. K - 1 collide: index 3 = (2 + 1) is keyframe 1
			for (int w = 0; w < 8; w++) ok &= std::isfinite(ro[(size_t)w * B + b]) ? 1 : 0;
		}
		ok &= t.contactScheduleInfo().period == K && c.obstacleScheduleInfo().period == K;
		// 3. a rewind replays the floor (the clearance summaries start over with it)
		c.resetClearanceSummary();
		c.rewindEnvironment(0);
		c.rolloutAsync(K, 5e-4, 2, no_gravity);
		const std::vector<double> cs2 = c.clearanceSummary();
		for (int b = 0; b < B; b++) ok &= cs2[(size_t)2 * B + b] == cs[(size_t)2 * B + b] && cs2[(size_t)3 * B + b] == 2.0;
		// ... and a rewind to a period past the jump starts inside the collision
		c.resetClearanceSummary();
		c.rewindEnvironment(3);
		c.rolloutAsync(2, 5e-4, 2, no_gravity);
		const std::vector<double> cs3 = c.clearanceSummary();
		for (int b = 0; b < B; b++) ok &= cs3[(size_t)2 * B + b] == 2.0 && cs3[(size_t)3 * B + b] == 0.0;
		// 4. the attachment takes its schedule with it
		c.detachClearance();
		ok &= throws<std::runtime_error>([&] { c.obstacleScheduleInfo(); });
		t.clearContactSchedule();
		ok &= t.contactVelocityDevice() == nullptr;
		t.setContactPlanes(planes);
		t.detachContactPlanes();
		printf("%d of %d instances touched the rising table; the floor collided in %g of %d periods from period %g on\n", touching, B, cs[(size_t)2 * B], K, cs[(size_t)3 * B]);
		std::cout << (ok ? "ENV_SCHEDULE_RUN_OK" : "ENV_SCHEDULE_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
