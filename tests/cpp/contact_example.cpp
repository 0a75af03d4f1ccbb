// Contact planes and the simulated force sensor through the C++ facade: a Panda with a config-13-like stack (force space along the world z
// axis under closed-loop force control with the passivity observer, a posture task behind) presses on a table with 5 N.
//   contact_example <robot.txt> cfgonly            no device: the argument and order errors
//   contact_example <robot.txt> run <B> <K> <q.bin>   K closed-loop periods on GPU 0 from the postures q [dof][B]; the example checks itself:
//       every instance in contact, pushed up by the table, penetration below 2 * 5 N / k, no status flag, everything finite
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

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	const double k = 2.0e4;
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		const std::vector<double> table = {0, 0, 1, 0.3, k, 400.0, 0.3, 1e-3};
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes(table, 2); });                    // shape
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes(table, 1, {0, 0, 0}, true, true); });  // [1][8][B] expected
		ok &= throws<std::invalid_argument>([&] { joint_task->attachContactPlanes(table, 1); });                           // not a motion-force task
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes({0, 0, 0, 0.3, k, 400.0, 0.3, 1e-3}, 1); });   // zero normal
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes({0, 0, 1, 0.3, 0.0, 400.0, 0.3, 1e-3}, 1); }); // k = 0
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes({0, 0, 1, 0.3, k, -1.0, 0.3, 1e-3}, 1); });    // c < 0
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPlanes({0, 0, 1, 0.3, k, 400.0, 0.3, 0.0}, 1); });    // v_s = 0
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { motion_force_task->attachContactPlanes(table, 1, {0.0, 0.0, 0.02}); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->contactReadout(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->contactSummary(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->resetContactSummary(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->setContactPlanes(table); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->detachContactPlanes(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.contactSense(); });
		ok &= motion_force_task->contactPlanesDevice() == nullptr;
		std::cout << (ok ? "CONTACT_CFG_OK" : "CONTACT_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> q((size_t)n * B);
		std::ifstream f(argv[5], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		if (!f) return 3;
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		motion_force_task->disableInternalOtg();
		motion_force_task->parametrizeForceMotionSpaces(1, 0.0, 0.0, 1.0);
		motion_force_task->setForceControlGains(0.9, 12.0, 1.7);
		motion_force_task->setClosedLoopForceControl(true);
		motion_force_task->enablePassivity();
		auto joint_task = std::make_shared<JointTask>(robot);
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		robot->setQ(q);
		robot->setDq(std::vector<double>((size_t)n * B, 0.0));
		robot->updateModel();
		robot_controller.reinitializeTasks();
		std::vector<double> force((size_t)3 * B, 0.0);
		for (int i = 0; i < B; i++) force[(size_t)2 * B + i] = -5.0;      // the robot presses down with 5 N
		motion_force_task->setGoalForce(force);
		robot_controller.updateControllerTaskModels();
		// a table facing up, 0.1 mm above every instance's control point
		std::vector<double> p = motion_force_task->getCurrentPosition();
		std::vector<double> planes((size_t)SAIP_CONTACT_PLANE_WORDS * B);
		const double row[8] = {0, 0, 1, 0, k, 400.0, 0.3, 1e-3};
		for (int w = 0; w < 8; w++)
			for (int i = 0; i < B; i++) planes[(size_t)w * B + i] = w == 3 ? p[(size_t)2 * B + i] + 1e-4 : row[w];
		motion_force_task->attachContactPlanes(planes, 1, {0.0, 0.0, 0.0}, true, true);
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		robot_controller.rolloutAsync(K, 5e-4, 2, no_gravity);
		robot_controller.synchronize();
		std::vector<double> ro = motion_force_task->contactReadout(), sm = motion_force_task->contactSummary();
		robot_controller.pullState();
		std::vector<double> torques = robot_controller.getTorques();
		int ok = 1;
		double fmin = 1e300, pen = 0.0;
		for (int i = 0; i < B; i++) {
			ok &= ro[(size_t)7 * B + i] == 1.0;                            // in contact
			ok &= ro[(size_t)2 * B + i] > 0.0;                             // pushed up by the table
			ok &= -ro[(size_t)6 * B + i] < 2.0 * 5.0 / k;                  // penetration
			ok &= robot_controller.status()[i] == 0;
			ok &= sm[(size_t)3 * B + i] > 0.0;
			fmin = std::fmin(fmin, ro[(size_t)2 * B + i]);
			pen = std::fmax(pen, -ro[(size_t)6 * B + i]);
		}
		for (double v : ro) ok &= std::isfinite(v);
		for (double v : sm) ok &= std::isfinite(v);
		for (double v : robot->q()) ok &= std::isfinite(v);
		for (double v : robot->dq()) ok &= std::isfinite(v);
		for (double v : torques) ok &= std::isfinite(v);
		motion_force_task->detachContactPlanes();
		ok &= motion_force_task->contactPlanesDevice() == nullptr;
		printf("smallest f_z %.3f N, largest penetration %.3e m (bound %.3e)\n", fmin, pen, 2.0 * 5.0 / k);
		std::cout << (ok ? "CONTACT_RUN_OK" : "CONTACT_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
