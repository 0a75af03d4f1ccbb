// Contact patches through the C++ facade: a Panda with a config-13-like stack (force space along the world z axis under closed-loop force
// control with the passivity observer, a posture task behind) presses a square plate of four contact points on a table with 5 N.
//   contact_patch_example <robot.txt> cfgonly                                 no device: the argument and order errors
//   contact_patch_example <robot.txt> run <B> <K> <q.bin> <planes.bin> <out.bin>
//       K closed-loop periods on GPU 0 from the postures q [dof][B] against the per-instance planes [1][8][B]; the example checks itself
//       (every instance in contact and pushed up, no status flag, everything finite) and writes readout [20][B], summary [6][B], q, dq and
//       torques [dof][B] for the caller to compare with the Python facade
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
	const std::vector<double> square = {0.05, 0.05, 0.0, -0.05, 0.05, 0.0, -0.05, -0.05, 0.0, 0.05, -0.05, 0.0};
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		const std::vector<double> table = {0, 0, 1, 0.3, k, 400.0, 0.3, 1e-3};
		std::vector<double> nine(27, 0.0), bad = square;
		bad[4] = NAN;
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch({0.0, 0.0}, table, 1); });           // [n][3] expected
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch({}, table, 1); });
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(nine, table, 1); });                 // nine points
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(bad, table, 1); });                  // not finite
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(square, table, 2); });               // shape
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(square, table, 1, true, true); });   // [1][8][B] expected
		ok &= throws<std::invalid_argument>([&] { joint_task->attachContactPatch(square, table, 1); });                      // not a motion-force task
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(square, {0, 0, 0, 0.3, k, 400.0, 0.3, 1e-3}, 1); });  // zero normal
		ok &= throws<std::invalid_argument>([&] { motion_force_task->attachContactPatch(square, {0, 0, 1, 0.3, 0.0, 400.0, 0.3, 1e-3}, 1); });  // k = 0
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { motion_force_task->attachContactPatch(square, table, 1); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->contactPatchReadout(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->contactPatchSummary(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->resetContactPatchSummary(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->setContactPatchPlanes(table); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->detachContactPatch(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->contactPatchPoints(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.contactPatchSense(); });
		ok &= motion_force_task->contactPatchPlanesDevice() == nullptr && motion_force_task->contactPatchTorquesDevice() == nullptr;
		std::cout << (ok ? "CONTACT_PATCH_CFG_OK" : "CONTACT_PATCH_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 8) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> q((size_t)n * B), planes((size_t)SAIP_CONTACT_PLANE_WORDS * B);
		std::ifstream f(argv[5], std::ios::binary), g(argv[6], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		g.read((char*)planes.data(), planes.size() * sizeof(double));
		if (!f || !g) return 3;
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
		motion_force_task->attachContactPatch(square, planes, 1, true, true);
		int ok = motion_force_task->contactPatchPoints() == 4;
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		robot_controller.rolloutAsync(K, 5e-4, 2, no_gravity);
		robot_controller.synchronize();
		std::vector<double> ro = motion_force_task->contactPatchReadout(), sm = motion_force_task->contactPatchSummary();
		robot_controller.pullState();
		std::vector<double> torques = robot_controller.getTorques();
		double fmin = 1e300, mmax = 0.0;
		for (int i = 0; i < B; i++) {
			ok &= ro[(size_t)7 * B + i] >= 1.0;                            // a point in contact
			ok &= ro[(size_t)2 * B + i] > 0.0;                             // pushed up by the table
			ok &= robot_controller.status()[i] == 0;
			ok &= sm[(size_t)3 * B + i] > 0.0;
			fmin = std::fmin(fmin, ro[(size_t)2 * B + i]);
			mmax = std::fmax(mmax, sm[(size_t)4 * B + i]);
		}
		for (double v : ro) ok &= std::isfinite(v);
		for (double v : sm) ok &= std::isfinite(v);
		for (double v : robot->q()) ok &= std::isfinite(v);
		for (double v : robot->dq()) ok &= std::isfinite(v);
		for (double v : torques) ok &= std::isfinite(v);
		motion_force_task->detachContactPatch();
		ok &= motion_force_task->contactPatchPlanesDevice() == nullptr;
		std::ofstream o(argv[7], std::ios::binary);
		const std::vector<double>* parts[5] = {&ro, &sm, &robot->q(), &robot->dq(), &torques};
		for (const std::vector<double>* a : parts) o.write((const char*)a->data(), a->size() * sizeof(double));
		ok &= (bool)o;
		printf("smallest f_z %.3f N, largest |M| %.3e N m\n", fmin, mmax);
		std::cout << (ok ? "CONTACT_PATCH_RUN_OK" : "CONTACT_PATCH_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
