// The pushed object through the C++ facade: the end-effector sphere of a Panda pushes a one-sphere body, inside rollouts.
//   link_object_example <robot.txt> cfgonly               no device: the argument and order errors
//   link_object_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from the postures q ([dof][B] doubles), at rest, no gravity; the example
//       checks itself: the body starts 2 cm inside the end-effector sphere on its +x side and K rollout periods push it along +x in every
//       instance; the readout and the summaries say so; an evaluation does not move it; the state round trip normalises the quaternion;
//       detaching link contact detaches the object
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
	const std::vector<RobotController::ClearanceSphere> spheres = {{"end-effector", {0.0, 0.0, 0.03}, 0.04}};
	const std::vector<double> obstacles = {1, 0.0, 0.0, 1.0, -50.0, 0, 0, 0};  // a floor far below: nothing of the world is in reach
	const std::vector<double> materials = {1.0e4, 10.0, 0.5, 1e-3};
	const std::vector<RobotController::ObjectSphere> body = {{{0.0, 0.0, 0.0}, 0.05}};
	const std::vector<double> material = {5.0e3, 5.0, 0.3, 1e-3}, inertial = {0.5, 1e-3, 1e-3, 1e-3};
	using Body = std::vector<RobotController::ObjectSphere>;
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(body, {5.0e3, 5.0, 0.3}, inertial); });                     // [4] material expected
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(body, material, {0.5, 1e-3, 1e-3}); });                     // [4] inertial expected
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(body, material, inertial, true); });                        // [4][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(Body{}, material, inertial); });                            // 0 spheres
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(Body(9, body[0]), material, inertial); });                  // above the maximum
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(Body{{{0, NAN, 0}, 0.05}}, material, inertial); });
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(Body{{{0, 0, 0}, -0.05}}, material, inertial); });          // radius below 0
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(body, {5.0e3, 5.0, 0.3, 0.0}, inertial); });                // friction without v_s
		ok &= throws<std::invalid_argument>([&] { c.attachLinkObject(body, material, {0.0, 1e-3, 1e-3, 1e-3}); });               // no mass
		ok &= throws<std::invalid_argument>([&] { c.setObjectState(std::vector<double>(12, 0.0)); });
		ok &= throws<std::invalid_argument>([&] { c.objectCost({0, 0, 0}, 1.0, {1, 0, 0}); });
		// valid arguments: the object is the second stage of a link contact that is not attached; so every other entry refuses
		ok &= throws<std::runtime_error>([&] { c.attachLinkObject(body, material, inertial); });
		ok &= throws<std::runtime_error>([&] { c.detachLinkObject(); });
		ok &= throws<std::runtime_error>([&] { c.linkObjectInfo(); });
		ok &= throws<std::runtime_error>([&] { c.setObjectState(std::vector<double>(13, 1.0)); });
		ok &= throws<std::runtime_error>([&] { c.objectState(); });
		ok &= throws<std::runtime_error>([&] { c.objectReadout(); });
		ok &= throws<std::runtime_error>([&] { c.objectSummary(); });
		ok &= throws<std::runtime_error>([&] { c.resetObjectSummary(); });
		ok &= throws<std::runtime_error>([&] { c.objectCost({0, 0, 0}, 1.0); });
		ok &= c.objectStateDevice() == nullptr && saip_batch_link_object_readout_device(c.handle()) == nullptr && saip_batch_link_object_summary_device(c.handle()) == nullptr;
		std::cout << (ok ? "LINK_OBJECT_CFG_OK" : "LINK_OBJECT_CFG_FAIL") << std::endl;
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
		c.attachLinkContact(spheres, obstacles, materials);
		c.attachLinkObject(body, material, inertial);
		ok &= throws<std::runtime_error>([&] { c.attachLinkObject(body, material, inertial); });  // twice
		const RobotController::LinkObjectInfo info = c.linkObjectInfo();
		ok &= info.n_spheres == 1 && !info.per_instance && c.objectStateDevice() != nullptr;
		// the body 2 cm inside the end-effector sphere of its instance, on the +x side; the quaternion comes back normalised
		const std::vector<double> ee = s.robot->position("end-effector", spheres[0].centre.data());  // [3][B]
		std::vector<double> x0((size_t)SAIP_LINK_OBJECT_STATE_ROWS * B, 0.0);
		for (int b = 0; b < B; b++) {
			for (int e = 0; e < 3; e++) x0[(size_t)e * B + b] = ee[(size_t)e * B + b] + (e == 0 ? 0.07 : 0.0);
			x0[(size_t)3 * B + b] = 2.0;
		}
		c.setObjectState(x0);
		std::vector<double> x = c.objectState();
		for (int b = 0; b < B; b++) ok &= x[(size_t)3 * B + b] == 1.0 && x[b] == x0[b];
		ok &= throws<std::invalid_argument>([&] { c.setObjectState(std::vector<double>(13, 0.0)); });  // a zero quaternion
		// an evaluation sees the contact and moves nothing
		c.evaluateLinkContact();
		const std::vector<double> ro = c.objectReadout();
		const std::vector<double> x1 = c.objectState();
		for (int b = 0; b < B; b++) {
			ok &= ro[(size_t)11 * B + b] == 1.0 && ro[b] > 0.0 && std::fabs(ro[(size_t)9 * B + b] + 0.02) < 1e-9;
			for (int r = 0; r < SAIP_LINK_OBJECT_STATE_ROWS; r++) ok &= x1[(size_t)r * B + b] == x[(size_t)r * B + b];
		}
		// K periods: pushed along +x, and the summaries say so
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		c.rolloutAsync(K, 5e-4, 2, no_gravity);
		x = c.objectState();
		const std::vector<double> sm = c.objectSummary();
		double least = 1e300;
		for (int b = 0; b < B; b++) {
			least = std::fmin(least, x[b] - x0[b]);
			ok &= x[b] > x0[b] && x[(size_t)7 * B + b] > 0.0 && sm[b] > 0.0 && sm[(size_t)B + b] > 0.0 && sm[(size_t)2 * B + b] == 0.0 && sm[(size_t)3 * B + b] >= 1.0 &&
				  sm[(size_t)3 * B + b] <= 2.0 * K;
		}
		ok &= throws<std::runtime_error>([&] { c.objectCost({0, 0, 0}, 1.0); });  // no sampler is attached
		c.resetObjectSummary();
		const std::vector<double> z = c.objectSummary();
		for (size_t i = 0; i < z.size(); i++) ok &= z[i] == 0.0;
		c.detachLinkContact();  // takes the object with it
		ok &= throws<std::runtime_error>([&] { c.objectState(); }) && c.objectStateDevice() == nullptr;
		printf("the body moved at least %.3e m along +x in %d periods, %d instances\n", least, K, B);
		std::cout << (ok ? "LINK_OBJECT_RUN_OK" : "LINK_OBJECT_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
