// Task-space diagnostics through the C++ facade, with the loop calls a control program makes every cycle: read back the goal and the
// desired state (joint control), print the position / orientation error and the sensed force, check whether the goal is reached.
//   diagnostics_example <robot.txt> cfgonly                      host-logic checks without a GPU (device -1)
//   diagnostics_example <robot.txt> run <B> <in.bin> <out.bin>   one cycle on GPU 0: in = q,dq,goal0[24],goal1[3n] as [c][B] doubles;
//       out = [24][B] diagnostics, goal position [3][B], desired position [3][B], goalPositionReached(0.05) [1][B], torques [n][B]
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

// the call throws the exception type E
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
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> tasks = {motion_force_task, joint_task};
		RobotController controller(robot, tasks);
		int ok = 1;
		// no device: every getter fails loudly, none computes on the CPU
		ok &= throws<std::runtime_error>([&] { motion_force_task->getPositionError(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->getOrientationError(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->getCurrentLinearVelocity(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->getSensedForceControlWorldFrame(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->getUnitMassForce(); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->goalPositionReached(0.01); });
		ok &= throws<std::runtime_error>([&] { motion_force_task->getGoalPosition(); });
		ok &= throws<std::runtime_error>([&] { joint_task->getDesiredPosition(); });
		std::cout << (ok ? "DIAG_CFG_OK" : "DIAG_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> in((size_t)(2 * n + 24 + 3 * n) * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)in.data(), in.size() * sizeof(double));
		if (!f) return 3;
		auto slice = [&](size_t first, size_t comps) { return std::vector<double>(in.begin() + first * B, in.begin() + (first + comps) * B); };
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		motion_force_task->disableInternalOtg();
		auto joint_task = std::make_shared<JointTask>(robot);
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		robot->setQ(slice(0, n));
		robot->setDq(slice(n, n));
		robot->updateModel();
		robot_controller.updateControllerTaskModels();
		size_t g = 2 * n;
		motion_force_task->setGoalPosition(slice(g, 3));
		motion_force_task->setGoalOrientation(slice(g + 3, 9));
		motion_force_task->setGoalLinearVelocity(slice(g + 12, 3));
		motion_force_task->setGoalAngularVelocity(slice(g + 15, 3));
		motion_force_task->setGoalLinearAcceleration(slice(g + 18, 3));
		motion_force_task->setGoalAngularAcceleration(slice(g + 21, 3));
		g += 24;
		joint_task->setGoalPosition(slice(g, n));
		joint_task->setGoalVelocity(slice(g + n, n));
		joint_task->setGoalAcceleration(slice(g + 2 * n, n));
		std::vector<double> control_torques = robot_controller.computeControlTorques();
		// joint control loop: goal and desired state read back
		int ok = 1;
		ok &= joint_task->getGoalPosition() == slice(g, n) && joint_task->getGoalVelocity() == slice(g + n, n) &&
			  joint_task->getGoalAcceleration() == slice(g + 2 * n, n) && joint_task->getDesiredPosition() == slice(g, n) &&
			  joint_task->getDesiredVelocity() == slice(g + n, n) && joint_task->getDesiredAcceleration() == slice(g + 2 * n, n);
		ok &= motion_force_task->getGoalOrientation() == slice(2 * n + 3, 9) && motion_force_task->getDesiredOrientation() == slice(2 * n + 3, 9) &&
			  motion_force_task->getGoalLinearVelocity() == slice(2 * n + 12, 3) && motion_force_task->getDesiredAngularAcceleration() == slice(2 * n + 21, 3) &&
			  motion_force_task->getGoalForce() == std::vector<double>((size_t)3 * B, 0.0);
		// motion-force loop: the errors and the sensed force, printed for instance 0
		const std::vector<double> d = motion_force_task->getTaskDiagnostics();
		const std::vector<double> pe = motion_force_task->getPositionError(), oe = motion_force_task->getOrientationError(),
								  fs = motion_force_task->getSensedForceControlWorldFrame(), um = motion_force_task->getUnitMassForce();
		ok &= pe == std::vector<double>(d.begin(), d.begin() + 3 * B) && oe == std::vector<double>(d.begin() + 3 * B, d.begin() + 6 * B) &&
			  fs == std::vector<double>(d.begin() + 12 * B, d.begin() + 15 * B) && um == std::vector<double>(d.begin() + 18 * B, d.end());
		printf("position error: %.6f %.6f %.6f  orientation error: %.6f %.6f %.6f  sensed force: %.3f %.3f %.3f\n", pe[0], pe[B], pe[2 * B], oe[0],
			   oe[B], oe[2 * B], fs[0], fs[B], fs[2 * B]);
		const std::vector<bool> reached = motion_force_task->goalPositionReached(0.05);
		const std::vector<bool> reached_ori = motion_force_task->goalOrientationReached(0.05);
		ok &= (int)reached.size() == B && (int)reached_ori.size() == B;
		std::vector<double> out(d);
		for (const auto& v : {motion_force_task->getGoalPosition(), motion_force_task->getDesiredPosition()}) out.insert(out.end(), v.begin(), v.end());
		for (int b = 0; b < B; b++) out.push_back(reached[b] ? 1.0 : 0.0);
		out.insert(out.end(), control_torques.begin(), control_torques.end());
		std::ofstream o(argv[5], std::ios::binary);
		o.write((const char*)out.data(), out.size() * sizeof(double));
		std::cout << (ok ? "DIAG_RUN_OK" : "DIAG_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
