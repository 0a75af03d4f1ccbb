// Robot-model queries through the C++ facade, with the setup lines of a control program that places its robot in the world: set the
// robot base, read the end-effector pose in the world frame and use it as the motion-force goal, then run one cycle.
//   model_queries_example <robot.txt> cfgonly                      host-logic checks without a GPU (device -1)
//   model_queries_example <robot.txt> run <B> <in.bin> <out.bin>   on GPU 0: in = q, dq as [c][B] doubles; out = [c][B] blocks: position (3),
//       rotation (9), positionInWorld (3), rotationInWorld (9), J (6n), M (n*n), jointGravityVector (n), torques (n)
#include <algorithm>
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
	const std::string link_name = "end-effector";
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	// T_world_robot: a quarter turn about z and an offset
	const double R_base[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, p_base[3] = {0.5, -0.25, 0.1};
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		int ok = 1;
		robot->setTRobotBase(R_base, p_base);
		double R[9], p[3];
		robot->TRobotBase(R, p);
		ok &= std::equal(R, R + 9, R_base) && std::equal(p, p + 3, p_base);
		// no device: every query fails loudly, none computes on the CPU; unknown links are argument errors
		ok &= throws<std::runtime_error>([&] { robot->positionInWorld(link_name, pos_in_link); });
		ok &= throws<std::runtime_error>([&] { robot->rotation(link_name); });
		ok &= throws<std::runtime_error>([&] { robot->J(link_name); });
		ok &= throws<std::runtime_error>([&] { robot->M(); });
		ok &= throws<std::runtime_error>([&] { robot->jointGravityVector(); });
		ok &= throws<std::invalid_argument>([&] { robot->position("no-such-link"); });
		// a controller built later sees the base as well
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, link_name, pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> tasks = {motion_force_task, joint_task};
		RobotController controller(robot, tasks);
		std::cout << (ok ? "MQ_CFG_OK" : "MQ_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> in((size_t)2 * n * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)in.data(), in.size() * sizeof(double));
		if (!f) return 3;
		robot->setTRobotBase(R_base, p_base);  // examples/05: robot->setTRobotBase(sim->getRobotBaseTransform(robot_name))
		robot->setQ(std::vector<double>(in.begin(), in.begin() + (size_t)n * B));
		robot->setDq(std::vector<double>(in.begin() + (size_t)n * B, in.end()));
		robot->updateModel();
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, link_name, pos_in_link);
		motion_force_task->disableInternalOtg();
		auto joint_task = std::make_shared<JointTask>(robot);
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		// examples/05: the initial pose in the world frame seeds the goal
		const std::vector<double> x_w = robot->positionInWorld(link_name, pos_in_link), R_w = robot->rotationInWorld(link_name);
		const std::vector<double> x = robot->position(link_name, pos_in_link), Rl = robot->rotation(link_name);
		robot_controller.updateControllerTaskModels();
		motion_force_task->setGoalPosition(x_w);
		motion_force_task->setGoalOrientation(R_w);
		joint_task->setGoalPosition(robot->q());
		std::vector<double> torques = robot_controller.computeControlTorques();
		// host checks: the world rows are the base-frame rows mapped through T_world_robot
		int ok = 1;
		double err = 0.0;
		for (int b = 0; b < B; b++)
			for (int i = 0; i < 3; i++) {
				double xi = p_base[i];
				for (int k = 0; k < 3; k++) xi += R_base[3 * i + k] * x[(size_t)k * B + b];
				err = std::max(err, std::fabs(xi - x_w[(size_t)i * B + b]));
				for (int j = 0; j < 3; j++) {
					double rij = 0.0;
					for (int k = 0; k < 3; k++) rij += R_base[3 * i + k] * Rl[(size_t)(3 * k + j) * B + b];
					err = std::max(err, std::fabs(rij - R_w[(size_t)(3 * i + j) * B + b]));
				}
			}
		ok &= err < 1e-12;
		// the same frame as the task's control frame: the pose readback agrees bit for bit
		ok &= motion_force_task->getCurrentPosition() == x && motion_force_task->getCurrentOrientation() == Rl;
		printf("positionInWorld: %.6f %.6f %.6f  max world-map error %.3e\n", x_w[0], x_w[B], x_w[2 * B], err);
		std::vector<double> out;
		for (const auto& v : {x, Rl, x_w, R_w, robot->J(link_name, pos_in_link), robot->M(), robot->jointGravityVector(), torques})
			out.insert(out.end(), v.begin(), v.end());
		std::ofstream o(argv[5], std::ios::binary);
		o.write((const char*)out.data(), out.size() * sizeof(double));
		std::cout << (ok ? "MQ_RUN_OK" : "MQ_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
