// A kinematic tree through the C++ facade: two arms on one torso, SaiModel(links, parent, batch, device), jointParent, and one control
// cycle of [MotionForceTask on each flange, JointTask] in a RobotController.
//   tree_example <robot.txt> topology              no device: prints jointParent of every joint (robot.txt: name type parent + the link fields)
//   tree_example <robot.txt> run <B> <in.bin> <out.bin>   one cycle on GPU 0: in = q, dq, goal_left[24], goal_right[24], goal_joint[3n] as
//       [c][B] doubles; out = the torques, [dof][B]
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../include/saip/SaiPrimitivesBatched.hpp"

using namespace SaiPrimitivesBatched;

static void read_robot(const char* path, std::vector<saip_link_desc>& links, std::vector<int>& parent) {
	std::ifstream f(path);
	int n;
	f >> n;
	links.resize(n);
	parent.resize(n);
	for (int i = 0; i < n; i++) {
		saip_link_desc& l = links[i];
		std::string name;
		memset(&l, 0, sizeof(l));
		f >> name >> l.joint_type >> parent[i];
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
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	std::vector<saip_link_desc> links;
	std::vector<int> parent;
	read_robot(argv[1], links, parent);
	if (std::string(argv[2]) == "topology") {
		auto robot = std::make_shared<SaiModel>(links, parent, 4, -1);
		std::cout << "TREE_PARENTS";
		for (int j = 0; j < robot->dof(); j++) std::cout << " " << robot->jointParent(j);
		std::cout << std::endl;
		bool threw = false;
		try {
			robot->jointParent(robot->dof());
		} catch (const std::invalid_argument&) {
			threw = true;
		}
		std::cout << (threw ? "TREE_TOPOLOGY_OK" : "TREE_TOPOLOGY_FAIL") << std::endl;
		return threw ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]);
		auto robot = std::make_shared<SaiModel>(links, parent, B, 0);
		const int n = robot->dof();
		std::vector<double> in((size_t)(2 * n + 48 + 3 * n) * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)in.data(), in.size() * sizeof(double));
		if (!f) return 3;
		auto slice = [&](size_t first, size_t comps) { return std::vector<double>(in.begin() + first * B, in.begin() + (first + comps) * B); };
		const double pos_in_link[3] = {0.0, 0.0, 0.1};
		auto left = std::make_shared<MotionForceTask>(robot, "left_link7", pos_in_link, "left");
		auto right = std::make_shared<MotionForceTask>(robot, "right_link7", pos_in_link, "right");
		auto joint_task = std::make_shared<JointTask>(robot);
		left->disableInternalOtg();
		right->disableInternalOtg();
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {left, right, joint_task};
		RobotController robot_controller(robot, task_list);
		robot->setQ(slice(0, n));
		robot->setDq(slice(n, n));
		robot->updateModel();
		robot_controller.updateControllerTaskModels();
		size_t g = 2 * n;
		for (auto& t : {left, right}) {
			t->setGoalPosition(slice(g, 3));
			t->setGoalOrientation(slice(g + 3, 9));
			t->setGoalLinearVelocity(slice(g + 12, 3));
			t->setGoalAngularVelocity(slice(g + 15, 3));
			t->setGoalLinearAcceleration(slice(g + 18, 3));
			t->setGoalAngularAcceleration(slice(g + 21, 3));
			g += 24;
		}
		joint_task->setGoalPosition(slice(g, n));
		joint_task->setGoalVelocity(slice(g + n, n));
		joint_task->setGoalAcceleration(slice(g + 2 * n, n));
		std::vector<double> control_torques = robot_controller.computeControlTorques();
		if (control_torques.size() != (size_t)n * B) return 4;
		std::ofstream o(argv[5], std::ios::binary);
		o.write((const char*)control_torques.data(), control_torques.size() * sizeof(double));
		std::cout << "TREE_RUN_OK" << std::endl;
		return 0;
	}
	return 2;
}
