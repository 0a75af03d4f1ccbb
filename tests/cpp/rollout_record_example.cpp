// The resident pipeline and the rollout recorder through the C++ facade: a Panda stack [MotionForceTask, JointTask] in a RobotController,
// a recorded closed-loop rollout, the log and the summaries read back.
//   rollout_record_example <robot.txt> cfgonly                    no device: the recorder's argument and order errors
//   rollout_record_example <robot.txt> run <B> <K> <in.bin> <out.bin>   K recorded periods on GPU 0: in = q, dq, goal_mf[24], goal_joint[3n] as
//       [c][B] doubles; out = samples, rows, first_period, stride (as doubles), the log [samples][rows][B], the status log [samples][B] (as
//       doubles), the summaries [8][B], then q, dq [dof][B] from pullState() and the torques [dof][B] from getTorques()
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
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		auto stranger = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link, "stranger");
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(0); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(4, 0); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(4, 1, 32); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(4, 1, 0); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(4, 1, SAIP_RECORD_POSE); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.recordRollouts(4, 1, SAIP_RECORD_ERROR, stranger); });
		// valid arguments reach the device check; nothing is attached, so the readers refuse
		ok &= throws<std::runtime_error>([&] { robot_controller.recordRollouts(4, 1, SAIP_RECORD_Q | SAIP_RECORD_ERROR, motion_force_task, true); });
		ok &= throws<std::runtime_error>([&] { robot_controller.rolloutLog(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.rolloutSummary(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.resetRolloutRecorder(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.stopRecordingRollouts(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.rolloutAsync(1, 1e-3); });
		ok &= throws<std::runtime_error>([&] { robot_controller.stepAsync(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.pullState(); });
		std::cout << (ok ? "RECORD_CFG_OK" : "RECORD_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 7) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> in((size_t)(2 * n + 24 + 3 * n) * B);
		std::ifstream f(argv[5], std::ios::binary);
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
		// record every period: state, torques, pose and error of the motion-force task, with the running summaries
		const unsigned all = SAIP_RECORD_Q | SAIP_RECORD_DQ | SAIP_RECORD_TAU | SAIP_RECORD_POSE | SAIP_RECORD_ERROR;
		robot_controller.recordRollouts(K, 1, all, motion_force_task, true);
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		robot_controller.rolloutAsync(K, 5e-4, 2, no_gravity);
		robot_controller.synchronize();
		RobotController::RolloutLog log = robot_controller.rolloutLog();
		std::vector<double> summary = robot_controller.rolloutSummary();
		robot_controller.pullState();
		std::vector<double> torques = robot_controller.getTorques();
		robot_controller.stopRecordingRollouts();
		if (log.samples != K || log.rows != 3 * n + 18 || torques.size() != (size_t)n * B) return 4;
		std::ofstream o(argv[6], std::ios::binary);
		const double head[4] = {(double)log.samples, (double)log.rows, (double)log.first_period, (double)log.stride};
		o.write((const char*)head, sizeof(head));
		o.write((const char*)log.data.data(), log.data.size() * sizeof(double));
		std::vector<double> status(log.status.begin(), log.status.end());
		o.write((const char*)status.data(), status.size() * sizeof(double));
		o.write((const char*)summary.data(), summary.size() * sizeof(double));
		o.write((const char*)robot->q().data(), robot->q().size() * sizeof(double));
		o.write((const char*)robot->dq().data(), robot->dq().size() * sizeof(double));
		o.write((const char*)torques.data(), torques.size() * sizeof(double));
		std::cout << "RECORD_RUN_OK" << std::endl;
		return 0;
	}
	return 2;
}
