// Goal schedules through the C++ facade: the circle of the reference's example 06 (goal position, linear velocity and linear acceleration
// of a MotionForceTask as functions of time, 0.1 m radius at 0.3 Hz in the x-z plane around the initial position) as keyframes resident
// on the device, one per control period, followed by one rolloutAsync(K) -- against the host-driven loop of the example: K x
// {setGoalPosition, setGoalLinearVelocity, setGoalLinearAcceleration, rolloutAsync(1)}.
//   goal_schedule_example <robot.txt> cfgonly                no device: the schedule's argument and order errors
//   goal_schedule_example <robot.txt> run <B> <K> <q.bin>    both loops on GPU 0 from q ([dof][B] doubles, at rest); they must agree bit for bit
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

// one Panda stack [MotionForceTask, JointTask] without internal OTGs
struct Stack {
	std::shared_ptr<SaiModel> robot;
	std::shared_ptr<MotionForceTask> motion_force_task;
	std::shared_ptr<JointTask> joint_task;
	std::unique_ptr<RobotController> robot_controller;
	Stack(const std::vector<saip_link_desc>& links, int B, int device) {
		const double pos_in_link[3] = {0.0, 0.0, 0.07};
		robot = std::make_shared<SaiModel>(links, B, device);
		motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		motion_force_task->disableInternalOtg();
		joint_task = std::make_shared<JointTask>(robot);
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		robot_controller = std::make_unique<RobotController>(robot, task_list);
	}
};

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
	return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		const std::vector<double> two(2 * 3, 0.0), rot(2 * 9, 0.0);
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule("pose", two, 2); });
		ok &= throws<std::invalid_argument>([&] { s.joint_task->setGoalSchedule("orientation", rot, 2); });
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule("position", two, 3); });             // size mismatch
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule("position", two, 2, 0); });          // stride
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule("position", two, 2, 1, 7); });       // mode
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule(34, 3, two, 2); });                  // past row 35
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule(2, 3, two, 2, 1, SAIP_SCHEDULE_LINEAR); });  // part of R
		ok &= throws<std::invalid_argument>([&] { s.motion_force_task->setGoalSchedule("orientation", rot, 2, 1, SAIP_SCHEDULE_LINEAR); });  // R = 0
		// valid arguments reach the device check; nothing is attached
		ok &= throws<std::runtime_error>([&] { s.motion_force_task->setGoalSchedule("position", two, 2, 4, SAIP_SCHEDULE_LINEAR); });
		ok &= throws<std::runtime_error>([&] { s.joint_task->setGoalSchedule("velocity", std::vector<double>(3 * 7 * 4, 0.0), 3); });
		ok &= throws<std::runtime_error>([&] { s.motion_force_task->clearGoalSchedule(); });
		ok &= s.motion_force_task->goalScheduleDevice() == nullptr;
		s.robot_controller->rewindGoalSchedules();
		std::cout << (ok ? "SCHEDULE_CFG_OK" : "SCHEDULE_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		const double dt = 1e-3, w = 2.0 * M_PI * 0.3, no_gravity[3] = {0.0, 0.0, 0.0};
		std::vector<double> q;
		std::vector<double> result[2][4];  // per loop: q, dq, torques, goal of the motion-force task
		for (int scheduled = 0; scheduled < 2; scheduled++) {
			Stack s(links, B, 0);
			const int n = s.robot->dof();
			if (q.empty()) {
				q.resize((size_t)n * B);
				std::ifstream f(argv[5], std::ios::binary);
				f.read((char*)q.data(), q.size() * sizeof(double));
				if (!f) return 3;
			}
			s.robot->setQ(q);
			s.robot->setDq(std::vector<double>((size_t)n * B, 0.0));
			s.robot->updateModel();
			s.robot_controller->reinitializeTasks();
			s.robot_controller->updateControllerTaskModels();
			const std::vector<double> initial_position = s.motion_force_task->getCurrentPosition();
			const std::vector<double> orientation = s.motion_force_task->getGoalOrientation();
			// goal rows 0..20 of period k: position 3, orientation 9 (kept), linear velocity 3, angular velocity 3 (zero), linear acceleration 3
			const int rows = 21;
			std::vector<double> keyframes((size_t)K * rows * B, 0.0);
			for (int k = 0; k < K; k++) {
				const double time = k * dt;
				const double p[3] = {0.1 * sin(w * time), 0.0, 0.1 * (1 - cos(w * time))};
				const double v[3] = {0.1 * w * cos(w * time), 0.0, 0.1 * w * sin(w * time)};
				const double a[3] = {-0.1 * w * w * sin(w * time), 0.0, 0.1 * w * w * cos(w * time)};
				double* frame = keyframes.data() + (size_t)k * rows * B;
				for (int b = 0; b < B; b++) {
					for (int i = 0; i < 3; i++) {
						frame[(size_t)i * B + b] = initial_position[(size_t)i * B + b] + p[i];
						frame[(size_t)(12 + i) * B + b] = v[i];
						frame[(size_t)(18 + i) * B + b] = a[i];
					}
					for (int e = 0; e < 9; e++) frame[(size_t)(3 + e) * B + b] = orientation[(size_t)e * B + b];
				}
			}
			if (scheduled) {
				s.motion_force_task->setGoalSchedule(0, rows, keyframes, K);
				s.robot_controller->rolloutAsync(K, dt, 1, no_gravity);
			} else {
				for (int k = 0; k < K; k++) {
					const double* frame = keyframes.data() + (size_t)k * rows * B;
					auto field = [&](int first) { return std::vector<double>(frame + (size_t)first * B, frame + (size_t)(first + 3) * B); };
					s.motion_force_task->setGoalPosition(field(0));
					s.motion_force_task->setGoalLinearVelocity(field(12));
					s.motion_force_task->setGoalLinearAcceleration(field(18));
					s.robot_controller->rolloutAsync(1, dt, 1, no_gravity);
				}
			}
			s.robot_controller->synchronize();
			s.robot_controller->pullState();
			result[scheduled][0] = s.robot->q();
			result[scheduled][1] = s.robot->dq();
			result[scheduled][2] = s.robot_controller->getTorques();
			result[scheduled][3] = s.motion_force_task->getGoalPosition();
			if (scheduled) s.motion_force_task->clearGoalSchedule();
		}
		int ok = 1;
		for (int i = 0; i < 4; i++) ok &= same_bits(result[0][i], result[1][i]);
		double moved = 0.0;
		for (size_t i = 0; i < q.size(); i++) moved = std::max(moved, std::fabs(result[1][0][i] - q[i]));
		ok &= moved > 1e-6;  // the arms followed the circle
		std::cout << (ok ? "SCHEDULE_RUN_OK" : "SCHEDULE_RUN_FAIL") << " moved " << moved << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
