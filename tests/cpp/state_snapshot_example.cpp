// State snapshots through the C++ facade: the loop of a sampling MPC on a Panda stack with internal OTGs.
//   state_snapshot_example <robot.txt> cfgonly               no device: the error behaviour of the facade
//   state_snapshot_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from q ([dof][B] doubles, at rest): save; K periods (run A); restore,
//       K periods again == A bit for bit; restore instance B-1 into all, K periods == column B-1 of A in every column (1e-5 relative); the
//       blob survives a round trip through host memory; a map with an entry of B is refused
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

// one Panda stack [MotionForceTask, JointTask] with the internal OTGs on (the reference default)
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
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		robot_controller = std::make_unique<RobotController>(robot, task_list);
	}
};

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
	return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}
struct End {
	std::vector<double> q, dq, tau;
};
static End roll(Stack& s, int K) {
	const double no_gravity[3] = {0.0, 0.0, 0.0};
	s.robot_controller->rolloutAsync(K, 1e-3, 1, no_gravity);
	s.robot_controller->synchronize();
	s.robot_controller->pullState();
	return {s.robot->q(), s.robot->dq(), s.robot_controller->getTorques()};
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		int ok = 1;
		ok &= throws<std::runtime_error>([&] { s.robot_controller->saveState(); });               // no device
		ok &= throws<std::runtime_error>([&] { s.robot_controller->createStateSnapshot(); });
		RobotController::StateSnapshot empty;
		ok &= !empty.valid() && empty.bytes() == 0 && empty.segments().empty();
		ok &= throws<std::invalid_argument>([&] { s.robot_controller->restoreState(empty); });    // null snapshot
		ok &= throws<std::invalid_argument>([&] { s.robot_controller->restoreState(empty, std::vector<int>(3, 0)); });
		ok &= throws<std::runtime_error>([&] { s.robot_controller->stateSnapshotFromBytes(std::vector<unsigned char>(1024, 0)); });  // no device to create it on
		ok &= saip_snapshot_import_host(s.robot_controller->handle(), nullptr, std::vector<unsigned char>(1024, 0).data(), 1024) == SAIP_ERR_INVALID_ARGUMENT;  // bad magic
		std::cout << (ok ? "SNAPSHOT_CFG_OK" : "SNAPSHOT_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		Stack s(links, B, 0);
		const int n = s.robot->dof();
		std::vector<double> q((size_t)n * B);
		std::ifstream f(argv[5], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		if (!f) return 3;
		s.robot->setQ(q);
		s.robot->setDq(std::vector<double>((size_t)n * B, 0.0));
		s.robot->updateModel();
		s.robot_controller->reinitializeTasks();
		std::vector<double> goal = s.motion_force_task->getCurrentPosition();
		for (int b = 0; b < B; b++) goal[(size_t)2 * B + b] += 0.03 + 0.001 * b;  // every instance its own goal height
		s.motion_force_task->setGoalPosition(goal);
		s.robot_controller->updateControllerTaskModels();
		roll(s, 3);
		RobotController::StateSnapshot snap = s.robot_controller->saveState();
		int ok = 1;
		bool has_otg = false;
		for (const auto& seg : snap.segments()) has_otg = has_otg || seg.name == "task0.otg.state";
		ok &= has_otg && snap.bytes() > 256;
		const End A = roll(s, K);
		const End other = roll(s, K);
		ok &= !same_bits(other.q, A.q);                                   // without a restore the next K periods end elsewhere
		s.robot_controller->restoreState(snap);
		const End again = roll(s, K);
		ok &= same_bits(again.q, A.q) && same_bits(again.dq, A.dq) && same_bits(again.tau, A.tau);
		// the candidate loop of a sampling MPC: the state of one instance into all of them
		s.robot_controller->restoreState(snap, B - 1);
		const End all = roll(s, K);
		double worst = 0.0;
		for (int j = 0; j < n; j++) {
			double scale = 1e-300, diff = 0.0;
			for (int b = 0; b < B; b++) {
				scale = std::max(scale, std::fabs(A.tau[(size_t)j * B + B - 1]));
				diff = std::max(diff, std::fabs(all.tau[(size_t)j * B + b] - A.tau[(size_t)j * B + B - 1]));
				diff = std::max(diff, std::fabs(all.q[(size_t)j * B + b] - A.q[(size_t)j * B + B - 1]));
			}
			worst = std::max(worst, diff / std::max(scale, 1.0));
		}
		ok &= worst <= 1e-5;
		// through host memory and back
		const std::vector<unsigned char> blob = snap.tobytes();
		RobotController::StateSnapshot copy = s.robot_controller->stateSnapshotFromBytes(blob);
		ok &= copy.tobytes() == blob;
		s.robot_controller->restoreState(copy);
		const End third = roll(s, K);
		ok &= same_bits(third.q, A.q) && same_bits(third.tau, A.tau);
		std::vector<int> bad((size_t)B, 0);
		bad[B / 2] = B;
		ok &= throws<std::invalid_argument>([&] { s.robot_controller->restoreState(snap, bad); });
		std::cout << (ok ? "SNAPSHOT_RUN_OK" : "SNAPSHOT_RUN_FAIL") << " broadcast worst " << worst << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
