// The sensing model through the C++ facade: a Panda with the full motion-force task and a posture task behind it whose encoders are
// miscalibrated by a constant offset.
//   sensing_example <robot.txt> cfgonly            no device: the argument and order errors
//   sensing_example <robot.txt> run <B> <q.bin>    on GPU 0 from the postures q [dof][B]: the torques the controller computes at the true
//       state (q, dq) with offsets (q_off, dq_off) attached equal, bit for bit, those of an unattached controller whose state is
//       (q + q_off, dq + dq_off); the true state keeps its bits and the measured copy is the shifted state
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>

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

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
	return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

struct Stack {
	std::shared_ptr<SaiModel> robot;
	std::shared_ptr<MotionForceTask> motion_force_task;
	std::shared_ptr<JointTask> joint_task;
	std::shared_ptr<RobotController> controller;
};
// the config-2 stack at the state (q, dq), its goals a little away from the pose it is built at
static Stack make_stack(const std::vector<saip_link_desc>& links, int B, int device, const std::vector<double>& q0) {
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	Stack s;
	s.robot = std::make_shared<SaiModel>(links, B, device);
	s.motion_force_task = std::make_shared<MotionForceTask>(s.robot, "end-effector", pos_in_link);
	s.motion_force_task->disableInternalOtg();
	s.joint_task = std::make_shared<JointTask>(s.robot);
	s.joint_task->disableInternalOtg();
	std::vector<std::shared_ptr<TemplateTask>> task_list = {s.motion_force_task, s.joint_task};
	s.controller = std::make_shared<RobotController>(s.robot, task_list);
	if (device >= 0) {
		s.robot->setQ(q0);
		s.robot->setDq(std::vector<double>(q0.size(), 0.0));
		s.robot->updateModel();
		s.controller->reinitializeTasks();  // the goals are the pose and posture of q0 in both stacks
	}
	return s;
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	if (std::string(argv[2]) == "cfgonly") {
		Stack s = make_stack(links, 4, -1, {});
		RobotController& c = *s.controller;
		const std::vector<double> joints((size_t)7 * SAIP_SENSE_JOINT_WORDS, 0.0), table((size_t)SAIP_SENSE_WRENCH_WORDS, 0.0);
		auto with = [&](int j, int word, double v) {
			std::vector<double> t = joints;
			t[(size_t)j * SAIP_SENSE_JOINT_WORDS + word] = v;
			return t;
		};
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(std::vector<double>(41, 0.0)); });                       // shape
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(joints, {}, true); });                                    // [7][6][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachSensing({}, {{0, {1.0, 2.0}}}); });                               // 18 words
		ok &= throws<std::invalid_argument>([&] { c.attachSensing({}, {{0, table}, {0, table}}); });                        // a task named twice
		ok &= throws<std::invalid_argument>([&] { c.attachSensing({}, {{1, table}}); });                                    // not a motion-force task
		ok &= throws<std::invalid_argument>([&] { c.attachSensing({}, {{0, table}, {0, table}, {0, table}}); });            // three wrench tasks
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(with(1, 1, -1.0)); });                                    // q_res < 0
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(with(3, 5, -1e-3)); });                                   // dq_sigma < 0
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(with(0, 0, std::numeric_limits<double>::infinity())); }); // q_off infinite
		ok &= throws<std::invalid_argument>([&] { c.attachSensing(with(6, 3, std::nan(""))); });                            // NaN
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { c.attachSensing(); });
		ok &= throws<std::runtime_error>([&] { c.attachSensing(with(1, 0, 0.01), {{0, table}}, false, 7); });
		ok &= throws<std::runtime_error>([&] { c.sensingInfo(); });
		ok &= throws<std::runtime_error>([&] { c.measureState(); });
		ok &= throws<std::runtime_error>([&] { c.setSensingPeriod(3); });
		ok &= throws<std::runtime_error>([&] { c.setSensingSeed(3); });
		ok &= throws<std::runtime_error>([&] { c.setSensingJoints(joints); });
		ok &= throws<std::runtime_error>([&] { c.sensingRandomize(1, 0, joints, joints); });
		ok &= throws<std::runtime_error>([&] { c.detachSensing(); });
		ok &= c.measuredQDevice() == nullptr && c.measuredDqDevice() == nullptr && c.sensingJointsDevice() == nullptr && c.sensingWrenchesDevice() == nullptr;
		std::cout << (ok ? "SENSING_CFG_OK" : "SENSING_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 5) {
		const int B = atoi(argv[3]);
		const int n = 7;
		std::vector<double> q0((size_t)n * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)q0.data(), q0.size() * sizeof(double));
		if (!f) return 3;
		// the true state: away from q0 (where the goals are), moving; the offsets differ from joint to joint
		std::vector<double> q(q0.size()), dq(q0.size()), qs(q0.size()), dqs(q0.size()), joints((size_t)n * SAIP_SENSE_JOINT_WORDS, 0.0);
		for (int j = 0; j < n; j++) {
			const double q_off = 0.004 * (j + 1) * (j % 2 ? -1.0 : 1.0), dq_off = 0.01 * (n - j) * (j % 3 ? 1.0 : -1.0);
			joints[(size_t)j * SAIP_SENSE_JOINT_WORDS + 0] = q_off;
			joints[(size_t)j * SAIP_SENSE_JOINT_WORDS + 3] = dq_off;
			for (int i = 0; i < B; i++) {
				const size_t k = (size_t)j * B + i;
				q[k] = q0[k] + 0.05 * std::sin(0.7 * i + j);
				dq[k] = 0.2 * std::cos(0.3 * i - j);
				qs[k] = q[k] + q_off;  // rounded once, as the kernel does
				dqs[k] = dq[k] + dq_off;
			}
		}
		Stack a = make_stack(links, B, 0, q0), b = make_stack(links, B, 0, q0), plain = make_stack(links, B, 0, q0);
		auto torques_at = [&](Stack& s, const std::vector<double>& qq, const std::vector<double>& dd) {
			s.robot->setQ(qq);
			s.robot->setDq(dd);
			s.robot->updateModel();
			s.controller->updateControllerTaskModels();
			return s.controller->computeControlTorques();
		};
		a.controller->attachSensing(joints);
		const std::vector<double> tau_sensed = torques_at(a, q, dq);
		const std::vector<uint8_t> status_sensed = a.controller->status();
		std::vector<double> qm, dqm;
		a.controller->measuredState(qm, dqm);
		a.controller->pullState();
		int ok = same_bits(a.robot->q(), q) && same_bits(a.robot->dq(), dq);  // the true state keeps its bits
		ok &= same_bits(qm, qs) && same_bits(dqm, dqs);
		const RobotController::SensingInfo info = a.controller->sensingInfo();
		ok &= info.per_instance_joints == 0 && info.n_wrench_tasks == 0 && info.period == 0;
		const std::vector<double> tau_shifted = torques_at(b, qs, dqs);
		ok &= same_bits(tau_sensed, tau_shifted) && status_sensed == b.controller->status();
		ok &= !same_bits(torques_at(plain, q, dq), tau_sensed);  // (the offsets matter)
		for (double v : tau_sensed) ok &= std::isfinite(v);
		a.controller->detachSensing();
		ok &= a.controller->measuredQDevice() == nullptr;
		ok &= same_bits(torques_at(a, qs, dqs), tau_shifted);    // detached: the controller reads the state again
		std::cout << (ok ? "SENSING_RUN_OK" : "SENSING_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
