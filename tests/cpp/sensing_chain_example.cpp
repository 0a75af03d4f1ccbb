// The sensing chain through the C++ facade: a Panda with the full motion-force task and a posture task behind it whose joint measurements
// arrive two samples late.
//   sensing_chain_example <robot.txt> cfgonly            no device: the argument and order errors
//   sensing_chain_example <robot.txt> run <B> <q.bin>    on GPU 0 from the postures q [dof][B]: both stacks are driven through the same
//       prescribed states with encoder offsets attached; the one with a chain of delay 2 reads, bit for bit, what its twin without a chain
//       read two samples earlier (the first sample before that), the true state keeps its bits, the taps hold the last samples, and after the
//       chain is detached the controller computes the twin's torques again
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
		s.controller->reinitializeTasks();
	}
	return s;
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const int n = 7;
	if (std::string(argv[2]) == "cfgonly") {
		Stack s = make_stack(links, 4, -1, {});
		RobotController& c = *s.controller;
		const std::vector<double> table((size_t)n * SAIP_SENSE_CHAIN_WORDS, 0.0);
		auto with = [&](int j, int word, double v) {
			std::vector<double> t = table;
			t[(size_t)j * SAIP_SENSE_CHAIN_WORDS + word] = v;
			return t;
		};
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(std::vector<double>(27, 0.0), false, 2, 1e-3); });  // shape
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(table, true, 2, 1e-3); });                          // [7][4][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(table, false, 9, 1e-3); });                         // depth
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(table, false, -1, 1e-3); });
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(table, false, 2, 0.0); });                          // sample time
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(with(1, 0, 3.0), false, 2, 1e-3); });               // delay > depth
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(with(1, 0, 0.5), false, 2, 1e-3); });               // delay not whole
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(with(2, 1, 2.0), false, 2, 1e-3); });               // vel_mode
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(with(3, 2, 1.5), false, 2, 1e-3); });               // a_q > 1
		ok &= throws<std::invalid_argument>([&] { c.attachSensingChain(with(6, 3, std::nan("")), false, 2, 1e-3); });      // NaN
		// valid arguments reach the order check: no sensing model is attached, so everything else refuses too
		ok &= throws<std::runtime_error>([&] { c.attachSensingChain({}, false, 0, 1e-3); });
		ok &= throws<std::runtime_error>([&] { c.attachSensingChain(with(1, 0, 2.0), false, 2, 1e-3); });
		ok &= throws<std::runtime_error>([&] { c.sensingChainInfo(); });
		ok &= throws<std::runtime_error>([&] { c.detachSensingChain(); });
		ok &= throws<std::runtime_error>([&] { c.resetSensingChain(); });
		ok &= throws<std::runtime_error>([&] { c.setSensingChainTable(table); });
		ok &= throws<std::runtime_error>([&] { c.sensingChainRandomize(1, 0, table, table); });
		ok &= throws<std::runtime_error>([&] { c.sensingChainState(); });
		ok &= c.sensingChainTableDevice() == nullptr;
		ok &= RobotController::sensingChainAlpha(50.0, 1e-3) == 1.0 - std::exp(-2.0 * M_PI * 50.0 * 1e-3);
		std::cout << (ok ? "SENSING_CHAIN_CFG_OK" : "SENSING_CHAIN_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 5) {
		const int B = atoi(argv[3]), P = 6, D = 2;
		std::vector<double> q0((size_t)n * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)q0.data(), q0.size() * sizeof(double));
		if (!f) return 3;
		std::vector<double> joints((size_t)n * SAIP_SENSE_JOINT_WORDS, 0.0), table((size_t)n * SAIP_SENSE_CHAIN_WORDS, 0.0);
		for (int j = 0; j < n; j++) {
			joints[(size_t)j * SAIP_SENSE_JOINT_WORDS + 0] = 0.004 * (j + 1) * (j % 2 ? -1.0 : 1.0);
			joints[(size_t)j * SAIP_SENSE_JOINT_WORDS + 1] = 1e-4;  // an encoder step
			table[(size_t)j * SAIP_SENSE_CHAIN_WORDS + 0] = D;
		}
		Stack a = make_stack(links, B, 0, q0), b = make_stack(links, B, 0, q0);
		a.controller->attachSensing(joints);
		b.controller->attachSensing(joints);
		a.controller->attachSensingChain(table, false, 4, 1e-3);
		const RobotController::SensingChainInfo info = a.controller->sensingChainInfo();
		const size_t ld = ((size_t)B + 31) / 32 * 32;  // the default leading dimension
		int ok = info.attached == 1 && info.per_instance == 0 && info.depth == 4 && info.sample_time == 1e-3 && info.state_bytes == ((size_t)(2 * 4 + 3) * 8 + 4) * n * ld;
		ok &= b.controller->sensingChainInfo().attached == 0;
		std::vector<std::vector<double>> qm_twin(P), dqm_twin(P), tau_twin(P);
		for (int p = 0; p < P; p++) {
			std::vector<double> q(q0.size()), dq(q0.size());
			for (int j = 0; j < n; j++)
				for (int i = 0; i < B; i++) {
					const size_t k = (size_t)j * B + i;
					q[k] = q0[k] + 0.05 * std::sin(0.7 * i + j + 0.4 * p);
					dq[k] = 0.2 * std::cos(0.3 * i - j + 0.4 * p);
				}
			std::vector<double> qm, dqm;
			for (Stack* s : {&b, &a}) {
				s->robot->setQ(q);
				s->robot->setDq(dq);
				s->robot->updateModel();
				s->controller->updateControllerTaskModels();
			}
			tau_twin[p] = b.controller->computeControlTorques();  // the cycle takes the measurement itself: one sample
			b.controller->measuredState(qm_twin[p], dqm_twin[p]);
			const std::vector<double> tau = a.controller->computeControlTorques();
			a.controller->measuredState(qm, dqm);
			const int src = p - D > 0 ? p - D : 0;
			ok &= same_bits(qm, qm_twin[src]) && same_bits(dqm, dqm_twin[src]);
			if (p >= 1 && p <= D) ok &= !same_bits(qm, qm_twin[p]);  // (the delay matters)
			a.controller->pullState();
			ok &= same_bits(a.robot->q(), q) && same_bits(a.robot->dq(), dq);  // the true state keeps its bits
			for (double v : tau) ok &= std::isfinite(v);
		}
		const RobotController::SensingChainState st = a.controller->sensingChainState();
		ok &= st.taps.size() == (size_t)n * 2 * 4 * B && st.filt.size() == (size_t)n * 3 * B && st.primed.size() == (size_t)n * B;
		for (int v : st.primed) ok &= v == 1;
		// tap 0 of q holds the last sample, tap 1 the one before
		for (int j = 0; j < n; j++)
			for (int i = 0; i < B; i++) {
				ok &= st.taps[(((size_t)j * 2 + 0) * 4 + 0) * B + i] == qm_twin[P - 1][(size_t)j * B + i];
				ok &= st.taps[(((size_t)j * 2 + 1) * 4 + 1) * B + i] == dqm_twin[P - 2][(size_t)j * B + i];
			}
		a.controller->detachSensingChain();
		ok &= a.controller->sensingChainInfo().attached == 0 && a.controller->sensingChainTableDevice() == nullptr;
		a.controller->updateControllerTaskModels();  // detached: the sensing model alone measures again
		const std::vector<double> tau = a.controller->computeControlTorques();
		ok &= same_bits(tau, tau_twin[P - 1]);
		a.controller->attachSensingChain({}, false, 0, 1e-3);
		a.controller->detachSensing();  // detaches the chain first
		ok &= a.controller->measuredQDevice() == nullptr && a.controller->sensingChainTableDevice() == nullptr;
		std::cout << (ok ? "SENSING_CHAIN_RUN_OK" : "SENSING_CHAIN_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
