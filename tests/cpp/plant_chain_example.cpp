// The actuation chain through the C++ facade: a Panda with the full motion-force task and a posture task behind it whose torque commands
// reach the joints two control periods late.
//   plant_chain_example <robot.txt> cfgonly            no device: the argument and order errors
//   plant_chain_example <robot.txt> run <B> <q.bin>    on GPU 0 from the postures q [dof][B]: both stacks are driven through the same
//       prescribed states behind a plant with a weak, saturating actuator; the one with a chain of delay 2 actuates, bit for bit, what its
//       twin without a chain actuated two periods earlier (the first period's torques before that), the commanded torques keep their bits,
//       the taps hold the last commands, and after the chain is detached the plant actuates the twin's torques again
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>

#include "../../include/saip/SaiPrimitivesBatched.hpp"

using namespace SaiPrimitivesBatched;

extern "C" int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);  // kind 2: device to host

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

// the actuated torques of the last substep, [dof][B], from the device array [dof][ld]
static std::vector<double> actuated(RobotController& c, int n, int B, size_t ld) {
	c.synchronize();
	std::vector<double> raw((size_t)n * ld), out((size_t)n * B);
	if (hipMemcpy(raw.data(), c.plantTorquesDevice(), raw.size() * sizeof(double), 2) != 0) throw std::runtime_error("hipMemcpy failed");
	for (int j = 0; j < n; j++)
		for (int i = 0; i < B; i++) out[(size_t)j * B + i] = raw[(size_t)j * ld + i];
	return out;
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const int n = 7;
	if (std::string(argv[2]) == "cfgonly") {
		Stack s = make_stack(links, 4, -1, {});
		RobotController& c = *s.controller;
		const std::vector<double> table = c.neutralActuationChainTable();
		auto with = [&](int j, int word, double v) {
			std::vector<double> t = table;
			t[(size_t)j * SAIP_PLANT_CHAIN_WORDS + word] = v;
			return t;
		};
		int ok = table.size() == (size_t)n * SAIP_PLANT_CHAIN_WORDS && table[0] == 0.0 && std::isinf(table[1]) && table[2] == 0.0;
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(std::vector<double>(20, 0.0), false, 2); });     // shape
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(table, true, 2); });                             // [7][3][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(table, false, 9); });                            // depth
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(table, false, -1); });
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(1, 0, 3.0), false, 2); });                  // delay > depth
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(1, 0, 0.5), false, 2); });                  // delay not whole
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(2, 1, 0.0), false, 2); });                  // rate_max not above 0
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(3, 2, -1e-3), false, 2); });                // tau_lag < 0
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(3, 2, INFINITY), false, 2); });             // tau_lag infinite
		ok &= throws<std::invalid_argument>([&] { c.attachActuationChain(with(6, 1, std::nan("")), false, 2); });         // NaN
		// valid arguments reach the order check: no plant model is attached, so everything else refuses too
		ok &= throws<std::runtime_error>([&] { c.attachActuationChain({}, false, 0); });
		ok &= throws<std::runtime_error>([&] { c.attachActuationChain(with(1, 0, 2.0), false, 2); });
		ok &= throws<std::runtime_error>([&] { c.actuationChainInfo(); });
		ok &= throws<std::runtime_error>([&] { c.detachActuationChain(); });
		ok &= throws<std::runtime_error>([&] { c.resetActuationChain(); });
		ok &= throws<std::runtime_error>([&] { c.setActuationChainTable(table); });
		ok &= throws<std::runtime_error>([&] { c.actuationChainRandomize(1, 0, table, table); });
		ok &= throws<std::runtime_error>([&] { c.actuationChainState(); });
		ok &= c.actuationChainTableDevice() == nullptr;
		std::cout << (ok ? "PLANT_CHAIN_CFG_OK" : "PLANT_CHAIN_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 5) {
		const int B = atoi(argv[3]), P = 6, D = 2, depth = 4;
		std::vector<double> q0((size_t)n * B);
		std::ifstream f(argv[4], std::ios::binary);
		f.read((char*)q0.data(), q0.size() * sizeof(double));
		if (!f) return 3;
		Stack a = make_stack(links, B, 0, q0), b = make_stack(links, B, 0, q0);
		// a weak actuator that saturates: what it makes of a command does not depend on the state, so the twin's torques of an earlier
		// period are the chained stack's torques of this one whatever the two states are
		std::vector<double> joints = a.controller->neutralPlantJoints(), table = a.controller->neutralActuationChainTable();
		for (int j = 0; j < n; j++) {
			joints[(size_t)j * SAIP_PLANT_JOINT_WORDS + 0] = 0.9;
			joints[(size_t)j * SAIP_PLANT_JOINT_WORDS + 2] = 4.0;
			table[(size_t)j * SAIP_PLANT_CHAIN_WORDS + 0] = D;
		}
		a.controller->attachPlant(joints);
		b.controller->attachPlant(joints);
		a.controller->attachActuationChain(table, false, depth);
		const RobotController::ActuationChainInfo info = a.controller->actuationChainInfo();
		const size_t ld = ((size_t)B + 31) / 32 * 32;  // the default leading dimension
		int ok = info.attached == 1 && info.per_instance == 0 && info.depth == depth && info.state_bytes == ((size_t)(depth + 3) * 8 + 4) * n * ld;
		ok &= b.controller->actuationChainInfo().attached == 0;
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		std::vector<std::vector<double>> act_twin(P), tau_twin(P);
		for (int p = 0; p < P; p++) {
			std::vector<double> q(q0.size()), dq(q0.size());
			for (int j = 0; j < n; j++)
				for (int i = 0; i < B; i++) {
					const size_t k = (size_t)j * B + i;
					q[k] = q0[k] + 0.05 * std::sin(0.7 * i + j + 0.4 * p);
					dq[k] = 0.2 * std::cos(0.3 * i - j + 0.4 * p);
				}
			for (Stack* s : {&b, &a}) {
				s->robot->setQ(q);
				s->robot->setDq(dq);
				s->robot->updateModel();
				s->controller->updateControllerTaskModels();
			}
			tau_twin[p] = b.controller->computeControlTorques();
			b.controller->integrate(5e-4, 3, no_gravity);
			act_twin[p] = actuated(*b.controller, n, B, ld);
			const std::vector<double> tau = a.controller->computeControlTorques();
			ok &= same_bits(tau, tau_twin[p]);  // the same state, the same command
			a.controller->integrate(5e-4, 3, no_gravity);
			const std::vector<double> act = actuated(*a.controller, n, B, ld);
			const int src = p - D > 0 ? p - D : 0;
			ok &= same_bits(act, act_twin[src]);
			if (p >= 1) ok &= !same_bits(act, act_twin[p]);  // (the delay matters)
			ok &= same_bits(a.controller->getTorques(), tau);  // the commanded torques keep their bits
			for (double v : act) ok &= std::isfinite(v);
		}
		const RobotController::ActuationChainState st = a.controller->actuationChainState();
		ok &= st.taps.size() == (size_t)n * depth * B && st.filt.size() == (size_t)n * 3 * B && st.primed.size() == (size_t)n * B;
		for (int v : st.primed) ok &= v == 1;
		// tap 0 holds the last command, tap 1 the one before; x_held is the command of two periods ago
		for (int j = 0; j < n; j++)
			for (int i = 0; i < B; i++) {
				ok &= st.taps[((size_t)j * depth + 0) * B + i] == tau_twin[P - 1][(size_t)j * B + i];
				ok &= st.taps[((size_t)j * depth + 1) * B + i] == tau_twin[P - 2][(size_t)j * B + i];
				ok &= st.filt[((size_t)j * 3 + 0) * B + i] == tau_twin[P - 1 - D][(size_t)j * B + i];
			}
		a.controller->detachActuationChain();
		ok &= a.controller->actuationChainInfo().attached == 0 && a.controller->actuationChainTableDevice() == nullptr;
		a.controller->integrate(5e-4, 1, no_gravity);  // detached: the plant alone actuates the last command
		b.controller->integrate(5e-4, 1, no_gravity);
		ok &= same_bits(actuated(*a.controller, n, B, ld), actuated(*b.controller, n, B, ld));
		a.controller->attachActuationChain({}, false, 0);
		a.controller->detachPlant();  // detaches the chain first
		ok &= a.controller->plantTorquesDevice() == nullptr && a.controller->actuationChainTableDevice() == nullptr;
		std::cout << (ok ? "PLANT_CHAIN_RUN_OK" : "PLANT_CHAIN_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
