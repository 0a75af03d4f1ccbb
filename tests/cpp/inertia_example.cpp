// The inertia table through the C++ facade: a Panda with the full motion-force task and a posture task behind it holds its pose under
// gravity while every instance simulates a robot of its own -- link masses scaled, a box in the hand whose mass grows with the instance.
//   inertia_example <robot.txt> cfgonly                        no device: the argument and order errors
//   inertia_example <robot.txt> run <B> <K> <q.bin> <out.bin>  K closed-loop periods on GPU 0 from the postures q [dof][B]; writes the table
//       as read back [dof][10][B], then the resident table [dof][10][ld], padding columns included (the one call outside the facade: a
//       device-to-host copy of the HIP runtime the engine links), then q and dq [dof][B] to out.bin
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

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

// the parts of instance i of B, the same in tests/test_cpp_inertia.py: s = 0.9 + 0.2 i / B on every body, a box of (0.5 + 2 i / B) kg
static void example_parts(int n, int B, std::vector<double>& bodies, std::vector<double>& payloads) {
	bodies.assign((size_t)n * SAIP_INERTIA_BODY_WORDS * B, 0.0);
	payloads.assign((size_t)SAIP_INERTIA_PAYLOAD_WORDS * B, 0.0);
	const double box[SAIP_INERTIA_PAYLOAD_WORDS] = {0.0, 0.0, 0.0, 0.1, 0.05, 0.04, 0.03};
	for (int i = 0; i < B; i++) {
		for (int j = 0; j < n; j++) bodies[((size_t)j * SAIP_INERTIA_BODY_WORDS) * B + i] = 0.9 + 0.2 * i / B;
		for (int w = 0; w < SAIP_INERTIA_PAYLOAD_WORDS; w++) payloads[(size_t)w * B + i] = box[w];
		payloads[i] = 0.5 + 2.0 * i / B;
	}
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		std::vector<double> rows((size_t)7 * SAIP_INERTIA_ROW_WORDS, 0.0);
		for (int j = 0; j < 7; j++) {
			double* w = rows.data() + (size_t)j * SAIP_INERTIA_ROW_WORDS;
			w[0] = 2.0;
			w[4] = w[5] = w[6] = 0.01;
		}
		auto with = [&](int j, int word, double v) {
			std::vector<double> t = rows;
			t[(size_t)j * SAIP_INERTIA_ROW_WORDS + word] = v;
			return t;
		};
		int ok = 1;
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia(std::vector<double>(69, 0.0)); });           // shape
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia(rows, true); });                             // [7][10][B] expected
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia({}, false, {"no-such-link"}); });
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia({}, false, {"link4", "link5", "link6"}); }); // three payloads
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia(with(1, 0, -1.0)); });                       // m < 0
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia(with(3, 7, 0.5)); });                        // a negative eigenvalue
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachInertia(with(6, 2, std::nan(""))); });               // NaN
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { robot_controller.attachInertia(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.attachInertia(rows, false, {"end-effector", "link4"}); });
		ok &= throws<std::runtime_error>([&] { robot_controller.inertiaInfo(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.inertiaRows(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.setInertiaRows(rows); });
		ok &= throws<std::runtime_error>([&] { robot_controller.setInertiaParts({}); });
		ok &= throws<std::runtime_error>([&] { robot_controller.randomizeInertia(1, 0, {}, {}); });
		ok &= throws<std::runtime_error>([&] { robot_controller.detachInertia(); });
		ok &= robot_controller.inertiaRowsDevice() == nullptr;
		std::cout << (ok ? "INERTIA_CFG_OK" : "INERTIA_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 7) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		auto robot = std::make_shared<SaiModel>(links, B, 0);
		const int n = robot->dof();
		std::vector<double> q((size_t)n * B);
		std::ifstream f(argv[5], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		if (!f) return 3;
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		motion_force_task->disableInternalOtg();
		auto joint_task = std::make_shared<JointTask>(robot);
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		robot->setQ(q);
		robot->setDq(std::vector<double>((size_t)n * B, 0.0));
		robot->updateModel();
		robot_controller.reinitializeTasks();       // the goals are the current pose and posture: the stack holds still
		robot_controller.updateControllerTaskModels();
		robot_controller.attachInertia({}, true, {"end-effector"});
		std::vector<double> bodies, payloads;
		example_parts(n, B, bodies, payloads);
		robot_controller.setInertiaParts(bodies, payloads);
		const RobotController::InertiaInfo info = robot_controller.inertiaInfo();
		const std::vector<double> rows = robot_controller.inertiaRows();
		robot_controller.rolloutAsync(K, 5e-4, 2);  // under gravity: the controller compensates its own model's weight, not the simulated robot's
		robot_controller.synchronize();
		robot_controller.pullState();
		int ok = info.per_instance == 1 && info.n_payloads == 1 && info.payload_bodies[0] == n - 1 && rows.size() == (size_t)n * SAIP_INERTIA_ROW_WORDS * B;
		for (double v : robot->q()) ok &= std::isfinite(v);
		for (double v : robot->dq()) ok &= std::isfinite(v);
		const size_t ld = (size_t)(B + 31) / 32 * 32;  // the default leading dimension
		std::vector<double> raw((size_t)n * SAIP_INERTIA_ROW_WORDS * ld);
		if (hipMemcpy(raw.data(), robot_controller.inertiaRowsDevice(), raw.size() * sizeof(double), 2) != 0) return 4;
		std::ofstream o(argv[6], std::ios::binary);
		o.write((const char*)rows.data(), rows.size() * sizeof(double));
		o.write((const char*)raw.data(), raw.size() * sizeof(double));
		o.write((const char*)robot->q().data(), robot->q().size() * sizeof(double));
		o.write((const char*)robot->dq().data(), robot->dq().size() * sizeof(double));
		robot_controller.detachInertia();
		ok &= robot_controller.inertiaRowsDevice() == nullptr;
		std::cout << (ok ? "INERTIA_RUN_OK" : "INERTIA_RUN_FAIL") << std::endl;
		return ok && o ? 0 : 1;
	}
	return 2;
}
