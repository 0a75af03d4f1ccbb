// The plant model through the C++ facade: a Panda with the full motion-force task and a posture task behind it holds its pose while a
// payload hangs on the flange, and on every second instance the actuator of joint 2 saturates.
//   plant_example <robot.txt> cfgonly                        no device: the argument and order errors
//   plant_example <robot.txt> run <B> <K> <q.bin> <out.bin>  K closed-loop periods on GPU 0 from the postures q [dof][B]; prints the plant
//       summaries and writes the resident summary [4][ld] and actuated torques [dof][ld], padding columns included, to out.bin (the one
//       call outside the facade: a device-to-host copy of the HIP runtime the engine links, to show the padding columns)
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

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	const double inf = std::numeric_limits<double>::infinity();
	const std::vector<double> weight = {0.0, 0.0, -2.0 * 9.81, 0.0, 0.0, 0.0, 0.0, inf};  // a 2 kg payload, for ever
	if (std::string(argv[2]) == "cfgonly") {
		auto robot = std::make_shared<SaiModel>(links, 4, -1);
		auto motion_force_task = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
		auto joint_task = std::make_shared<JointTask>(robot);
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		RobotController robot_controller(robot, task_list);
		std::vector<double> joints = robot_controller.neutralPlantJoints();
		int ok = joints.size() == (size_t)7 * SAIP_PLANT_JOINT_WORDS && joints[0] == 1.0 && joints[2] == inf && joints[6] < joints[7];
		auto with = [&](int j, int word, double v) {
			std::vector<double> t = joints;
			t[(size_t)j * SAIP_PLANT_JOINT_WORDS + word] = v;
			return t;
		};
		const RobotController::PlantWrench hang = {"end-effector", {0.0, 0.0, 0.1}, false, weight};
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(std::vector<double>(69, 0.0)); });            // shape
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(joints, {}, true); });                         // [7][10][B] expected
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant({}, {{"end-effector", {0, 0, 0}, false, {1.0, 2.0}}}); });  // 8 values
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant({}, {hang, hang, hang, hang, hang}); });       // five wrenches
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(with(1, 2, -1.0)); });                         // tau_max < 0
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(with(3, 4, 0.5)); });                          // fc > 0 with v_s = 0
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(with(0, 6, 3.5)); });                          // q_lo > q_hi
		ok &= throws<std::invalid_argument>([&] { robot_controller.attachPlant(with(6, 0, std::nan(""))); });                 // NaN
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { robot_controller.attachPlant(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.attachPlant(with(1, 2, 5.0), {hang}); });
		ok &= throws<std::runtime_error>([&] { robot_controller.plantInfo(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.plantSummary(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.resetPlantSummary(); });
		ok &= throws<std::runtime_error>([&] { robot_controller.setPlantPeriod(3); });
		ok &= throws<std::runtime_error>([&] { robot_controller.setPlantJoints(joints); });
		ok &= throws<std::runtime_error>([&] { robot_controller.randomizePlant(1, 0, joints, joints); });
		ok &= throws<std::runtime_error>([&] { robot_controller.detachPlant(); });
		ok &= robot_controller.plantTorquesDevice() == nullptr && robot_controller.plantJointsDevice() == nullptr;
		std::cout << (ok ? "PLANT_CFG_OK" : "PLANT_CFG_FAIL") << std::endl;
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
		// per-instance joints: neutral, but the actuator of joint 2 gives at most 0.1 N m on the even instances
		const std::vector<double> row = robot_controller.neutralPlantJoints();
		std::vector<double> joints((size_t)n * SAIP_PLANT_JOINT_WORDS * B), hang((size_t)SAIP_PLANT_WRENCH_WORDS * B);
		for (size_t w = 0; w < row.size(); w++)
			for (int i = 0; i < B; i++) joints[w * B + i] = row[w];
		for (int i = 0; i < B; i += 2) joints[((size_t)1 * SAIP_PLANT_JOINT_WORDS + 2) * B + i] = 0.1;
		for (int w = 0; w < SAIP_PLANT_WRENCH_WORDS; w++)
			for (int i = 0; i < B; i++) hang[(size_t)w * B + i] = weight[w];
		robot_controller.attachPlant(joints, {{"end-effector", {0.0, 0.0, 0.1}, false, hang}}, true);
		const double no_gravity[3] = {0.0, 0.0, 0.0};  // the arm itself floats: the payload is the only load
		robot_controller.rolloutAsync(K, 5e-4, 2, no_gravity);
		robot_controller.synchronize();
		const RobotController::PlantInfo info = robot_controller.plantInfo();
		std::vector<double> sm = robot_controller.plantSummary();
		robot_controller.pullState();
		int ok = info.period == K && info.n_wrenches == 1 && info.per_instance_joints == 1 && info.per_instance_wrenches == 1;
		for (double v : sm) ok &= std::isfinite(v);
		for (double v : robot->q()) ok &= std::isfinite(v);
		for (double v : robot->dq()) ok &= std::isfinite(v);
		for (double v : robot_controller.getTorques()) ok &= std::isfinite(v);
		for (int r = 0; r < SAIP_PLANT_SUMMARY_ROWS; r++) {
			printf("PLANT_SUMMARY %d", r);
			for (int i = 0; i < B; i++) printf(" %.17g", sm[(size_t)r * B + i]);
			printf("\n");
		}
		const size_t ld = (size_t)(B + 31) / 32 * 32;  // the default leading dimension
		std::vector<double> raw((SAIP_PLANT_SUMMARY_ROWS + (size_t)n) * ld);
		if (hipMemcpy(raw.data(), robot_controller.plantSummaryDevice(), SAIP_PLANT_SUMMARY_ROWS * ld * sizeof(double), 2) != 0) return 4;
		if (hipMemcpy(raw.data() + SAIP_PLANT_SUMMARY_ROWS * ld, robot_controller.plantTorquesDevice(), (size_t)n * ld * sizeof(double), 2) != 0) return 4;
		std::ofstream o(argv[6], std::ios::binary);
		o.write((const char*)raw.data(), raw.size() * sizeof(double));
		robot_controller.detachPlant();
		ok &= robot_controller.plantTorquesDevice() == nullptr;
		std::cout << (ok ? "PLANT_RUN_OK" : "PLANT_RUN_FAIL") << std::endl;
		return ok && o ? 0 : 1;
	}
	return 2;
}
