// Link contact through the C++ facade: link spheres of a Panda against a floor that pushes back, inside rollouts.
//   link_contact_example <robot.txt> cfgonly               no device: the argument and order errors
//   link_contact_example <robot.txt> run <B> <K> <q.bin>   on GPU 0 from the postures q ([dof][B] doubles), at rest; the example checks
//       itself: the readout of an evaluation against a recomputation from the model queries (distance 1e-12 m, the same active count away
//       from d = 0, the net force of a robot at rest = sum k (-d) along the normal); K rollout periods: exactly the instances that
//       start inside the floor have summaries, the others none; the reset of the summaries; the detach
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
		motion_force_task->disableInternalOtg();
		joint_task->disableInternalOtg();
		std::vector<std::shared_ptr<TemplateTask>> task_list = {motion_force_task, joint_task};
		robot_controller = std::make_unique<RobotController>(robot, task_list);
	}
};

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	auto links = read_robot(argv[1]);
	const std::vector<RobotController::ClearanceSphere> spheres = {
		{"link4", {0.0, 0.0, 0.0}, 0.06}, {"link6", {0.0, 0.0, 0.0}, 0.05}, {"end-effector", {0.0, 0.0, 0.03}, 0.04}};
	const double floor_z = 0.35, k = 5.0e3;
	const std::vector<double> obstacles = {1, 0.0, 0.0, 1.0, floor_z, 0, 0, 0};  // the floor z >= floor_z
	const std::vector<double> materials = {k, 40.0, 0.3, 1e-3};
	const int S = 3;
	if (std::string(argv[2]) == "cfgonly") {
		Stack s(links, 4, -1);
		auto& c = *s.robot_controller;
		int ok = 1;
		using Sph = std::vector<RobotController::ClearanceSphere>;
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, {1, 0, 0, 1, 0.05, 0, 0}, materials); });            // shape
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, obstacles, materials, true); });                   // [O][8][B] expected
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, obstacles, {k, 40.0, 0.3}); });                    // [O][4] expected
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(Sph{{"no-such-link", {0, 0, 0}, 0.1}}, obstacles, materials); });
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(Sph{}, obstacles, materials); });                            // 0 spheres
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, {}, {}); });                                        // 0 obstacles
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(Sph{{"link4", {0, 0, 0}, -0.1}}, obstacles, materials); });  // radius below 0
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(Sph{{"link4", {0, NAN, 0}, 0.1}}, obstacles, materials); });
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, {2, 0, 0, 1, 0.05, 0, 0, 0}, materials); });        // unknown kind
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, {1, 0, 0, 1.001, 0.05, 0, 0, 0}, materials); });    // not a unit normal
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, obstacles, {-1.0, 40.0, 0.3, 1e-3}); });            // k below 0
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, obstacles, {k, NAN, 0.3, 1e-3}); });
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(spheres, obstacles, {k, 40.0, 0.3, 0.0}); });                // friction without v_s
		ok &= throws<std::invalid_argument>([&] { c.attachLinkContact(Sph(33, spheres[0]), obstacles, materials); });              // above the maximum
		// valid arguments reach the device check; nothing is attached, so everything else refuses
		ok &= throws<std::runtime_error>([&] { c.attachLinkContact(spheres, obstacles, materials, false, true); });
		ok &= throws<std::runtime_error>([&] { c.attachLinkContact(spheres, obstacles, {k, 0.0, 0.0, 0.0}); });
		ok &= throws<std::runtime_error>([&] { c.detachLinkContact(); });
		ok &= throws<std::runtime_error>([&] { c.linkContactInfo(); });
		ok &= throws<std::runtime_error>([&] { c.setLinkContactObstacles(obstacles); });
		ok &= throws<std::runtime_error>([&] { c.setLinkContactMaterials(materials); });
		ok &= throws<std::runtime_error>([&] { c.evaluateLinkContact(); });
		ok &= throws<std::runtime_error>([&] { c.linkContactReadout(); });
		ok &= throws<std::runtime_error>([&] { c.linkContactSummary(); });
		ok &= throws<std::runtime_error>([&] { c.resetLinkContactSummary(); });
		ok &= throws<std::runtime_error>([&] { c.linkContactCost(1.0); });
		ok &= c.linkContactObstaclesDevice() == nullptr && c.linkContactTorquesDevice() == nullptr && c.linkContactKeepDevice() == nullptr;
		ok &= saip_batch_link_contact_readout_device(c.handle()) == nullptr && saip_batch_link_contact_summary_device(c.handle()) == nullptr;
		std::cout << (ok ? "LINK_CONTACT_CFG_OK" : "LINK_CONTACT_CFG_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	if (std::string(argv[2]) == "run" && argc == 6) {
		const int B = atoi(argv[3]), K = atoi(argv[4]);
		Stack s(links, B, 0);
		auto& c = *s.robot_controller;
		const int n = s.robot->dof();
		std::vector<double> q((size_t)n * B);
		std::ifstream f(argv[5], std::ios::binary);
		f.read((char*)q.data(), q.size() * sizeof(double));
		if (!f) return 3;
		s.robot->setQ(q);
		s.robot->setDq(std::vector<double>((size_t)n * B, 0.0));
		s.robot->updateModel();
		c.reinitializeTasks();
		c.updateControllerTaskModels();
		int ok = 1;
		c.attachLinkContact(spheres, obstacles, materials);
		const RobotController::LinkContactInfo info = c.linkContactInfo();
		ok &= info.n_spheres == S && info.n_obstacles == 1 && !info.per_instance && !info.keep;
		ok &= c.linkContactKeepDevice() == nullptr && c.linkContactObstaclesDevice() != nullptr && c.linkContactTorquesDevice() != nullptr;
		// 1. an evaluation against the model queries (the robot is at rest: f = k (-d) n, no damping, no friction)
		c.evaluateLinkContact();
		const std::vector<double> ro = c.linkContactReadout();
		std::vector<std::vector<double>> centre;  // [S] of [3][B]
		for (const auto& sp : spheres) centre.push_back(s.robot->position(sp.link, sp.centre.data()));
		double worst = 0.0, worst_f = 0.0;
		int inside = 0;
		std::vector<int> starts_inside(B, 0);
		for (int b = 0; b < B; b++) {
			double dmin = 1e300, fz = 0.0;
			int active = 0, near = 0;
			for (int i = 0; i < S; i++) {
				const double d = centre[i][(size_t)2 * B + b] - floor_z - spheres[i].radius;
				dmin = std::fmin(dmin, d);
				near |= std::fabs(d) < 1e-9;
				if (d < 0) {
					active++;
					fz += k * -d;
				}
			}
			worst = std::fmax(worst, std::fabs(ro[(size_t)3 * B + b] - dmin));
			worst_f = std::fmax(worst_f, std::fabs(ro[(size_t)2 * B + b] - fz));
			ok &= ro[b] == 0.0 && ro[(size_t)B + b] == 0.0;  // a frictionless push at rest has no horizontal part
			if (!near) ok &= ro[(size_t)5 * B + b] == (double)active;
			starts_inside[b] = active > 0;
			inside += active > 0;
		}
		ok &= worst <= 1e-12 && worst_f <= 1e-9 * k && inside > 0 && inside < B;
		// 2. K periods: the instances that start inside the floor are pushed, the summaries say so
		const double no_gravity[3] = {0.0, 0.0, 0.0};
		c.rolloutAsync(K, 5e-4, 2, no_gravity);
		const std::vector<double> sm = c.linkContactSummary();
		for (int b = 0; b < B; b++) {
			if (starts_inside[b]) ok &= sm[b] > 0.0 && sm[(size_t)B + b] > 0.0 && sm[(size_t)2 * B + b] > 0.0 && sm[(size_t)3 * B + b] >= 1.0;
			ok &= sm[(size_t)3 * B + b] <= 2.0 * K && sm[b] >= 0.0;
		}
		// 3. the reset, the detach
		c.resetLinkContactSummary();
		const std::vector<double> z = c.linkContactSummary();
		for (size_t i = 0; i < z.size(); i++) ok &= z[i] == 0.0;
		c.detachLinkContact();
		ok &= throws<std::runtime_error>([&] { c.linkContactReadout(); }) && c.linkContactObstaclesDevice() == nullptr;
		printf("worst |dmin - recomputation| %.3e m, worst |F_z - sum k (-d)| %.3e N, %d of %d instances start inside the floor\n", worst, worst_f, inside, B);
		std::cout << (ok ? "LINK_CONTACT_RUN_OK" : "LINK_CONTACT_RUN_FAIL") << std::endl;
		return ok ? 0 : 1;
	}
	return 2;
}
