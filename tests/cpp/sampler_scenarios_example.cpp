// The sampler's scenario groups through the C++ facade, without a device: the facade's own checks of the risk and alpha, and the
// order errors of the four methods on a controller that has no sampler.
//   sampler_scenarios_example <robot.txt> cfgonly
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
	if (argc < 3 || std::string(argv[2]) != "cfgonly") return 2;
	auto links = read_robot(argv[1]);
	const double pos_in_link[3] = {0.0, 0.0, 0.07};
	auto robot = std::make_shared<SaiModel>(links, 6, -1);
	auto mf = std::make_shared<MotionForceTask>(robot, "end-effector", pos_in_link);
	auto jt = std::make_shared<JointTask>(robot);
	std::vector<std::shared_ptr<TemplateTask>> task_list = {mf, jt};
	RobotController c(robot, task_list);
	int ok = 1;
	// the facade's own checks: the risk by name, alpha with "cvar" and with nothing else
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "median"); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "cvar"); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "cvar", 1.5); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "cvar", -0.1); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "max", 0.5); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(2, "mean", 0.5); });
	// the ABI's argument errors come through as std::invalid_argument ...
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(0); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(SAIP_SAMPLER_MAX_SCENARIOS + 1); });
	ok &= throws<std::invalid_argument>([&] { c.setSamplerScenarios(4); });  // 6 instances are no multiple of 4
	// ... and without a sampler every method is an order error
	ok &= throws<std::runtime_error>([&] { c.setSamplerScenarios(2); });
	ok &= throws<std::runtime_error>([&] { c.setSamplerScenarios(3, "cvar", 0.5); });
	ok &= throws<std::runtime_error>([&] { c.samplerScenarios(); });
	ok &= throws<std::runtime_error>([&] { c.samplerGroupCost(); });
	ok &= throws<std::runtime_error>([&] { c.shareScenarioTables(); });
	ok &= saip_batch_sampler_group_cost_device(c.handle()) == nullptr;
	std::cout << (ok ? "SCENARIOS_CFG_OK" : "SCENARIOS_CFG_FAIL") << std::endl;
	return ok ? 0 : 1;
}
