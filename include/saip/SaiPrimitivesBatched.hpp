// SaiPrimitivesBatched.hpp -- header-only C++17 facade over the C-ABI (include/saip.h) that keeps the reference's
// class and method names for the control-cycle path, in a batched flavour: one object = B robot instances.
//
//   reference (one robot, Eigen)                                   this facade (B robots, SoA std::vector<double>)
//   SaiModel::SaiModel robot(urdf)                                  SaiPrimitivesBatched::SaiModel robot(links, B, device)
//   robot->setQ(q); robot->setDq(dq); robot->updateModel();         robot->setQ(q); robot->setDq(dq); robot->updateModel();   q: [dof][B]
//   MotionForceTask(robot, link, compliant_frame)                   MotionForceTask(robot, link, pos_in_link)
//   JointTask(robot) / JointTask(robot, S)                          JointTask(robot) / JointTask(robot, S, rows)
//   RobotController(robot, tasks)                                   RobotController(robot, tasks)
//   controller->updateControllerTaskModels();                       controller->updateControllerTaskModels();
//   task->setGoalPosition(x) ...                                    task->setGoalPosition(x) ...                               x: [3][B]
//   tau = controller->computeControlTorques();                      tau = controller->computeControlTorques();                  tau: [dof][B]
//   task->updateTaskModel(N_prec); task->computeTorques()           the same (TemplateTask.h:43-60; examples/04-task_and_redundancy):      N_prec: [dof*dof][B]
//   N_prec = task->getTaskAndPreviousNullspace()                    a task driven by hand without a RobotController owns a private one-task batch
//
// Reference interface: /root/reference/src/RobotController.h:47-90, src/tasks/TemplateTask.h:26-124,
// src/tasks/MotionForceTask.h:96-110,211-300,423,670-736, src/tasks/JointTask.h:56-75,140-175,237-257,323,363.
// Errors: std::invalid_argument where the reference throws it; std::runtime_error for device / unsupported / order errors.
// Every array is struct-of-arrays, component-major: value of component c for instance b at [c * B + b].
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <array>
#include <string>
#include <vector>

#include "../saip.h"

namespace SaiPrimitivesBatched {

enum TaskType { UNDEFINED = 0, JOINT_LIMIT_AVOIDANCE_TASK = 1, JOINT_TASK = 2, MOTION_FORCE_TASK = 3 };  // TemplateTask.h:19-24
enum DynamicDecouplingType { FULL_DYNAMIC_DECOUPLING = 0, BOUNDED_INERTIA_ESTIMATES = 1, IMPEDANCE = 2 };  // SaiPrimitivesCommonDefinitions.h:14-20
struct PIDGains {  // SaiPrimitivesCommonDefinitions.h:26-32
	double kp, kv, ki;
	PIDGains(double kp_, double kv_, double ki_) : kp(kp_), kv(kv_), ki(ki_) {}
};

inline void check(saip_status st) {
	if (st == SAIP_OK) return;
	const std::string msg = saip_last_error();
	if (st == SAIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(msg);
	throw std::runtime_error("[saip status " + std::to_string((int)st) + "] " + msg);
}

class RobotController;
class TemplateTask;

// a [dof*dof][ld] nullspace matrix resident on the GPU: what getTaskAndPreviousNullspaceDevice() returns and updateTaskModel accepts
struct DeviceNullspace {
	saip_batch* batch = nullptr;
	const double* ptr = nullptr;
};

// B instances of one robot: constants + host-side q/dq staging (the kinematics/dynamics run inside the GPU cycle)
class SaiModel {
public:
	SaiModel(const std::vector<saip_link_desc>& links, int batch_size, int device = 0) : _batch(batch_size), _device(device) {
		check(saip_model_create_serial_chain(links.data(), (int)links.size(), &_model));
		_q.assign((size_t)dof() * _batch, 0.0);
		_dq.assign((size_t)dof() * _batch, 0.0);
	}
	// kinematic tree: parent[l] = index of link l's parent in `links`, -1 for the fixed base (saip_model_create_tree)
	SaiModel(const std::vector<saip_link_desc>& links, const std::vector<int>& parent, int batch_size, int device = 0)
		: _batch(batch_size), _device(device) {
		if (parent.size() != links.size()) throw std::invalid_argument("SaiModel: one parent index per link expected");
		check(saip_model_create_tree(links.data(), parent.data(), (int)links.size(), &_model));
		_q.assign((size_t)dof() * _batch, 0.0);
		_dq.assign((size_t)dof() * _batch, 0.0);
	}
	~SaiModel() {
		if (_mq) saip_batch_destroy(_mq);  // the query batch refers to the model: it goes first
		saip_model_destroy(_model);
	}
	SaiModel(const SaiModel&) = delete;
	SaiModel& operator=(const SaiModel&) = delete;

	int dof() const { return saip_model_dof(_model); }
	int batchSize() const { return _batch; }
	int device() const { return _device; }
	const std::vector<double>& q() const { return _q; }
	const std::vector<double>& dq() const { return _dq; }
	void setQ(const std::vector<double>& q) {
		if (q.size() != _q.size()) throw std::invalid_argument("setQ: expected dof*batch values");
		_q = q;
		_version++;
	}
	void setDq(const std::vector<double>& dq) {
		if (dq.size() != _dq.size()) throw std::invalid_argument("setDq: expected dof*batch values");
		_dq = dq;
		_version++;
	}
	// pushes the state to every batch that mirrors this robot (the RobotController's and the private batches of tasks driven by hand)
	void updateModel() {
		for (auto& a : _attached) push(a);
		_mq_q = _q;
		_mq_dq = _dq;
		_mq_version++;
		if (_mq) pushQueryState();
	}
	const saip_model* handle() const { return _model; }
	// movable parent body of joint `joint` (-1: the fixed base)
	int jointParent(int joint) const {
		const int p = saip_model_joint_parent(_model, joint);
		if (p == -2) throw std::invalid_argument("jointParent: joint index out of range");
		return p;
	}
	int linkIndex(const std::string& link) const {
		const int i = saip_model_link_index(_model, link.c_str());
		if (i < 0) throw std::invalid_argument("link " + link + " does not exist in the robot model");
		return i;
	}

	// ---- model queries: the sai-model accessors at the state of the last updateModel() (saip_batch_model_frames_host /
	// saip_batch_model_dynamics_host on a model-only batch of this robot, created at the first query).  Results in the [c*B + b] layout.
	std::vector<double> position(const std::string& link, const double* pos_in_link = nullptr) { return frameRows(link, pos_in_link, 0, 0, 3); }
	std::vector<double> rotation(const std::string& link) { return frameRows(link, nullptr, 0, 3, 9); }
	std::vector<double> transform(const std::string& link, const double* pos_in_link = nullptr) { return toTransform(frameRows(link, pos_in_link, 0, 0, 12)); }
	std::vector<double> linearVelocity(const std::string& link, const double* pos_in_link = nullptr) { return frameRows(link, pos_in_link, 0, 12, 3); }
	std::vector<double> angularVelocity(const std::string& link) { return frameRows(link, nullptr, 0, 15, 3); }
	std::vector<double> J(const std::string& link, const double* pos_in_link = nullptr) { return frameRows(link, pos_in_link, SAIP_QUERY_JACOBIAN, 18, 6 * dof()); }
	std::vector<double> Jv(const std::string& link, const double* pos_in_link = nullptr) { return frameRows(link, pos_in_link, SAIP_QUERY_JACOBIAN, 18, 3 * dof()); }
	std::vector<double> Jw(const std::string& link) { return frameRows(link, nullptr, SAIP_QUERY_JACOBIAN, 18 + 3 * dof(), 3 * dof()); }
	std::vector<double> positionInWorld(const std::string& link, const double* pos_in_link = nullptr) { return frameRows(link, pos_in_link, SAIP_QUERY_WORLD, 0, 3); }
	std::vector<double> rotationInWorld(const std::string& link) { return frameRows(link, nullptr, SAIP_QUERY_WORLD, 3, 9); }
	std::vector<double> transformInWorld(const std::string& link, const double* pos_in_link = nullptr) {
		return toTransform(frameRows(link, pos_in_link, SAIP_QUERY_WORLD, 0, 12));
	}
	std::vector<double> linearVelocityInWorld(const std::string& link, const double* pos_in_link = nullptr) {
		return frameRows(link, pos_in_link, SAIP_QUERY_WORLD, 12, 3);
	}
	std::vector<double> angularVelocityInWorld(const std::string& link) { return frameRows(link, nullptr, SAIP_QUERY_WORLD, 15, 3); }
	std::vector<double> JWorldFrame(const std::string& link, const double* pos_in_link = nullptr) {
		return frameRows(link, pos_in_link, SAIP_QUERY_JACOBIAN | SAIP_QUERY_WORLD, 18, 6 * dof());
	}
	// SaiModel::setTRobotBase: T_world_robot (R row-major, p), the same for every instance; reaches every batch of this robot.  Only the
	// *InWorld queries use it: gravity and the torques stay in the robot base frame (saip.h)
	void setTRobotBase(const double R[9], const double p[3]) {
		for (auto& a : _attached) check(saip_batch_set_robot_base(a.batch, R, p));
		if (_mq) check(saip_batch_set_robot_base(_mq, R, p));
		std::copy(R, R + 9, _Rb);
		std::copy(p, p + 3, _pb);
	}
	void TRobotBase(double R[9], double p[3]) const {
		std::copy(_Rb, _Rb + 9, R);
		std::copy(_pb, _pb + 3, p);
	}
	std::vector<double> M() { return dynamics(0); }
	std::vector<double> MInv() { return dynamics(1); }
	std::vector<double> jointGravityVector() { return dynamics(2); }
	std::vector<double> coriolisForce() { return dynamics(3); }

private:
	friend class RobotController;
	friend class TemplateTask;
	struct Attached {
		saip_batch* batch;
		long pushed;
	};
	void attach(saip_batch* b) {
		_attached.push_back({b, -1});
		check(saip_batch_set_robot_base(b, _Rb, _pb));
	}
	saip_batch* queryBatch() {
		if (!_mq) {
			saip_batch* b = nullptr;
			check(saip_batch_create(_model, _batch, _device, &b));
			saip_status st = saip_batch_finalize_model_only(b);
			if (st == SAIP_OK) st = saip_batch_set_robot_base(b, _Rb, _pb);
			if (st != SAIP_OK) {
				saip_batch_destroy(b);
				check(st);
			}
			_mq = b;
		}
		pushQueryState();
		return _mq;
	}
	void pushQueryState() {
		if (_device < 0 || _mq_pushed == _mq_version) return;
		if (_mq_q.empty()) {
			_mq_q.assign(_q.size(), 0.0);
			_mq_dq.assign(_dq.size(), 0.0);
		}
		check(saip_batch_set_state_host(_mq, _mq_q.data(), _mq_dq.data()));
		_mq_pushed = _mq_version;
	}
	// rows [first, first + count) of one frame
	std::vector<double> frameRows(const std::string& link, const double* pos_in_link, int flags, int first, int count) {
		saip_batch* b = queryBatch();
		const int li = linkIndex(link);
		const int rows = saip_batch_model_frame_rows(b, flags);
		std::vector<double> out((size_t)rows * _batch);
		check(saip_batch_model_frames_host(b, 1, &li, pos_in_link, flags, out.data()));
		return std::vector<double>(out.begin() + (size_t)first * _batch, out.begin() + (size_t)(first + count) * _batch);
	}
	// rows 0..11 (position, rotation) -> [16][B] row-major 4 x 4
	std::vector<double> toTransform(const std::vector<double>& r) const {
		std::vector<double> T((size_t)16 * _batch, 0.0);
		for (int b = 0; b < _batch; b++) {
			for (int i = 0; i < 3; i++) {
				for (int j = 0; j < 3; j++) T[(size_t)(4 * i + j) * _batch + b] = r[(size_t)(3 + 3 * i + j) * _batch + b];
				T[(size_t)(4 * i + 3) * _batch + b] = r[(size_t)i * _batch + b];
			}
			T[(size_t)15 * _batch + b] = 1.0;
		}
		return T;
	}
	// 0 M, 1 M^-1, 2 g, 3 b
	std::vector<double> dynamics(int which) {
		saip_batch* b = queryBatch();
		const size_t n = dof();
		std::vector<double> out((which < 2 ? n * n : n) * _batch);
		double* p[4] = {nullptr, nullptr, nullptr, nullptr};
		p[which] = out.data();
		check(saip_batch_model_dynamics_host(b, p[0], p[1], p[2], p[3]));
		return out;
	}
	void detach(saip_batch* b) {
		for (size_t i = 0; i < _attached.size(); i++)
			if (_attached[i].batch == b) {
				_attached.erase(_attached.begin() + i);
				return;
			}
	}
	void push(Attached& a) {
		if (a.pushed != _version) {
			check(saip_batch_set_state_host(a.batch, _q.data(), _dq.data()));
			a.pushed = _version;
		}
	}
	void pushTo(saip_batch* b) {
		for (auto& a : _attached)
			if (a.batch == b) push(a);
	}
	saip_model* _model = nullptr;
	int _batch, _device;
	std::vector<double> _q, _dq;
	long _version = 0;
	std::vector<Attached> _attached;
	saip_batch* _mq = nullptr;  // model-only batch of the queries
	std::vector<double> _mq_q, _mq_dq;  // the state of the last updateModel()
	long _mq_version = 0, _mq_pushed = -1;
	double _Rb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, _pb[3] = {0, 0, 0};
};

// TemplateTask.h:26-124
class TemplateTask {
public:
	TemplateTask(std::shared_ptr<SaiModel>& robot, const std::string& task_name, TaskType type, double loop_timestep)
		: _robot(robot), _task_name(task_name), _task_type(type), _loop_timestep(loop_timestep) {}
	virtual ~TemplateTask() { dropPrivateBatch(); }
	TemplateTask(const TemplateTask&) = delete;
	TemplateTask& operator=(const TemplateTask&) = delete;
	const std::shared_ptr<SaiModel>& getConstRobotModel() const { return _robot; }
	const double& getLoopTimestep() const { return _loop_timestep; }
	const TaskType& getTaskType() const { return _task_type; }
	const std::string& getTaskName() const { return _task_name; }

	void setDynamicDecouplingType(DynamicDecouplingType t) { cfg([=](saip_batch* b, int id) { return saip_batch_set_dynamic_decoupling_type(b, id, (int)t); }); }
	void setBoundedInertiaEstimateThreshold(double thr) {
		_bie_threshold = thr;
		cfg([=](saip_batch* b, int id) { return saip_batch_set_bie_threshold(b, id, thr); });
	}
	double getBoundedInertiaEstimateThreshold() const { return _bie_threshold; }
	// ---- the reference's per-task interface, TemplateTask.h:43-60, driven by hand in examples/04-task_and_redundancy/04-task_and_redundancy.cpp:141-206
	// N_prec: [dof*dof][B] (row-major per instance) or dof*dof values shared by every instance
	void updateTaskModel(const std::vector<double>& N_prec) {
		need();
		const size_t n = _robot->dof(), B = _robot->batchSize();
		if (N_prec.size() == n * n) {
			std::vector<double> all(n * n * B);
			for (size_t e = 0; e < n * n; e++)
				for (size_t b = 0; b < B; b++) all[e * B + b] = N_prec[e];
			pushAndUpdate(all.data());
		} else if (N_prec.size() == n * n * B) {
			pushAndUpdate(N_prec.data());
		} else {
			throw std::invalid_argument("N_prec matrix size not consistent with robot dof in updateTaskModel\n");  // JointTask.cpp:224-229
		}
	}
	// N_prec stays on the GPU: the handle another task's getTaskAndPreviousNullspaceDevice() returned
	void updateTaskModel(const DeviceNullspace& N_prec) {
		need();
		_robot->pushTo(_batch);
		if (N_prec.batch && N_prec.batch != _batch) check(saip_batch_wait_for(_batch, N_prec.batch));
		check(saip_batch_task_update_model_device(_batch, _id, N_prec.ptr));
		_manual = true;
	}
	// [dof][B] torques of THIS task (no RobotController post-processing); per-instance status in status()
	std::vector<double> computeTorques() { return torques(nullptr); }
	// ... with the feed-forward compensation of the torques of the previous tasks (JointTask.cpp:285-292)
	std::vector<double> computeTorques(const std::vector<double>& tau_prec) {
		if (tau_prec.size() != (size_t)_robot->dof() * _robot->batchSize()) throw std::invalid_argument("tau_prec: expected [dof][B]");
		return torques(tau_prec.data());
	}
	const std::vector<uint8_t>& status() const { return _status; }
	DeviceNullspace getTaskAndPreviousNullspaceDevice() {
		if (!_manual) throw std::runtime_error("getTaskAndPreviousNullspaceDevice: call updateTaskModel first");
		return DeviceNullspace{_batch, saip_batch_task_device_nullspace(_batch, _id, 2)};
	}
	// TemplateTask::reInitializeTask of this task alone
	void reInitializeTask() {
		need();
		_robot->pushTo(_batch);
		check(saip_batch_reinitialize_task(_batch, _id));
	}
	// resetIntegrators (both tasks), resetIntegratorsLinear / Angular (MotionForceTask.cpp:988-1002)
	void resetIntegrators() {
		need();
		check(saip_batch_reset_integrators(_batch, _id, 3));
	}
	void disableInternalOtg() {
		_otg_enabled = false;
		cfg([](saip_batch* b, int id) { return saip_batch_set_internal_otg(b, id, 0); });
	}
	bool getInternalOtgEnabled() const { return _otg_enabled; }
	// [goal_components][B]: what the control law tracks -- the internal OTG's output when enabled, else the goal (getDesired*)
	std::vector<double> getDesiredState() {
		need();
		std::vector<double> d((size_t)saip_batch_goal_components(_batch, _id) * _robot->batchSize());
		check(saip_batch_get_desired_host(_batch, _id, d.data()));
		return d;
	}
	// OTG::isGoalReached per instance
	std::vector<bool> isInternalOtgGoalReached() {
		need();
		std::vector<int> fl(_robot->batchSize());
		check(saip_batch_get_otg_status_host(_batch, _id, fl.data(), nullptr));
		std::vector<bool> r(fl.size());
		for (size_t i = 0; i < fl.size(); i++) r[i] = (fl[i] & 1) != 0;
		return r;
	}
	void disableVelocitySaturation() { cfg([](saip_batch* b, int id) { return saip_batch_set_velocity_saturation(b, id, 0); }); }
	// ---- goal schedules: time-varying goals inside RobotController::rolloutAsync from keyframes resident on the device (saip.h).
	// Goal components [first, first + count) of this task; keyframes [n_keyframes][count] (the same for every instance) or
	// [n_keyframes][count][B] (per instance); mode SAIP_SCHEDULE_HOLD or SAIP_SCHEDULE_LINEAR
	void setGoalSchedule(int first, int count, const std::vector<double>& keyframes, int n_keyframes, int stride = 1, int mode = SAIP_SCHEDULE_HOLD) {
		need();
		const size_t per_frame = (size_t)(count > 0 ? count : 0), B = _robot->batchSize();
		const size_t K = (size_t)(n_keyframes > 0 ? n_keyframes : 0);
		if (K == 0 || per_frame == 0 || (keyframes.size() != K * per_frame && keyframes.size() != K * per_frame * B))
			throw std::invalid_argument("setGoalSchedule: expected [n_keyframes][count] or [n_keyframes][count][B] keyframes");
		const int per_instance = keyframes.size() == K * per_frame ? 0 : 1;  // (B == 1: the two layouts coincide)
		check(saip_batch_goal_schedule_attach(_batch, _id, first, count, keyframes.data(), n_keyframes, stride, mode, per_instance));
	}
	// field: the name of a goal setter's field ("position", "orientation", "linear_velocity", ... / joint task: "position", "velocity",
	// "acceleration")
	void setGoalSchedule(const std::string& field, const std::vector<double>& keyframes, int n_keyframes, int stride = 1, int mode = SAIP_SCHEDULE_HOLD) {
		int first = 0, count = 0;
		if (!scheduleField(field, &first, &count)) throw std::invalid_argument("setGoalSchedule: task [" + _task_name + "] has no goal field " + field);
		setGoalSchedule(first, count, keyframes, n_keyframes, stride, mode);
	}
	// detach this task's schedule; its goal keeps the values applied last
	void clearGoalSchedule() {
		need();
		check(saip_batch_goal_schedule_detach(_batch, _id));
	}
	// the resident keyframes ([n_keyframes][count][ld] per instance, else [n_keyframes][count]), to be rewritten in place; nullptr without a schedule
	double* goalScheduleDevice() {
		need();
		return saip_batch_goal_schedule_device(_batch, _id);
	}
	// ---- resident rollout sampler on this task's per-instance goal schedule (saip.h): sigma [d] over the scheduled rows in order, an
	// orientation (rows 3..11 of a motion-force task) counting as three tangent coordinates; nominal [n_keyframes][count], empty =
	// instance 0's keyframes; instances 0 .. exempt - 1 always run the nominal plan
	void contactMine(int* n_planes = nullptr, int* per_instance = nullptr) {  // the controller's contact planes are attached to THIS task
		need();
		int task = -1;
		check(saip_batch_contact_info(_batch, &task, n_planes, per_instance, nullptr, nullptr));
		if (task != _id) throw std::runtime_error("the contact planes of this controller are attached to another task");
	}
	int contactTarget(int* per_instance = nullptr) {  // whichever of contact planes or contact patch THIS task has, as an environment-schedule target
		need();
		int task = -1, per = 0;
		if (saip_batch_contact_info(_batch, &task, nullptr, &per, nullptr, nullptr) == SAIP_OK && task == _id) {
			if (per_instance) *per_instance = per;
			return SAIP_ENV_TARGET_PLANES;
		}
		if (saip_batch_contact_patch_info(_batch, _id, nullptr, nullptr, nullptr, &per, nullptr, nullptr) == SAIP_OK) {
			if (per_instance) *per_instance = per;
			return SAIP_ENV_TARGET_PATCH;
		}
		throw std::runtime_error("this task has neither contact planes nor a contact patch");
	}
	void attachSampler(const std::vector<double>& sigma, const std::vector<double>& nominal = {}, int exempt = 1) {
		need();
		int first = 0, count = 0, nk = 0;
		check(saip_batch_goal_schedule_info(_batch, _id, &first, &count, &nk, nullptr, nullptr, nullptr));
		int f0 = 0, c0 = 0;
		const bool rot = scheduleField("orientation", &f0, &c0) && first <= 3 && first + count >= 12;
		if ((int)sigma.size() != (rot ? count - 6 : count)) throw std::invalid_argument("attachSampler: one sigma per sampler coordinate expected");
		if (!nominal.empty() && nominal.size() != (size_t)nk * count) throw std::invalid_argument("attachSampler: expected a [n_keyframes][count] nominal plan");
		check(saip_batch_sampler_attach(_batch, _id, sigma.data(), nominal.empty() ? nullptr : nominal.data(), exempt));
	}
	void detachSampler() {
		need();
		check(saip_batch_sampler_detach(_batch, _id));
	}
	// ---- contact planes and the simulated force sensor of the resident simulator (saip.h): one contact point (`point`, in this task's control
	// frame) on this task's body against 1..4 world-fixed half-spaces.  planes: [P][8] rows { n[3], offset, k, c, mu, v_s }, or [P][8][B] with
	// per_instance.  A motion-force task only (the engine refuses any other).
	void attachContactPlanes(const std::vector<double>& planes, int n_planes, const std::array<double, 3>& point = {0.0, 0.0, 0.0}, bool sensor = true,
							 bool per_instance = false) {
		need();
		const size_t cols = per_instance ? (size_t)saip_batch_size(_batch) : 1;
		if (n_planes < 1 || planes.size() != (size_t)n_planes * SAIP_CONTACT_PLANE_WORDS * cols)
			throw std::invalid_argument("attachContactPlanes: expected [n_planes][8] planes, or [n_planes][8][B] per instance");
		check(saip_batch_contact_attach(_batch, _id, point.data(), n_planes, planes.data(), per_instance ? 1 : 0, sensor ? 1 : 0));
	}
	void detachContactPlanes() {
		contactMine();
		check(saip_batch_contact_detach(_batch));
	}
	void setContactPlanes(const std::vector<double>& planes) {
		int np = 0, per = 0;
		contactMine(&np, &per);
		if (planes.size() != (size_t)np * SAIP_CONTACT_PLANE_WORDS * (per ? (size_t)saip_batch_size(_batch) : 1))
			throw std::invalid_argument("setContactPlanes: the shape of the attached plane table expected");
		check(saip_batch_contact_set_planes_host(_batch, planes.data()));
	}
	double* contactPlanesDevice() {
		need();
		return saip_batch_contact_planes_device(_batch);
	}
	// [8][B]: force on the robot (world) 3, point 3, smallest signed distance, active planes -- of the last contact launch; waits for the stream
	std::vector<double> contactReadout() {
		contactMine();
		std::vector<double> out((size_t)SAIP_CONTACT_READOUT_ROWS * saip_batch_size(_batch));
		check(saip_batch_contact_readout_host(_batch, out.data()));
		return out;
	}
	// [4][B]: sum dt * normal force, max |f|, max penetration, substeps in contact; waits for the stream
	std::vector<double> contactSummary() {
		contactMine();
		std::vector<double> out((size_t)SAIP_CONTACT_SUMMARY_ROWS * saip_batch_size(_batch));
		check(saip_batch_contact_summary_host(_batch, out.data()));
		return out;
	}
	void resetContactSummary() {
		contactMine();
		check(saip_batch_contact_summary_reset(_batch));
	}
	// ---- guards (saip.h): event-triggered phases of the rollout periods on this task's goal.  A guard moves an instance from one phase to
	// another on what the instance senses; a phase leaves the goal alone (FREE), holds the pose latched at the transition into it (HOLD) or
	// that pose moved by an offset in the world frame (OFFSET).  Phase 0 must be FREE.  A motion-force task only.
	struct Guard {
		int from = 0, to = 0, signal = SAIP_GUARD_PERIODS, axis = 0, cmp = SAIP_GUARD_GE;
		double threshold = 0.0;
		int hold = 1, blank = 0;
	};
	struct GuardPhase {
		int mode = SAIP_GUARD_FREE;
		std::array<double, 3> offset = {0.0, 0.0, 0.0};
	};
	void attachGuards(const std::vector<Guard>& guards, const std::vector<GuardPhase>& phases) {
		need();
		std::vector<double> g, p;
		for (const auto& x : guards) g.insert(g.end(), {(double)x.from, (double)x.to, (double)x.signal, (double)x.axis, (double)x.cmp, x.threshold, (double)x.hold, (double)x.blank});
		for (const auto& x : phases) p.insert(p.end(), {(double)x.mode, x.offset[0], x.offset[1], x.offset[2]});
		check(saip_batch_guard_attach(_batch, _id, (int)guards.size(), g.empty() ? nullptr : g.data(), 0, (int)phases.size(), p.empty() ? nullptr : p.data()));
	}
	// the raw tables: guards [G][8], or [G][8][B] with per_instance; phases [P][4]
	void attachGuards(const std::vector<double>& guards, int n_guards, const std::vector<double>& phases, int n_phases, bool per_instance = false) {
		need();
		const size_t cols = per_instance ? (size_t)saip_batch_size(_batch) : 1;
		if (n_guards < 1 || guards.size() != (size_t)n_guards * SAIP_GUARD_WORDS * cols || n_phases < 1 || phases.size() != (size_t)n_phases * SAIP_GUARD_PHASE_WORDS)
			throw std::invalid_argument("attachGuards: expected [n_guards][8] guards, or [n_guards][8][B] per instance, and [n_phases][4] phases");
		check(saip_batch_guard_attach(_batch, _id, n_guards, guards.data(), per_instance ? 1 : 0, n_phases, phases.data()));
	}
	void detachGuards() {
		need();
		int task = -1;
		check(saip_batch_guard_info(_batch, &task, nullptr, nullptr, nullptr, nullptr));
		if (task != _id) throw std::runtime_error("the guards of this controller are attached to another task");
		check(saip_batch_guard_detach(_batch));
	}
	// ---- contact patches (saip.h): 1..8 contact points (`points`, [n][3], in this task's control frame) on this task's body against the
	// patch's own planes (format of attachContactPlanes), the net force and moment fed to the integrator and to the simulated sensor.  Up
	// to two patches per controller, on different motion-force tasks; never together with attachContactPlanes.
	void attachContactPatch(const std::vector<double>& points, const std::vector<double>& planes, int n_planes, bool sensor = true, bool per_instance = false) {
		need();
		const size_t cols = per_instance ? (size_t)saip_batch_size(_batch) : 1;
		if (points.empty() || points.size() % 3 != 0) throw std::invalid_argument("attachContactPatch: expected [n][3] points");
		if (n_planes < 1 || planes.size() != (size_t)n_planes * SAIP_CONTACT_PLANE_WORDS * cols)
			throw std::invalid_argument("attachContactPatch: expected [n_planes][8] planes, or [n_planes][8][B] per instance");
		check(saip_batch_contact_patch_attach(_batch, _id, (int)(points.size() / 3), points.data(), n_planes, planes.data(), per_instance ? 1 : 0, sensor ? 1 : 0));
	}
	void detachContactPatch() {
		need();
		check(saip_batch_contact_patch_detach(_batch, _id));
	}
	void setContactPatchPlanes(const std::vector<double>& planes) {
		need();
		int np = 0, per = 0;
		check(saip_batch_contact_patch_info(_batch, _id, nullptr, nullptr, &np, &per, nullptr, nullptr));
		if (planes.size() != (size_t)np * SAIP_CONTACT_PLANE_WORDS * (per ? (size_t)saip_batch_size(_batch) : 1))
			throw std::invalid_argument("setContactPatchPlanes: the shape of the attached plane table expected");
		check(saip_batch_contact_patch_set_planes_host(_batch, _id, planes.data()));
	}
	int contactPatchPoints() {  // the number of points of this task's patch
		need();
		int n = 0;
		check(saip_batch_contact_patch_info(_batch, _id, nullptr, &n, nullptr, nullptr, nullptr, nullptr));
		return n;
	}
	double* contactPatchPlanesDevice() {
		need();
		return saip_batch_contact_patch_planes_device(_batch, _id);
	}
	double* contactPatchReadoutDevice() {
		need();
		return saip_batch_contact_patch_readout_device(_batch, _id);
	}
	double* contactPatchSummaryDevice() {
		need();
		return saip_batch_contact_patch_summary_device(_batch, _id);
	}
	double* contactPatchTorquesDevice() {
		need();
		return saip_batch_contact_patch_torques_device(_batch);
	}
	// [20][B]: net force on the robot (world) 3, net moment about the control point 3, smallest signed distance, points touching, index of the
	// deepest point, control point 3, normal-force sum of each of the eight point slots -- of the last launch; waits for the stream
	std::vector<double> contactPatchReadout() {
		need();
		std::vector<double> out((size_t)SAIP_CONTACT_PATCH_READOUT_ROWS * saip_batch_size(_batch));
		check(saip_batch_contact_patch_readout_host(_batch, _id, out.data()));
		return out;
	}
	// [6][B]: sum dt * normal force, max |F|, max penetration, substeps in contact, max |M|, substeps in full contact; waits for the stream
	std::vector<double> contactPatchSummary() {
		need();
		std::vector<double> out((size_t)SAIP_CONTACT_PATCH_SUMMARY_ROWS * saip_batch_size(_batch));
		check(saip_batch_contact_patch_summary_host(_batch, _id, out.data()));
		return out;
	}
	void resetContactPatchSummary() {  // pairs with a snapshot restore: the summaries are not part of a snapshot
		need();
		check(saip_batch_contact_patch_summary_reset(_batch, _id));
	}
	// ---- environment schedule of this task's contact surfaces (saip.h): the planes of its contact planes or of its contact patch, whichever
	// it has, move during rollouts.  keyframes: [K][n][12] rows { n[3], offset, k, c, mu, v_s, u[3], 0 } (u: the velocity of the surface in the
	// base frame), or [K][n][12][B] when the planes are per instance; the schedule covers planes first .. first + n - 1.
	struct EnvScheduleInfo {
		int first = 0, n_items = 0, n_keyframes = 0, stride = 1, mode = 0, per_instance = 0;
		long long period = 0;
	};
	void setContactSchedule(const std::vector<double>& keyframes, int n_keyframes, int stride = 1, int mode = SAIP_ENV_HOLD, int first = 0) {
		int per = 0;
		const int target = contactTarget(&per);
		const size_t frame = (size_t)SAIP_ENV_PLANE_WORDS * (per ? (size_t)saip_batch_size(_batch) : 1);
		if (n_keyframes < 1 || keyframes.empty() || keyframes.size() % ((size_t)n_keyframes * frame) != 0)
			throw std::invalid_argument("setContactSchedule: expected [K][n][12] keyframes, or [K][n][12][B] when the planes are per instance");
		check(saip_batch_env_schedule_attach(_batch, target, _id, first, (int)(keyframes.size() / ((size_t)n_keyframes * frame)), keyframes.data(), n_keyframes, stride, mode));
	}
	void clearContactSchedule() { check(saip_batch_env_schedule_detach(_batch, contactTarget(), _id)); }
	EnvScheduleInfo contactScheduleInfo() {
		EnvScheduleInfo i;
		check(saip_batch_env_schedule_info(_batch, contactTarget(), _id, &i.first, &i.n_items, &i.n_keyframes, &i.stride, &i.mode, &i.per_instance, &i.period));
		return i;
	}
	double* contactVelocityDevice() { return saip_batch_env_schedule_velocity_device(_batch, contactTarget(), _id); }  // [P][4] or [P][4][ld]; nullptr without a schedule
	std::vector<double> samplerNominal() {
		need();
		check(saip_batch_sampler_info(_batch, _id, nullptr, nullptr, nullptr, nullptr));
		int count = 0, nk = 0;
		check(saip_batch_goal_schedule_info(_batch, _id, nullptr, &count, &nk, nullptr, nullptr, nullptr));
		std::vector<double> out((size_t)nk * count);
		check(saip_batch_sampler_get_nominal_host(_batch, _id, out.data()));
		return out;
	}
	void setSamplerNominal(const std::vector<double>& nominal) {
		need();
		check(saip_batch_sampler_info(_batch, _id, nullptr, nullptr, nullptr, nullptr));
		int count = 0, nk = 0;
		check(saip_batch_goal_schedule_info(_batch, _id, nullptr, &count, &nk, nullptr, nullptr, nullptr));
		if (nominal.size() != (size_t)nk * count) throw std::invalid_argument("setSamplerNominal: expected a [n_keyframes][count] nominal plan");
		check(saip_batch_sampler_set_nominal_host(_batch, _id, nominal.data()));
	}
	// (B x dof x dof as [dof*dof][B]) nullspace projector of this task for the current state, TemplateTask.h:71-77
	std::vector<double> getTaskNullspace() {
		need();
		const int n = _robot->dof();
		std::vector<double> N((size_t)n * n * _robot->batchSize());
		if (_manual) check(saip_batch_task_get_nullspaces_host(_batch, _id, N.data(), nullptr, nullptr));
		else check(saip_batch_get_task_nullspace_host(_batch, _id, N.data()));
		return N;
	}
	// N_prec this task was updated with = N_{t-1} ... N_0 of the tasks above it (identity for the first), TemplateTask.h:79-83; same layout
	std::vector<double> getPreviousTasksNullspace() {
		need();
		const int n = _robot->dof();
		const size_t B = _robot->batchSize();
		std::vector<double> Np((size_t)n * n * B, 0.0), Ns(Np.size()), T(Np.size());
		if (_manual) {
			check(saip_batch_task_get_nullspaces_host(_batch, _id, nullptr, Np.data(), nullptr));
			return Np;
		}
		for (int i = 0; i < n; i++)
			for (size_t b = 0; b < B; b++) Np[((size_t)i * n + i) * B + b] = 1.0;
		for (int s = 0; s < _id; s++) {
			check(saip_batch_get_task_nullspace_host(_batch, s, Ns.data()));
			matmulBatched(Ns, Np, T, n, B);
			Np.swap(T);
		}
		return Np;
	}
	// N N_prec, what the next task of the hierarchy is updated with, TemplateTask.h:85-89
	std::vector<double> getTaskAndPreviousNullspace() {
		const int n = _robot->dof();
		const size_t B = _robot->batchSize();
		if (_manual) {
			std::vector<double> Nt((size_t)n * n * B);
			check(saip_batch_task_get_nullspaces_host(_batch, _id, nullptr, nullptr, Nt.data()));
			return Nt;
		}
		std::vector<double> N = getTaskNullspace(), Np = getPreviousTasksNullspace(), T(N.size());
		matmulBatched(N, Np, T, n, B);
		return T;
	}

protected:
	friend class RobotController;
	static void matmulBatched(const std::vector<double>& A, const std::vector<double>& Bm, std::vector<double>& C, int n, size_t B) {  // [n*n][B] layout
		for (int i = 0; i < n; i++)
			for (int j = 0; j < n; j++)
				for (size_t b = 0; b < B; b++) {
					double s = 0.0;
					for (int l = 0; l < n; l++) s += A[((size_t)i * n + l) * B + b] * Bm[((size_t)l * n + j) * B + b];
					C[((size_t)i * n + j) * B + b] = s;
				}
	}
	template <typename F>
	void cfg(F f) {
		_log.emplace_back(f);  // replayed into whichever batch the task joins later
		if (_batch) check(f(_batch, _id));
	}
	// the batch this task is evaluated in: its RobotController's, or -- for a task driven by hand like in the reference's example 04 --
	// a private one-task batch created on first use
	void need() {
		if (_batch) return;
		saip_batch* b = nullptr;
		check(saip_batch_create(_robot->handle(), _robot->batchSize(), _robot->device(), &b));
		try {
			check(add(b, &_id));
			check(saip_batch_finalize(b));
			for (auto& f : _log) check(f(b, _id));
		} catch (...) {
			saip_batch_destroy(b);
			throw;
		}
		_batch = b;
		_private = true;
		_robot->attach(b);
	}
	void dropPrivateBatch() {
		if (_private && _batch) {
			_robot->detach(_batch);
			saip_batch_destroy(_batch);
		}
		_private = false;
		_batch = nullptr;
	}
	void pushState() { _robot->pushTo(_batch); }
	void pushAndUpdate(const double* N_prec) {
		_robot->pushTo(_batch);
		check(saip_batch_task_update_model(_batch, _id, N_prec));
		_manual = true;
	}
	std::vector<double> torques(const double* tau_prec) {
		need();
		if (!_manual) throw std::runtime_error("task [" + _task_name + "]: call updateTaskModel(N_prec) before computeTorques()");
		std::vector<double> tau((size_t)_robot->dof() * _robot->batchSize());
		_status.assign(_robot->batchSize(), 0);
		check(saip_batch_task_compute_torques(_batch, _id, tau_prec, tau.data(), _status.data()));
		return tau;
	}
	// rows first .. first + comps - 1 of the goal block (desired = false) or of the desired state, [comps][B]; rows the task's goal block
	// does not have (goal force / moment of a task without force or moment space) read as zero, their value in the reference
	std::vector<double> blockRows(bool desired, int first, int comps) {
		need();
		const size_t B = _robot->batchSize();
		const int gc = saip_batch_goal_components(_batch, _id);
		std::vector<double> g((size_t)gc * B);
		check(desired ? saip_batch_get_desired_host(_batch, _id, g.data()) : saip_batch_get_goal_host(_batch, _id, g.data()));
		if (first + comps > gc) return std::vector<double>((size_t)comps * B, 0.0);
		return std::vector<double>(g.begin() + (size_t)first * B, g.begin() + (size_t)(first + comps) * B);
	}
	void setField(int first, int comps, const std::vector<double>& v, const char* what) {
		need();
		if (v.size() != (size_t)comps * _robot->batchSize()) throw std::invalid_argument(what);
		check(saip_batch_set_goal_field_host(_batch, _id, first, comps, v.data()));
	}
	virtual saip_status add(saip_batch* b, int* id) = 0;
	virtual bool scheduleField(const std::string& field, int* first, int* count) const = 0;

	std::shared_ptr<SaiModel> _robot;
	std::string _task_name;
	TaskType _task_type;
	double _loop_timestep;
	bool _otg_enabled = true;  // reference default (JointTask.h:38, MotionForceTask.h:67)
	double _bie_threshold = 0.1;
	saip_batch* _batch = nullptr;
	int _id = -1;
	bool _private = false;  // _batch is this task's own one-task batch (no RobotController)
	bool _manual = false;   // model last updated through updateTaskModel(N_prec)
	std::vector<uint8_t> _status;
	std::vector<std::function<saip_status(saip_batch*, int)>> _log;
};

class MotionForceTask : public TemplateTask {
public:
	// full 6-dof task, MotionForceTask.h:96-101
	MotionForceTask(std::shared_ptr<SaiModel>& robot, const std::string& link_name, const double (&pos_in_link)[3],
					const std::string& task_name = "motion_force_task", double loop_timestep = 0.001)
		: TemplateTask(robot, task_name, MOTION_FORCE_TASK, loop_timestep), _link(link_name), _partial(false) {
		for (int i = 0; i < 3; i++) _pos[i] = pos_in_link[i];
	}
	// partial task, MotionForceTask.h:103-110: controlled directions as flat xyz triples
	MotionForceTask(std::shared_ptr<SaiModel>& robot, const std::string& link_name, const std::vector<double>& controlled_directions_translation,
					const std::vector<double>& controlled_directions_rotation, const double (&pos_in_link)[3],
					const std::string& task_name = "partial_motion_force_task", double loop_timestep = 0.001)
		: TemplateTask(robot, task_name, MOTION_FORCE_TASK, loop_timestep), _link(link_name), _partial(true),
		  _dt(controlled_directions_translation), _dr(controlled_directions_rotation) {
		for (int i = 0; i < 3; i++) _pos[i] = pos_in_link[i];
		if (_dt.empty() && _dr.empty())
			throw std::invalid_argument("controlled_directions_translation and controlled_directions_rotation cannot both be empty in MotionForceTask::MotionForceTask\n");
	}
	void setGoalPosition(const std::vector<double>& x) { setField(0, 3, x, "setGoalPosition: expected [3][B]"); }
	void setGoalOrientation(const std::vector<double>& R) { setField(3, 9, R, "setGoalOrientation: expected [9][B] (row-major R)"); }
	void setGoalLinearVelocity(const std::vector<double>& v) { setField(12, 3, v, "setGoalLinearVelocity: expected [3][B]"); }
	void setGoalAngularVelocity(const std::vector<double>& w) { setField(15, 3, w, "setGoalAngularVelocity: expected [3][B]"); }
	void setGoalLinearAcceleration(const std::vector<double>& a) { setField(18, 3, a, "setGoalLinearAcceleration: expected [3][B]"); }
	void setGoalAngularAcceleration(const std::vector<double>& a) { setField(21, 3, a, "setGoalAngularAcceleration: expected [3][B]"); }
	void setPosControlGains(double kp, double kv, double ki = 0) { cfg([=](saip_batch* b, int id) { return saip_batch_set_pos_control_gains(b, id, &kp, &kv, &ki, 1); }); }
	void setOriControlGains(double kp, double kv, double ki = 0) { cfg([=](saip_batch* b, int id) { return saip_batch_set_ori_control_gains(b, id, &kp, &kv, &ki, 1); }); }
	void enableSingularityHandling() { cfg([](saip_batch* b, int id) { return saip_batch_set_singularity_handling(b, id, 1); }); }    // MotionForceTask.h:715
	void disableSingularityHandling() { cfg([](saip_batch* b, int id) { return saip_batch_set_singularity_handling(b, id, 0); }); }  // :723
	// blended type-1 / type-2 strategies for instances inside the singularity bounds: on by default like in the reference; off = flagged instead
	void setSingularityStrategies(bool enabled) { cfg([=](saip_batch* b, int id) { return saip_batch_set_singularity_strategies(b, id, enabled ? 1 : 0); }); }
	void setSingularityHandlingGains(double kp_type_1, double kv_type_1, double kv_type_2) {  // MotionForceTask.h:749
		cfg([=](saip_batch* b, int id) { return saip_batch_set_singularity_gains(b, id, kp_type_1, kv_type_1, kv_type_2); });
	}
	void handleAllSingularitiesAsType1(bool flag) { cfg([=](saip_batch* b, int id) { return saip_batch_set_all_singularities_type1(b, id, flag ? 1 : 0); }); }  // :698
	void setType1Posture(const std::vector<double>& q_des) {  // :707, one posture for every instance
		cfg([q_des](saip_batch* b, int id) { return saip_batch_set_type1_posture(b, id, q_des.data(), 0); });
	}
	void setSingularityHandlingBounds(double s_min, double s_max) { cfg([=](saip_batch* b, int id) { return saip_batch_set_singularity_bounds(b, id, s_min, s_max); }); }
	// MotionForceTask.cpp:510-523 (defaults MotionForceTask.h:68-71); the jerk-limited variant throws (not on the device)
	void enableInternalOtgAccelerationLimited(double max_linear_velocity = 0.3, double max_linear_acceleration = 2.0,
											  double max_angular_velocity = M_PI / 3, double max_angular_acceleration = 2 * M_PI) {
		_otg_enabled = true;
		cfg([=](saip_batch* b, int id) {
			const double v[2] = {max_linear_velocity, max_angular_velocity}, a[2] = {max_linear_acceleration, max_angular_acceleration};
			return saip_batch_set_otg_acceleration_limited(b, id, v, a, 2);
		});
	}
	// MotionForceTask::enableInternalOtgJerkLimited, MotionForceTask.cpp:525-545 (argument order of MotionForceTask.h:416-421)
	void enableInternalOtgJerkLimited(double max_linear_velocity, double max_linear_acceleration, double max_linear_jerk, double max_angular_velocity,
									  double max_angular_acceleration, double max_angular_jerk) {
		_otg_enabled = true;
		cfg([=](saip_batch* b, int id) {
			const double v[2] = {max_linear_velocity, max_angular_velocity}, a[2] = {max_linear_acceleration, max_angular_acceleration},
						 j[2] = {max_linear_jerk, max_angular_jerk};
			return saip_batch_set_otg_jerk_limited(b, id, v, a, j, 2);
		});
	}
	// MotionForceTask::enableVelocitySaturation(linear, angular), MotionForceTask.cpp:771-792
	void enableVelocitySaturation(double linear_vel_sat = 0.3, double angular_vel_sat = M_PI / 3) {
		cfg([=](saip_batch* b, int id) {
			const double v[2] = {linear_vel_sat, angular_vel_sat};
			saip_status st = saip_batch_set_saturation_velocities(b, id, v, 2);
			return st ? st : saip_batch_set_velocity_saturation(b, id, 1);
		});
	}
	// hybrid motion/force control, MotionForceTask.h:560-600 (open-loop force control; closed loop is refused)
	void parametrizeForceMotionSpaces(int force_space_dimension, double ax = 0, double ay = 0, double az = 0) {
		cfg([=](saip_batch* b, int id) {
			const double a[3] = {ax, ay, az};
			return saip_batch_parametrize_force_motion_spaces(b, id, force_space_dimension, a, nullptr);
		});
	}
	void parametrizeMomentRotMotionSpaces(int moment_space_dimension, double ax = 0, double ay = 0, double az = 0) {
		cfg([=](saip_batch* b, int id) {
			const double a[3] = {ax, ay, az};
			return saip_batch_parametrize_moment_rot_motion_spaces(b, id, moment_space_dimension, a, nullptr);
		});
	}
	void setGoalForce(const std::vector<double>& f) { setField(24, 3, f, "setGoalForce: expected [3][B]"); }
	void setGoalMoment(const std::vector<double>& m) { setField(27, 3, m, "setGoalMoment: expected [3][B]"); }
	void setForceControlGains(double kp, double kv, double ki) { cfg([=](saip_batch* b, int id) { return saip_batch_set_force_control_gains(b, id, kp, kv, ki); }); }
	void setMomentControlGains(double kp, double kv, double ki) { cfg([=](saip_batch* b, int id) { return saip_batch_set_moment_control_gains(b, id, kp, kv, ki); }); }
	void setClosedLoopForceControl(bool e) { cfg([=](saip_batch* b, int id) { return saip_batch_set_closed_loop_force_control(b, id, e); }); }
	void setClosedLoopMomentControl(bool e) { cfg([=](saip_batch* b, int id) { return saip_batch_set_closed_loop_moment_control(b, id, e); }); }
	// control point [3][B] and compliant-frame orientation [9][B] (row-major per instance) in the world frame at the robot's current
	// state, MotionForceTask.h:121-138
	std::vector<double> getCurrentPosition() {
		need();
		std::vector<double> p((size_t)3 * _robot->batchSize());
		pushState();
		check(saip_batch_get_current_pose_host(_batch, _id, p.data(), nullptr));
		return p;
	}
	std::vector<double> getCurrentOrientation() {
		need();
		std::vector<double> r((size_t)9 * _robot->batchSize());
		pushState();
		check(saip_batch_get_current_pose_host(_batch, _id, nullptr, r.data()));
		return r;
	}
	// goal and desired state, [3][B] (orientations [9][B], row-major per instance): MotionForceTask.h getGoal* / getDesired*
	std::vector<double> getGoalPosition() { return blockRows(false, 0, 3); }
	std::vector<double> getGoalOrientation() { return blockRows(false, 3, 9); }
	std::vector<double> getGoalLinearVelocity() { return blockRows(false, 12, 3); }
	std::vector<double> getGoalAngularVelocity() { return blockRows(false, 15, 3); }
	std::vector<double> getGoalLinearAcceleration() { return blockRows(false, 18, 3); }
	std::vector<double> getGoalAngularAcceleration() { return blockRows(false, 21, 3); }
	std::vector<double> getGoalForce() { return blockRows(false, 24, 3); }
	std::vector<double> getGoalMoment() { return blockRows(false, 27, 3); }
	std::vector<double> getDesiredPosition() { return blockRows(true, 0, 3); }
	std::vector<double> getDesiredOrientation() { return blockRows(true, 3, 9); }
	std::vector<double> getDesiredLinearVelocity() { return blockRows(true, 12, 3); }
	std::vector<double> getDesiredAngularVelocity() { return blockRows(true, 15, 3); }
	std::vector<double> getDesiredLinearAcceleration() { return blockRows(true, 18, 3); }
	std::vector<double> getDesiredAngularAcceleration() { return blockRows(true, 21, 3); }
	// task-space diagnostics at the robot's current state, one launch (saip_batch_get_task_diagnostics_host): [24][B], rows 0-2 position
	// error, 3-5 orientation error, 6-8 / 9-11 current linear / angular velocity, 12-14 / 15-17 sensed force / moment (control point,
	// world frame), 18-23 unit-mass force
	std::vector<double> getTaskDiagnostics() {
		need();
		std::vector<double> d((size_t)24 * _robot->batchSize());
		pushState();
		check(saip_batch_get_task_diagnostics_host(_batch, _id, d.data()));
		return d;
	}
	std::vector<double> getPositionError() { return diagRows(0, 3); }                   // MotionForceTask.cpp:540-542
	std::vector<double> getOrientationError() { return diagRows(3, 3); }                // :544-546
	std::vector<double> getCurrentLinearVelocity() { return diagRows(6, 3); }           // :293-295
	std::vector<double> getCurrentAngularVelocity() { return diagRows(9, 3); }          // :296-298
	std::vector<double> getSensedForceControlWorldFrame() { return diagRows(12, 3); }   // :805-828
	std::vector<double> getSensedMomentControlWorldFrame() { return diagRows(15, 3); }
	std::vector<double> getUnitMassForce() { return diagRows(18, 6); }                  // MotionForceTask.h:266 (see saip.h)
	// MotionForceTask.cpp:548-579: sqrt(e^T sigma e) < tolerance per instance.  sigmaPosition / sigmaOrientation are symmetric projectors,
	// so e^T sigma e = |sigma e|^2: the norm of the error rows
	std::vector<bool> goalPositionReached(double tolerance) { return errorBelow(0, tolerance); }
	std::vector<bool> goalOrientationReached(double tolerance) { return errorBelow(3, tolerance); }
	void resetIntegratorsLinear() {
		need();
		check(saip_batch_reset_integrators(_batch, _id, 1));
	}
	void resetIntegratorsAngular() {
		need();
		check(saip_batch_reset_integrators(_batch, _id, 2));
	}
	void enablePassivity() { cfg([](saip_batch* b, int id) { return saip_batch_set_passivity(b, id, 1); }); }    // MotionForceTask.h:630-631
	void disablePassivity() { cfg([](saip_batch* b, int id) { return saip_batch_set_passivity(b, id, 0); }); }
	// MotionForceTask.cpp:805-828: sensed force / moment in the sensor frame, [3][B] each
	void updateSensedForceAndMoment(const std::vector<double>& force, const std::vector<double>& moment) {
		setField(30, 3, force, "updateSensedForceAndMoment: expected [3][B]");
		setField(33, 3, moment, "updateSensedForceAndMoment: expected [3][B]");
	}
	// setFeedforwardForceGain / MomentGain, setMaxForceControlFeedbackOutput / Moment (MotionForceTask.h:330-355) in one call
	void setForceControlParameters(double kff_force = 0.95, double kff_moment = 0.95, double max_force_feedback = 20.0, double max_moment_feedback = 10.0) {
		cfg([=](saip_batch* b, int id) { return saip_batch_set_force_control_parameters(b, id, kff_force, kff_moment, max_force_feedback, max_moment_feedback); });
	}
	void setPosControlGainsUnsafe(double kp, double kv, double ki = 0) { setPosControlGains(kp, kv, ki); }
	void setOriControlGainsUnsafe(double kp, double kv, double ki = 0) { setOriControlGains(kp, kv, ki); }

protected:
	std::vector<double> diagRows(int first, int comps) {
		const std::vector<double> d = getTaskDiagnostics();
		const size_t B = _robot->batchSize();
		return std::vector<double>(d.begin() + (size_t)first * B, d.begin() + (size_t)(first + comps) * B);
	}
	std::vector<bool> errorBelow(int first, double tolerance) {
		const std::vector<double> e = diagRows(first, 3);
		const size_t B = _robot->batchSize();
		std::vector<bool> r(B);
		for (size_t b = 0; b < B; b++) r[b] = std::sqrt(e[b] * e[b] + e[B + b] * e[B + b] + e[2 * B + b] * e[2 * B + b]) < tolerance;
		return r;
	}
	bool scheduleField(const std::string& field, int* first, int* count) const override {
		static const struct {
			const char* name;
			int first, count;
		} fields[] = {{"position", 0, 3},          {"orientation", 3, 9},           {"linear_velocity", 12, 3}, {"angular_velocity", 15, 3},
					  {"linear_acceleration", 18, 3}, {"angular_acceleration", 21, 3}, {"force", 24, 3},           {"moment", 27, 3},
					  {"sensed_force", 30, 3},     {"sensed_moment", 33, 3}};
		for (const auto& f : fields)
			if (field == f.name) {
				*first = f.first;
				*count = f.count;
				return true;
			}
		return false;
	}
	saip_status add(saip_batch* b, int* id) override {
		return saip_batch_add_motion_force_task(b, _task_name.c_str(), _link.c_str(), _pos, nullptr, _dt.empty() ? nullptr : _dt.data(),
												_partial ? (int)_dt.size() / 3 : -1, _dr.empty() ? nullptr : _dr.data(),
												_partial ? (int)_dr.size() / 3 : -1, _loop_timestep, id);
	}
	std::string _link;
	bool _partial;
	double _pos[3];
	std::vector<double> _dt, _dr;
};

class JointTask : public TemplateTask {
public:
	JointTask(std::shared_ptr<SaiModel>& robot, const std::string& task_name = "joint_task", double loop_timestep = 0.001)
		: TemplateTask(robot, task_name, JOINT_TASK, loop_timestep), _rows(0) {}
	// joint_selection_matrix: rows x dof, row-major (JointTask.h:66-75)
	JointTask(std::shared_ptr<SaiModel>& robot, const std::vector<double>& joint_selection_matrix, int rows,
			  const std::string& task_name = "partial_joint_task", double loop_timestep = 0.001)
		: TemplateTask(robot, task_name, JOINT_TASK, loop_timestep), _S(joint_selection_matrix), _rows(rows) {
		if (rows <= 0 || _S.size() != (size_t)rows * robot->dof())
			throw std::invalid_argument("joint selection matrix size not consistent with robot dof in JointTask constructor\n");
	}
	int getTaskDof() const { return _rows > 0 ? _rows : _robot->dof(); }
	bool isFullJointTask() const { return getTaskDof() == _robot->dof(); }
	void setGoalPosition(const std::vector<double>& q) { setField(0, getTaskDof(), q, "goal position vector size not consistent with task dof in JointTask::setGoalPosition\n"); }
	void setGoalVelocity(const std::vector<double>& dq) { setField(getTaskDof(), getTaskDof(), dq, "goal velocity vector size not consistent with task dof in JointTask::setGoalVelocity\n"); }
	void setGoalAcceleration(const std::vector<double>& ddq) { setField(2 * getTaskDof(), getTaskDof(), ddq, "goal acceleration vector size not consistent with task dof in JointTask::setGoalAcceleration\n"); }
	// goal and desired state, [task dof][B] (JointTask.h getGoal* / getDesired*; desired = the OTG output when enabled, else the goal)
	std::vector<double> getGoalPosition() { return blockRows(false, 0, getTaskDof()); }
	std::vector<double> getGoalVelocity() { return blockRows(false, getTaskDof(), getTaskDof()); }
	std::vector<double> getGoalAcceleration() { return blockRows(false, 2 * getTaskDof(), getTaskDof()); }
	std::vector<double> getDesiredPosition() { return blockRows(true, 0, getTaskDof()); }
	std::vector<double> getDesiredVelocity() { return blockRows(true, getTaskDof(), getTaskDof()); }
	std::vector<double> getDesiredAcceleration() { return blockRows(true, 2 * getTaskDof(), getTaskDof()); }
	void setGains(double kp, double kv, double ki = 0) { cfg([=](saip_batch* b, int id) { return saip_batch_set_joint_gains(b, id, &kp, &kv, &ki, 1); }); }
	void setGainsUnsafe(double kp, double kv, double ki = 0) { setGains(kp, kv, ki); }
	// rows x dof, row-major (identity for the full task), JointTask.h getJointSelectionMatrix
	std::vector<double> getJointSelectionMatrix() const {
		if (_rows > 0) return _S;
		const int n = _robot->dof();
		std::vector<double> I((size_t)n * n, 0.0);
		for (int i = 0; i < n; i++) I[(size_t)i * n + i] = 1.0;
		return I;
	}
	// JointTask.cpp:358-381 (defaults JointTask.h:40-41); jerk-limited: JointTask.cpp:383-410
	void enableInternalOtgAccelerationLimited(double max_velocity = M_PI / 3.0, double max_acceleration = 2.0 * M_PI) {
		_otg_enabled = true;
		cfg([=](saip_batch* b, int id) { return saip_batch_set_otg_acceleration_limited(b, id, &max_velocity, &max_acceleration, 1); });
	}
	void enableInternalOtgJerkLimited(double max_velocity, double max_acceleration, double max_jerk) {
		_otg_enabled = true;
		cfg([=](saip_batch* b, int id) { return saip_batch_set_otg_jerk_limited(b, id, &max_velocity, &max_acceleration, &max_jerk, 1); });
	}
	void enableVelocitySaturation(double saturation_velocity = M_PI / 3.0) {  // JointTask.cpp:410-421
		cfg([=](saip_batch* b, int id) {
			saip_status st = saip_batch_set_saturation_velocities(b, id, &saturation_velocity, 1);
			return st ? st : saip_batch_set_velocity_saturation(b, id, 1);
		});
	}

protected:
	bool scheduleField(const std::string& field, int* first, int* count) const override {
		const int m = getTaskDof();
		*count = m;
		*first = field == "position" ? 0 : field == "velocity" ? m : 2 * m;
		return field == "position" || field == "velocity" || field == "acceleration";
	}
	saip_status add(saip_batch* b, int* id) override {
		return saip_batch_add_joint_task(b, _task_name.c_str(), _rows > 0 ? _S.data() : nullptr, _rows, _loop_timestep, id);
	}
	std::vector<double> _S;
	int _rows;
};

// RobotController.h:47-90
class RobotController {
public:
	RobotController(std::shared_ptr<SaiModel>& robot, std::vector<std::shared_ptr<TemplateTask>>& tasks) : _robot(robot), _tasks(tasks) {
		if (tasks.empty()) throw std::invalid_argument("RobotController must have at least one task");
		for (auto& t : tasks)
			if (t->getConstRobotModel() != robot) throw std::invalid_argument("All tasks must have the same robot model in RobotController");
		for (auto& t : tasks)
			if (t->_batch && !t->_private) throw std::invalid_argument("task [" + t->getTaskName() + "] already belongs to a RobotController");
		check(saip_batch_create(robot->handle(), robot->batchSize(), robot->device(), &_batch));
		std::vector<int> ids(tasks.size(), -1);
		try {
			for (size_t i = 0; i < tasks.size(); i++) check(tasks[i]->add(_batch, &ids[i]));
			check(saip_batch_finalize(_batch));
		} catch (...) {
			saip_batch_destroy(_batch);
			_batch = nullptr;
			throw;
		}
		for (size_t i = 0; i < tasks.size(); i++) {
			auto& t = tasks[i];
			// a task that was driven by hand before moves here: configuration replayed, goal kept, integrators start afresh
			std::vector<double> goal;
			if (t->_private && robot->device() >= 0) {
				goal.resize((size_t)saip_batch_goal_components(t->_batch, t->_id) * robot->batchSize());
				check(saip_batch_get_goal_host(t->_batch, t->_id, goal.data()));
			}
			t->dropPrivateBatch();
			t->_batch = _batch;
			t->_id = ids[i];
			t->_manual = false;
			for (auto& f : t->_log) check(f(_batch, t->_id));
			if (!goal.empty()) check(saip_batch_set_goal_host(_batch, t->_id, goal.data()));
			_task_names.push_back(t->getTaskName());
		}
		robot->attach(_batch);
	}
	~RobotController() {
		for (auto& t : _tasks)
			if (t->_batch == _batch) {
				t->_batch = nullptr;
				t->_manual = false;
			}
		_robot->detach(_batch);
		saip_batch_destroy(_batch);
	}
	RobotController(const RobotController&) = delete;
	RobotController& operator=(const RobotController&) = delete;

	void updateControllerTaskModels() {
		pushState();
		check(saip_batch_update_task_models(_batch));
		for (auto& t : _tasks) t->_manual = false;
	}
	// [dof][B] joint torques; instances that left the non-singular branch carry NaN and status()[b] == 1
	std::vector<double> computeControlTorques() {
		std::vector<double> tau((size_t)_robot->dof() * _robot->batchSize());
		_status.assign(_robot->batchSize(), 0);
		check(saip_batch_compute_control_torques(_batch, tau.data(), _status.data()));
		return tau;
	}
	const std::vector<uint8_t>& status() const { return _status; }
	void enableGravityCompensation(bool e) { check(saip_batch_enable_gravity_compensation(_batch, e)); }
	void enableJointLimitAvoidance(bool e) { check(saip_batch_enable_joint_limit_avoidance(_batch, e)); }
	void enableTorqueSaturation(bool e) { check(saip_batch_enable_torque_saturation(_batch, e)); }
	// torques of instances that end a cycle flagged (status 1): false (default) = the last valid torques are held, true = NaN
	void setFlaggedTorquePolicy(bool nan) { check(saip_batch_set_flagged_torque_policy(_batch, nan ? 1 : 0)); }
	void setFlaggedRecompute(bool on_list) { check(saip_batch_set_flagged_recompute(_batch, on_list ? 1 : 0)); }
	void reinitializeTasks() {
		pushState();
		check(saip_batch_reinitialize_tasks(_batch));
	}
	const std::vector<std::string>& getTaskNames() const { return _task_names; }
	std::shared_ptr<JointTask> getJointTaskByName(const std::string& name) { return byName<JointTask>(name, JOINT_TASK, "JointTask"); }
	std::shared_ptr<MotionForceTask> getMotionForceTaskByName(const std::string& name) { return byName<MotionForceTask>(name, MOTION_FORCE_TASK, "MotionForceTask"); }
	saip_batch* handle() { return _batch; }
	void pushState() { _robot->pushTo(_batch); }

	// ---- the resident pipeline (engine extras): control cycles and forward dynamics on the device, no host in the loop
	// one control cycle enqueued on the engine stream (torques: getTorques() after synchronize())
	void stepAsync() { check(saip_batch_step_async(_batch)); }
	// semi-implicit Euler steps of the resident state under the torques of the last cycle; gravity nullptr = the model's
	void integrate(double dt, int substeps = 1, const double* gravity = nullptr, double damping = 0.0) {
		pushState();
		check(saip_batch_integrate(_batch, dt, substeps, gravity, damping));
	}
	// `steps` closed-loop periods {internal OTGs, control cycle, integrate} enqueued without host synchronisation
	void rolloutAsync(int steps, double sim_dt, int substeps = 1, const double* gravity = nullptr, double damping = 0.0) {
		pushState();
		check(saip_batch_rollout_async(_batch, steps, sim_dt, substeps, gravity, damping));
	}
	void synchronize() { check(saip_batch_synchronize(_batch)); }
	// [dof][B] torques of the last cycle; status() is refreshed
	std::vector<double> getTorques() {
		std::vector<double> tau((size_t)_robot->dof() * _robot->batchSize());
		_status.assign(_robot->batchSize(), 0);
		check(saip_batch_get_torques_host(_batch, tau.data(), _status.data()));
		return tau;
	}
	// read the resident state back into the SaiModel mirror (after integrate / rolloutAsync): robot->q(), robot->dq()
	void pullState() {
		std::vector<double> q(_robot->_q.size()), dq(_robot->_dq.size());
		check(saip_batch_get_state_host(_batch, q.data(), dq.data()));
		_robot->_q = std::move(q);
		_robot->_dq = std::move(dq);
		_robot->_version++;
		for (auto& a : _robot->_attached)
			if (a.batch == _batch) a.pushed = _robot->_version;  // the device already holds this state
	}

	// the period counter of the tasks' goal schedules (TemplateTask::setGoalSchedule) back to 0
	void rewindGoalSchedules() { check(saip_batch_goal_schedule_rewind(_batch)); }

	// ---- state snapshots: the complete per-instance state saved on the device and written back through a source index (saip.h).
	// A sampling MPC: auto s = ctrl.saveState(); { ctrl.restoreState(s, 0); ctrl.rolloutAsync(K, ...); rolloutSummary(); } ctrl.restoreState(s, best);
	// Pair a restore with resetRolloutRecorder() / rewindGoalSchedules(): neither is part of a snapshot.
	class StateSnapshot {
	public:
		struct Segment {
			std::string name;
			int rows = 0, elem_bytes = 0, group = 1, kind = SAIP_SNAPSHOT_SOA;
			size_t offset = 0;  // inside tobytes()
		};
		StateSnapshot() = default;
		StateSnapshot(StateSnapshot&& o) noexcept : _s(o._s), _batch(o._batch) { o._s = nullptr; }
		StateSnapshot& operator=(StateSnapshot&& o) noexcept {
			if (this != &o) {
				close();
				_s = o._s;
				_batch = o._batch;
				o._s = nullptr;
			}
			return *this;
		}
		StateSnapshot(const StateSnapshot&) = delete;
		StateSnapshot& operator=(const StateSnapshot&) = delete;
		~StateSnapshot() { close(); }
		void close() {
			saip_snapshot_destroy(_s);
			_s = nullptr;
		}
		bool valid() const { return _s != nullptr; }
		saip_snapshot* handle() const { return _s; }
		size_t bytes() const { return saip_snapshot_bytes(_s); }
		std::vector<Segment> segments() const {
			std::vector<Segment> out((size_t)saip_snapshot_segments(_s));
			for (size_t i = 0; i < out.size(); i++) {
				const char* name = nullptr;
				check(saip_snapshot_segment_info(_s, (int)i, &name, &out[i].rows, &out[i].elem_bytes, &out[i].group, &out[i].kind, &out[i].offset));
				out[i].name = name;
			}
			return out;
		}
		// the snapshot as a host blob (waits for the engine stream); not a stable format across versions of the library
		std::vector<unsigned char> tobytes() const {
			std::vector<unsigned char> blob(bytes());
			check(saip_snapshot_export_host(_batch, _s, blob.data(), blob.size()));
			return blob;
		}

	private:
		friend class RobotController;
		saip_snapshot* _s = nullptr;
		saip_batch* _batch = nullptr;
	};
	StateSnapshot createStateSnapshot() {
		StateSnapshot s;
		check(saip_batch_snapshot_create(_batch, &s._s));
		s._batch = _batch;
		return s;
	}
	// capture the complete resident state into `snapshot` (asynchronous), or into a new one
	void saveState(StateSnapshot& snapshot) {
		pushState();
		check(saip_batch_snapshot_save(_batch, snapshot._s));
	}
	StateSnapshot saveState() {
		StateSnapshot s = createStateSnapshot();
		saveState(s);
		return s;
	}
	// instance i takes the state instance source[i] had at the save: every instance its own / all that of `instance` / a host map of B
	// indices (checked) / a device map of B ints read in stream order (an entry outside 0 .. B-1 leaves that instance as it is)
	void restoreState(const StateSnapshot& snapshot) { restored(saip_batch_snapshot_restore(_batch, snapshot._s, nullptr)); }
	void restoreState(const StateSnapshot& snapshot, int instance) { restoreState(snapshot, std::vector<int>((size_t)_robot->batchSize(), instance)); }
	void restoreState(const StateSnapshot& snapshot, const std::vector<int>& source) {
		if ((int)source.size() != _robot->batchSize()) throw std::invalid_argument("restoreState: one source index per instance expected");
		restored(saip_batch_snapshot_restore(_batch, snapshot._s, source.data()));
	}
	void restoreStateDevice(const StateSnapshot& snapshot, const int* source_dev) { restored(saip_batch_snapshot_restore_device(_batch, snapshot._s, source_dev)); }
	// a new snapshot of this controller filled from a blob of tobytes(); the controller must have the layout the blob was taken from
	StateSnapshot stateSnapshotFromBytes(const std::vector<unsigned char>& blob) {
		StateSnapshot s = createStateSnapshot();
		check(saip_snapshot_import_host(_batch, s._s, blob.data(), blob.size()));
		return s;
	}

	// ---- resident rollout sampler (task->attachSampler; saip.h): the device steps of a sampling-MPC round
	//   auto s = ctrl.saveState();
	//   per round: ctrl.restoreState(s, 0); rewindGoalSchedules(); resetRolloutRecorder(); perturbGoalSchedules(); rolloutAsync(K, dt);
	//              rolloutCost(...); updateSampler(temperature);
	//   ctrl.restoreStateBest(s);
	struct SamplerResult {
		int best = -1, n_valid = 0;
		double min_cost = 0, sum_w = 0, ess = 0;
	};
	void seedSampler(unsigned long long seed) { check(saip_batch_sampler_seed(_batch, seed)); }
	void perturbGoalSchedules() { check(saip_batch_sampler_perturb(_batch)); }
	// summary_weights: 8 or none; target: 3 or none
	void rolloutCost(const std::vector<double>& summary_weights = {}, const std::vector<double>& target = {}, double path_weight = 0, double final_weight = 0) {
		if (!summary_weights.empty() && summary_weights.size() != SAIP_RECORD_SUMMARY_ROWS) throw std::invalid_argument("rolloutCost: 8 summary weights expected");
		if (!target.empty() && target.size() != 3) throw std::invalid_argument("rolloutCost: a target of 3 components expected");
		check(saip_batch_sampler_cost(_batch, summary_weights.empty() ? nullptr : summary_weights.data(), target.empty() ? nullptr : target.data(), path_weight, final_weight));
	}
	void setRolloutCost(const std::vector<double>& cost) {
		if ((int)cost.size() != _robot->batchSize()) throw std::invalid_argument("setRolloutCost: one cost per instance expected");
		check(saip_batch_sampler_set_cost_host(_batch, cost.data()));
	}
	std::vector<double> getRolloutCost() {
		std::vector<double> out((size_t)_robot->batchSize());
		check(saip_batch_sampler_get_cost_host(_batch, out.data()));
		return out;
	}
	void updateSampler(double temperature) { check(saip_batch_sampler_update(_batch, temperature)); }
	void shiftSampler(int n) { check(saip_batch_sampler_shift(_batch, n)); }
	SamplerResult samplerResult() {
		SamplerResult r;
		check(saip_batch_sampler_result_host(_batch, &r.best, &r.n_valid, &r.min_cost, &r.sum_w, &r.ess));
		return r;
	}
	// every instance takes the saved state of the last update's best instance (the device-resident best map; none is moved without a finite cost)
	void restoreStateBest(const StateSnapshot& snapshot) {
		const int* map = saip_batch_sampler_best_map_device(_batch);
		if (!map) throw std::runtime_error("restoreStateBest: no sampler is attached");
		restoreStateDevice(snapshot, map);
	}
	// ---- scenario groups (saip.h): B = C * M instances as C candidate plans rolled out in M scenarios each, instance i = s * C + c.
	//   risk "mean", "max" or "cvar"; alpha in (0, 1] with "cvar" only (the mean of the worst ceil(alpha * M) scenarios), else 0
	struct SamplerScenarios {
		int n_scenarios = 1, n_candidates = 0, tail = 0;
		std::string risk = "mean";
	};
	void setSamplerScenarios(int n_scenarios, const std::string& risk = "mean", double alpha = 0) {
		const int r = risk == "mean" ? SAIP_SAMPLER_RISK_MEAN : risk == "max" ? SAIP_SAMPLER_RISK_MAX : risk == "cvar" ? SAIP_SAMPLER_RISK_CVAR : -1;
		if (r < 0) throw std::invalid_argument("setSamplerScenarios: unknown risk \"" + risk + "\" (mean, max or cvar)");
		int tail = 0;
		if (r == SAIP_SAMPLER_RISK_CVAR) {
			if (!(alpha > 0.0 && alpha <= 1.0)) throw std::invalid_argument("setSamplerScenarios: risk \"cvar\" needs alpha in (0, 1], got " + std::to_string(alpha));
			tail = std::min(n_scenarios, std::max(1, (int)std::ceil(alpha * n_scenarios)));
		} else if (alpha != 0.0)
			throw std::invalid_argument("setSamplerScenarios: alpha = " + std::to_string(alpha) + " applies to risk \"cvar\" only, not to \"" + risk + "\"");
		check(saip_batch_sampler_set_scenarios(_batch, n_scenarios, r, tail));
	}
	SamplerScenarios samplerScenarios() {
		SamplerScenarios s;
		int risk = 0;
		check(saip_batch_sampler_scenarios_info(_batch, &s.n_scenarios, &s.n_candidates, &risk, &s.tail));
		s.risk = risk == SAIP_SAMPLER_RISK_MAX ? "max" : risk == SAIP_SAMPLER_RISK_CVAR ? "cvar" : "mean";
		return s;
	}
	// [C] the group cost per candidate of the last updateSampler(); without scenario groups the per-instance costs themselves
	std::vector<double> samplerGroupCost() {
		std::vector<double> out((size_t)samplerScenarios().n_candidates);
		check(saip_batch_sampler_get_group_cost_host(_batch, out.data()));
		return out;
	}
	// column i of every resident per-instance randomisable table takes column (i / C) * C; returns the number of arrays touched
	int shareScenarioTables() {
		int n = 0;
		check(saip_batch_sampler_share_scenario_tables(_batch, &n));
		return n;
	}

	// ---- rollout recorder: per-period trajectory log and running summaries of rolloutAsync, kept on the device (saip.h)
	struct RolloutLog {
		int samples = 0, rows = 0, first_period = 0, stride = 1;
		std::vector<double> data;     // [samples][rows][B], chronological; rows: the recorded channels in the order of their bits
		std::vector<uint8_t> status;  // [samples][B]
	};
	// channels: SAIP_RECORD_* bits; task: the motion-force task of the pose / error channels and of the error summaries, or nullptr
	void recordRollouts(int capacity, int stride = 1, unsigned channels = SAIP_RECORD_Q | SAIP_RECORD_DQ | SAIP_RECORD_TAU,
						const std::shared_ptr<MotionForceTask>& task = nullptr, bool summaries = false) {
		const TemplateTask* t = task.get();
		if (t && t->_batch != _batch) throw std::invalid_argument("recordRollouts: the task does not belong to this controller");
		check(saip_batch_rollout_recorder_attach(_batch, capacity, stride, channels, t ? t->_id : -1, summaries ? 1 : 0));
	}
	void stopRecordingRollouts() { check(saip_batch_rollout_recorder_detach(_batch)); }
	void resetRolloutRecorder() { check(saip_batch_rollout_recorder_reset(_batch)); }
	RolloutLog rolloutLog() {
		RolloutLog log;
		check(saip_batch_rollout_log_info(_batch, &log.samples, &log.rows, &log.first_period, &log.stride));
		log.data.resize((size_t)log.samples * log.rows * _robot->batchSize());
		log.status.resize((size_t)log.samples * _robot->batchSize());
		if (log.samples) check(saip_batch_rollout_log_host(_batch, log.data.data(), log.status.data()));
		return log;
	}
	// [8][B] (saip.h)
	std::vector<double> rolloutSummary() {
		std::vector<double> out((size_t)SAIP_RECORD_SUMMARY_ROWS * _robot->batchSize());
		check(saip_batch_rollout_summary_host(_batch, out.data()));
		return out;
	}
	// the simulated sensor of the attached contact planes (task->attachContactPlanes) at the current state: what a rollout period does first,
	// for a host-driven loop { contactSense, computeControlTorques / stepAsync, integrate }
	void contactSense() {
		check(saip_batch_contact_info(_batch, nullptr, nullptr, nullptr, nullptr, nullptr));  // without an attachment: that error, before the device is needed
		pushState();
		check(saip_batch_contact_sense(_batch));
	}
	// the simulated sensors of the attached contact patches (task->attachContactPatch): the same, for { contactPatchSense, stepAsync, integrate }
	void contactPatchSense() {
		check(saip_batch_contact_patch_info(_batch, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));  // without a patch: that error first
		pushState();
		check(saip_batch_contact_patch_sense(_batch));
	}

	// ---- clearance monitor: link spheres against world-fixed obstacles and against each other, inside rollouts (saip.h).  While attached
	// every period of rolloutAsync advances clearanceSummary(); clearanceCost() adds it to the sampler's cost:
	//   per round: ... resetRolloutRecorder(); resetClearanceSummary(); perturbGoalSchedules(); rolloutAsync(K, dt); rolloutCost(...);
	//              clearanceCost(w_penalty); updateSampler(temperature);
	struct ClearanceSphere {
		std::string link;
		std::array<double, 3> centre;  // in the link frame
		double radius;
	};
	struct ClearanceInfo {
		int n_spheres = 0, n_obstacles = 0, per_instance = 0, n_pairs = 0, keep_centres = 0;
		double margin = 0;
		long long period = 0;  // monitored periods since the last reset
	};
	// obstacles: [O][8] rows { kind, a[3], b[3], r } (kind 0 a capsule a-b of radius r, kind 1 a half-space with unit normal a and offset
	// b[0]), or [O][8][B] with per_instance; pairs: (s1, s2) sphere indices
	void attachClearance(const std::vector<ClearanceSphere>& spheres, const std::vector<double>& obstacles = {}, const std::vector<std::array<int, 2>>& pairs = {},
						 double margin = 0.0, bool per_instance = false, bool keep_centres = false) {
		const size_t per = (size_t)SAIP_CLEARANCE_OBSTACLE_WORDS * (per_instance ? (size_t)_robot->batchSize() : 1);
		if (obstacles.size() % per) throw std::invalid_argument("attachClearance: expected [O][8] obstacles, or [O][8][B] per instance");
		std::vector<int> links, pr;
		std::vector<double> centres, radii;
		for (const auto& s : spheres) {
			links.push_back(_robot->linkIndex(s.link));
			centres.insert(centres.end(), s.centre.begin(), s.centre.end());
			radii.push_back(s.radius);
		}
		for (const auto& p : pairs) pr.insert(pr.end(), p.begin(), p.end());
		check(saip_batch_clearance_attach(_batch, (int)spheres.size(), links.data(), centres.data(), radii.data(), (int)(obstacles.size() / per),
										  obstacles.empty() ? nullptr : obstacles.data(), per_instance ? 1 : 0, (int)pairs.size(), pr.empty() ? nullptr : pr.data(), margin,
										  keep_centres ? 1 : 0));
	}
	void detachClearance() { check(saip_batch_clearance_detach(_batch)); }
	ClearanceInfo clearanceInfo() {
		ClearanceInfo i;
		check(saip_batch_clearance_info(_batch, &i.n_spheres, &i.n_obstacles, &i.per_instance, &i.n_pairs, &i.margin, &i.keep_centres, &i.period));
		return i;
	}
	void setClearanceObstacles(const std::vector<double>& obstacles) {
		const ClearanceInfo i = clearanceInfo();
		if (obstacles.size() != (size_t)i.n_obstacles * SAIP_CLEARANCE_OBSTACLE_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setClearanceObstacles: the shape of the attached obstacle table expected");
		check(saip_batch_clearance_set_obstacles_host(_batch, obstacles.data()));
	}
	// one evaluation at the current state: clearanceReadout() (and the kept centres) only, the summaries stay
	void evaluateClearance() {
		clearanceInfo();  // without an attachment: that error, before the device is needed
		pushState();
		check(saip_batch_clearance_evaluate(_batch));
	}
	// [8][B]: the smallest signed distance, its item k (s O + o, then S O + p), the penalty, the items under the margin, the centre of the
	// (first) sphere of item k (3), the smallest self-pair distance -- of the last launch; waits for the stream
	std::vector<double> clearanceReadout() {
		std::vector<double> out((size_t)SAIP_CLEARANCE_READOUT_ROWS * _robot->batchSize());
		check(saip_batch_clearance_readout_host(_batch, out.data()));
		return out;
	}
	// [4][B]: min over the monitored periods of the distance, sum dt * penalty, periods in collision, the first of them or -1; waits for the stream
	std::vector<double> clearanceSummary() {
		std::vector<double> out((size_t)SAIP_CLEARANCE_SUMMARY_ROWS * _robot->batchSize());
		check(saip_batch_clearance_summary_host(_batch, out.data()));
		return out;
	}
	// pair it with restoreState: the summaries are not part of a snapshot
	void resetClearanceSummary() { check(saip_batch_clearance_summary_reset(_batch)); }
	double* clearanceObstaclesDevice() { return saip_batch_clearance_obstacles_device(_batch); }
	double* clearanceCentresDevice() { return saip_batch_clearance_centres_device(_batch); }  // [3 S][ld]; nullptr unless keep_centres
	// cost += w_penalty * summary penalty + (min distance < d_safe ? w_collision : 0), after rolloutCost(); the default makes collision a hard constraint
	void clearanceCost(double w_penalty, double w_collision = std::numeric_limits<double>::infinity(), double d_safe = 0.0) {
		check(saip_batch_clearance_add_cost(_batch, w_penalty, w_collision, d_safe));
	}
	// ---- link contact: world-fixed obstacles push back on the robot's link spheres in front of every integration substep (saip.h).  While
	// attached integrate() and rolloutAsync() add sum_s J_v(c_s)^T F_s to the torques they integrate and advance linkContactSummary();
	// linkContactCost() adds it to the sampler's cost, after rolloutCost() as clearanceCost() is.
	struct LinkContactInfo {
		int n_spheres = 0, n_obstacles = 0, per_instance = 0, keep = 0;
	};
	// obstacles: [O][8] rows as attachClearance takes them, or [O][8][B] with per_instance; materials: [O][4] rows { k, c, mu, v_s }
	void attachLinkContact(const std::vector<ClearanceSphere>& spheres, const std::vector<double>& obstacles, const std::vector<double>& materials,
						   bool per_instance = false, bool keep = false) {
		const size_t per = (size_t)SAIP_LINK_CONTACT_OBSTACLE_WORDS * (per_instance ? (size_t)_robot->batchSize() : 1);
		if (obstacles.size() % per) throw std::invalid_argument("attachLinkContact: expected [O][8] obstacles, or [O][8][B] per instance");
		if (materials.size() != obstacles.size() / per * SAIP_LINK_CONTACT_MATERIAL_WORDS) throw std::invalid_argument("attachLinkContact: expected [O][4] materials");
		std::vector<int> links;
		std::vector<double> centres, radii;
		for (const auto& s : spheres) {
			links.push_back(_robot->linkIndex(s.link));
			centres.insert(centres.end(), s.centre.begin(), s.centre.end());
			radii.push_back(s.radius);
		}
		check(saip_batch_link_contact_attach(_batch, (int)spheres.size(), links.data(), centres.data(), radii.data(), (int)(obstacles.size() / per),
											 obstacles.empty() ? nullptr : obstacles.data(), materials.empty() ? nullptr : materials.data(), per_instance ? 1 : 0, keep ? 1 : 0));
	}
	void detachLinkContact() { check(saip_batch_link_contact_detach(_batch)); }
	LinkContactInfo linkContactInfo() {
		LinkContactInfo i;
		check(saip_batch_link_contact_info(_batch, &i.n_spheres, &i.n_obstacles, &i.per_instance, &i.keep));
		return i;
	}
	void setLinkContactObstacles(const std::vector<double>& obstacles) {
		const LinkContactInfo i = linkContactInfo();
		if (obstacles.size() != (size_t)i.n_obstacles * SAIP_LINK_CONTACT_OBSTACLE_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setLinkContactObstacles: the shape of the attached obstacle table expected");
		check(saip_batch_link_contact_set_obstacles_host(_batch, obstacles.data()));
	}
	void setLinkContactMaterials(const std::vector<double>& materials) {
		const LinkContactInfo i = linkContactInfo();
		if (materials.size() != (size_t)i.n_obstacles * SAIP_LINK_CONTACT_MATERIAL_WORDS) throw std::invalid_argument("setLinkContactMaterials: expected [O][4] materials");
		check(saip_batch_link_contact_set_materials_host(_batch, materials.data()));
	}
	// one evaluation at the current state: linkContactReadout() (and the kept arrays) only, torques and summaries stay
	void evaluateLinkContact() {
		linkContactInfo();  // without an attachment: that error, before the device is needed
		pushState();
		check(saip_batch_link_contact_evaluate(_batch));
	}
	// [8][B]: the net force (3), the smallest signed distance, its item s O + o, the active items, sum f_n, the largest single-item |f| -- of
	// the last launch; waits for the stream
	std::vector<double> linkContactReadout() {
		std::vector<double> out((size_t)SAIP_LINK_CONTACT_READOUT_ROWS * _robot->batchSize());
		check(saip_batch_link_contact_readout_host(_batch, out.data()));
		return out;
	}
	// [4][B]: sum dt sum f_n, the largest single-item |f|, the largest penetration, substeps with an active item; waits for the stream
	std::vector<double> linkContactSummary() {
		std::vector<double> out((size_t)SAIP_LINK_CONTACT_SUMMARY_ROWS * _robot->batchSize());
		check(saip_batch_link_contact_summary_host(_batch, out.data()));
		return out;
	}
	// pair it with restoreState: the summaries are not part of a snapshot
	void resetLinkContactSummary() { check(saip_batch_link_contact_summary_reset(_batch)); }
	double* linkContactObstaclesDevice() { return saip_batch_link_contact_obstacles_device(_batch); }
	double* linkContactTorquesDevice() { return saip_batch_link_contact_torques_device(_batch); }  // [dof][ld] tau_sim of the last integrated substep
	double* linkContactKeepDevice() { return saip_batch_link_contact_keep_device(_batch); }        // [9 S][ld]; nullptr unless keep
	// cost += w_impulse * summary impulse + w_peak * summary peak force, after rolloutCost()
	void linkContactCost(double w_impulse, double w_peak = 0.0) { check(saip_batch_link_contact_add_cost(_batch, w_impulse, w_peak)); }
	// ---- link object: a free rigid body the robot's link spheres push, the second stage of link contact (saip.h).  While attached every
	// integration substep lets the robot and the link-contact obstacles push the body and integrates it; its state is part of a snapshot.
	struct ObjectSphere {
		double centre[3];  // in the body frame
		double radius;
	};
	struct LinkObjectInfo {
		int n_spheres = 0, per_instance = 0;
	};
	// material: [4] { k, c, mu, v_s }; inertial: [4] { m, Ix, Iy, Iz }, or [4][B] with per_instance
	void attachLinkObject(const std::vector<ObjectSphere>& spheres, const std::vector<double>& material, const std::vector<double>& inertial, bool per_instance = false) {
		if (material.size() != SAIP_LINK_CONTACT_MATERIAL_WORDS) throw std::invalid_argument("attachLinkObject: expected a [4] material");
		if (inertial.size() != (size_t)SAIP_LINK_OBJECT_INERTIAL_WORDS * (per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("attachLinkObject: expected [4] inertial words, or [4][B] per instance");
		std::vector<double> centres, radii;
		for (const auto& s : spheres) {
			centres.insert(centres.end(), s.centre, s.centre + 3);
			radii.push_back(s.radius);
		}
		check(saip_batch_link_object_attach(_batch, (int)spheres.size(), centres.data(), radii.data(), material.data(), inertial.data(), per_instance ? 1 : 0));
	}
	void detachLinkObject() { check(saip_batch_link_object_detach(_batch)); }
	LinkObjectInfo linkObjectInfo() {
		LinkObjectInfo i;
		check(saip_batch_link_object_info(_batch, &i.n_spheres, &i.per_instance));
		return i;
	}
	// [13] for every instance, or [13][B]: p, quaternion (w, x, y, z) body to world (normalised by the engine), v, omega (world frame)
	void setObjectState(const std::vector<double>& state) {
		const size_t R = SAIP_LINK_OBJECT_STATE_ROWS;
		if (state.size() != R && state.size() != R * (size_t)_robot->batchSize()) throw std::invalid_argument("setObjectState: expected a [13] or [13][B] state");
		check(saip_batch_link_object_set_state_host(_batch, state.data(), state.size() == R ? 0 : 1));
	}
	std::vector<double> objectState() {  // [13][B]
		std::vector<double> out((size_t)SAIP_LINK_OBJECT_STATE_ROWS * _robot->batchSize());
		check(saip_batch_link_object_state_host(_batch, out.data()));
		return out;
	}
	std::vector<double> objectReadout() {  // [12][B]: robot-on-object force 3, moment 3, world force 3, distance, item, active items
		std::vector<double> out((size_t)SAIP_LINK_OBJECT_READOUT_ROWS * _robot->batchSize());
		check(saip_batch_link_object_readout_host(_batch, out.data()));
		return out;
	}
	std::vector<double> objectSummary() {  // [4][B]: impulse, largest robot-object penetration, largest object-world penetration, substeps in contact
		std::vector<double> out((size_t)SAIP_LINK_OBJECT_SUMMARY_ROWS * _robot->batchSize());
		check(saip_batch_link_object_summary_host(_batch, out.data()));
		return out;
	}
	void resetObjectSummary() { check(saip_batch_link_object_summary_reset(_batch)); }
	double* objectStateDevice() { return saip_batch_link_object_state_device(_batch); }  // [13][ld]; nullptr when detached
	// cost += w_pos |p - target_p|^2 + w_ori (1 - (q . target_quat)^2), after rolloutCost(); target_quat empty: the position term alone
	void objectCost(const std::array<double, 3>& target_p, double w_pos, const std::vector<double>& target_quat = {}, double w_ori = 0.0) {
		if (!target_quat.empty() && target_quat.size() != 4) throw std::invalid_argument("objectCost: expected a [4] target quaternion, or none");
		check(saip_batch_link_object_add_cost(_batch, target_p.data(), w_pos, target_quat.empty() ? nullptr : target_quat.data(), w_ori));
	}
	// ---- guards: event-triggered phases inside rollouts (task->attachGuards; saip.h).  rolloutAsync() evaluates them in every period in
	// front of the OTG step and the cycle; evaluateGuards() does the same for a host-driven loop { contactSense, evaluateGuards, stepAsync,
	// integrate }.
	struct GuardInfo {
		int task = -1, n_guards = 0, per_instance = 0, n_phases = 0, needs_pose = 0;
	};
	struct GuardState {
		std::vector<int> phase, since, clock, run, entry, fires;  // [B], [B], [B], [G][B], [P][B], [G][B]
		std::vector<double> latch;                                // [12][B]: position 3, rotation 9 row-major
	};
	GuardInfo guardInfo() {
		GuardInfo i;
		check(saip_batch_guard_info(_batch, &i.task, &i.n_guards, &i.per_instance, &i.n_phases, &i.needs_pose));
		return i;
	}
	void evaluateGuards() {
		guardInfo();  // without an attachment: that error, before the device is needed
		pushState();
		check(saip_batch_guard_evaluate(_batch));
	}
	void resetGuards() { check(saip_batch_guard_reset(_batch)); }
	// waits for the stream
	GuardState guardState() {
		const GuardInfo i = guardInfo();
		const size_t B = (size_t)_robot->batchSize();
		GuardState s;
		s.phase.resize(B);
		s.since.resize(B);
		s.clock.resize(B);
		s.run.resize(i.n_guards * B);
		s.entry.resize(i.n_phases * B);
		s.fires.resize(i.n_guards * B);
		s.latch.resize(12 * B);
		check(saip_batch_guard_state_host(_batch, s.phase.data(), s.since.data(), s.clock.data(), s.run.data(), s.entry.data(), s.fires.data(), s.latch.data()));
		return s;
	}
	// [8][B]: force norm, moment norm, position error norm, orientation error norm, joint speed, position 3 -- of the last launch, NaN where
	// the tables did not need the quantity; waits for the stream
	std::vector<double> guardReadout() {
		std::vector<double> out((size_t)SAIP_GUARD_READOUT_ROWS * _robot->batchSize());
		check(saip_batch_guard_readout_host(_batch, out.data()));
		return out;
	}
	double* guardTableDevice() { return saip_batch_guard_guards_device(_batch); }  // [G][8] or [G][8][ld]; nullptr when detached
	// cost += w_time * (period of the first entry into `phase`), or w_miss where the instance never got there, after rolloutCost()
	void guardCost(int phase, double w_time, double w_miss = std::numeric_limits<double>::infinity()) {
		check(saip_batch_guard_add_cost(_batch, phase, w_time, w_miss));
	}
	// ---- environment schedules: obstacles and contact surfaces that move inside rollouts (saip.h; the contact side: task->setContactSchedule).
	// keyframes: [K][n][8] obstacle rows, or [K][n][8][B] when the obstacle table is per instance.  The monitor of rollout period c looks at
	// the state at the END of the period, so it sees the obstacles of period index c + 1; the last keyframe is held.
	void setObstacleSchedule(const std::vector<double>& keyframes, int n_keyframes, int stride = 1, int mode = SAIP_ENV_HOLD, int first = 0) {
		const ClearanceInfo ci = clearanceInfo();
		const size_t frame = (size_t)SAIP_CLEARANCE_OBSTACLE_WORDS * (ci.per_instance ? (size_t)saip_batch_size(_batch) : 1);
		if (n_keyframes < 1 || keyframes.empty() || keyframes.size() % ((size_t)n_keyframes * frame) != 0)
			throw std::invalid_argument("setObstacleSchedule: expected [K][n][8] keyframes, or [K][n][8][B] when the obstacles are per instance");
		check(saip_batch_env_schedule_attach(_batch, SAIP_ENV_TARGET_OBSTACLES, -1, first, (int)(keyframes.size() / ((size_t)n_keyframes * frame)), keyframes.data(),
											 n_keyframes, stride, mode));
	}
	void clearObstacleSchedule() { check(saip_batch_env_schedule_detach(_batch, SAIP_ENV_TARGET_OBSTACLES, -1)); }
	TemplateTask::EnvScheduleInfo obstacleScheduleInfo() {
		TemplateTask::EnvScheduleInfo i;
		check(saip_batch_env_schedule_info(_batch, SAIP_ENV_TARGET_OBSTACLES, -1, &i.first, &i.n_items, &i.n_keyframes, &i.stride, &i.mode, &i.per_instance, &i.period));
		return i;
	}
	void clearEnvironmentSchedules() { check(saip_batch_env_schedule_detach(_batch, -1, -1)); }
	// the next rollout period is period `period` of the environment schedules: 0 to replay them, the current period to start a
	// receding-horizon prediction at the current time; what goes with restoreState (tables are not part of a snapshot)
	void rewindEnvironment(long long period = 0) { check(saip_batch_env_schedule_rewind(_batch, period)); }

	// ---- plant model: actuator limits, friction, joint stops and external wrenches between the commanded torques and the resident
	// simulator (saip.h).  While attached, integrate() and rolloutAsync() run it in front of every substep (and in front of the contact
	// launch, if any); the period counter of the wrench windows advances once per integrate() and once per rollout period.
	struct PlantWrench {
		std::string link;
		std::array<double, 3> point;   // in the link frame
		bool link_frame;               // F and M are given in the link frame (else: the world)
		std::vector<double> values;    // { F[3], M[3], p_start, p_end }: 8, or [8][B] with per_instance
	};
	struct PlantInfo {
		int per_instance_joints = 0, n_wrenches = 0, per_instance_wrenches = 0;
		long long period = 0;          // the period the next integration belongs to
	};
	// [dof][10] rows { gain, bias, tau_max, fv, fc, v_s, q_lo, q_hi, k_stop, c_stop } that change nothing, with the model's joint limits
	std::vector<double> neutralPlantJoints() {
		const int n = _robot->dof();
		std::vector<double> lo(n), hi(n), t((size_t)n * SAIP_PLANT_JOINT_WORDS, 0.0);
		check(saip_model_joint_limits(_robot->_model, lo.data(), hi.data(), nullptr, nullptr));
		for (int j = 0; j < n; j++) {
			double* w = t.data() + (size_t)j * SAIP_PLANT_JOINT_WORDS;
			const bool limits = lo[j] <= hi[j];
			w[0] = 1.0;
			w[2] = std::numeric_limits<double>::infinity();
			w[6] = limits ? lo[j] : -w[2];
			w[7] = limits ? hi[j] : w[2];
		}
		return t;
	}
	// joints: [dof][10], or [dof][10][B] with per_instance; empty: the neutral rows.  wrenches: up to SAIP_PLANT_MAX_WRENCHES
	void attachPlant(const std::vector<double>& joints = {}, const std::vector<PlantWrench>& wrenches = {}, bool per_instance = false) {
		const size_t cols = per_instance ? (size_t)_robot->batchSize() : 1;
		if (!joints.empty() && joints.size() != (size_t)_robot->dof() * SAIP_PLANT_JOINT_WORDS * cols)
			throw std::invalid_argument("attachPlant: expected [dof][10] joints, or [dof][10][B] per instance");
		std::vector<int> links, frames;
		std::vector<double> points, table(wrenches.size() * SAIP_PLANT_WRENCH_WORDS * cols);
		for (size_t k = 0; k < wrenches.size(); k++) {
			const PlantWrench& w = wrenches[k];
			if (w.values.size() != SAIP_PLANT_WRENCH_WORDS * cols) throw std::invalid_argument("attachPlant: expected 8 values per wrench, or [8][B] per instance");
			links.push_back(_robot->linkIndex(w.link));
			frames.push_back(w.link_frame ? SAIP_PLANT_FRAME_LINK : SAIP_PLANT_FRAME_WORLD);
			points.insert(points.end(), w.point.begin(), w.point.end());
			std::copy(w.values.begin(), w.values.end(), table.begin() + k * SAIP_PLANT_WRENCH_WORDS * cols);
		}
		check(saip_batch_plant_attach(_batch, joints.empty() ? nullptr : joints.data(), per_instance ? 1 : 0, (int)wrenches.size(), links.data(), points.data(),
									  frames.data(), table.data(), per_instance ? 1 : 0));
	}
	void detachPlant() { check(saip_batch_plant_detach(_batch)); }
	PlantInfo plantInfo() {
		PlantInfo i;
		check(saip_batch_plant_info(_batch, &i.per_instance_joints, &i.n_wrenches, &i.per_instance_wrenches, &i.period));
		return i;
	}
	void setPlantJoints(const std::vector<double>& joints) {
		const PlantInfo i = plantInfo();
		if (joints.size() != (size_t)_robot->dof() * SAIP_PLANT_JOINT_WORDS * (i.per_instance_joints ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setPlantJoints: the shape of the attached joint table expected");
		check(saip_batch_plant_set_joints_host(_batch, joints.data()));
	}
	void setPlantWrenches(const std::vector<double>& values) {
		const PlantInfo i = plantInfo();
		if (values.size() != (size_t)i.n_wrenches * SAIP_PLANT_WRENCH_WORDS * (i.per_instance_wrenches ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setPlantWrenches: the shape of the attached wrench table expected");
		check(saip_batch_plant_set_wrenches_host(_batch, values.data()));
	}
	// per-instance tables drawn on the device, uniform between two batch-uniform tables ([dof][10], [W][8]); an empty pair leaves that table alone
	void randomizePlant(unsigned long long seed, long long round, const std::vector<double>& joint_lo, const std::vector<double>& joint_hi,
						const std::vector<double>& wrench_lo = {}, const std::vector<double>& wrench_hi = {}) {
		const PlantInfo i = plantInfo();
		const size_t jw = (size_t)_robot->dof() * SAIP_PLANT_JOINT_WORDS, ww = (size_t)i.n_wrenches * SAIP_PLANT_WRENCH_WORDS;
		if ((!joint_lo.empty() || !joint_hi.empty()) && (joint_lo.size() != jw || joint_hi.size() != jw))
			throw std::invalid_argument("randomizePlant: expected [dof][10] joint bounds");
		if ((!wrench_lo.empty() || !wrench_hi.empty()) && (wrench_lo.size() != ww || wrench_hi.size() != ww))
			throw std::invalid_argument("randomizePlant: expected [W][8] wrench bounds");
		check(saip_batch_plant_randomize(_batch, seed, round, joint_lo.empty() ? nullptr : joint_lo.data(), joint_hi.empty() ? nullptr : joint_hi.data(),
										 wrench_lo.empty() ? nullptr : wrench_lo.data(), wrench_hi.empty() ? nullptr : wrench_hi.data()));
	}
	// pair it with restoreState: the counter is not part of a snapshot
	void setPlantPeriod(long long period) { check(saip_batch_plant_set_period(_batch, period)); }
	// [4][B]: sum dt sum_j |fr_j dq_j|, the largest clipped torque, substeps in which a joint clipped or a stop acted, sum dt sum ext_j dq_j; waits for the stream
	std::vector<double> plantSummary() {
		std::vector<double> out((size_t)SAIP_PLANT_SUMMARY_ROWS * _robot->batchSize());
		check(saip_batch_plant_summary_host(_batch, out.data()));
		return out;
	}
	void resetPlantSummary() { check(saip_batch_plant_summary_reset(_batch)); }
	double* plantJointsDevice() { return saip_batch_plant_joints_device(_batch); }      // [dof][10] or [dof][10][ld]
	double* plantWrenchesDevice() { return saip_batch_plant_wrenches_device(_batch); }  // [W][8] or [W][8][ld]; nullptr without wrenches
	double* plantTorquesDevice() { return saip_batch_plant_torques_device(_batch); }    // [dof][ld] actuated torques of the last substep
	double* plantSummaryDevice() { return saip_batch_plant_summary_device(_batch); }    // [4][ld]

	// ---- actuation chain: per joint a delay line, a slew-rate limit and a first-order lag between the commanded torque and the plant's
	// joint rows (saip.h).  Needs an attached plant model (attachPlant() alone is a neutral carrier).  Its state is part of saveState() /
	// restoreState().
	struct ActuationChainInfo {
		int attached = 0, per_instance = 0, depth = 0;
		size_t state_bytes = 0;                // device bytes of taps, filt and primed
	};
	struct ActuationChainState {
		std::vector<double> taps, filt;        // [dof][depth][B], [dof][3][B] { x_held, y_rate, y_lag }
		std::vector<int> primed;               // [dof][B]
	};
	// the [dof][3] table that changes nothing: rows { 0, +inf, 0 }
	std::vector<double> neutralActuationChainTable() {
		std::vector<double> t((size_t)_robot->dof() * SAIP_PLANT_CHAIN_WORDS, 0.0);
		for (size_t j = 0; j < (size_t)_robot->dof(); j++) t[j * SAIP_PLANT_CHAIN_WORDS + 1] = INFINITY;
		return t;
	}
	// table: [dof][3] rows { delay, rate_max, tau_lag }, or [dof][3][B] with per_instance; empty: neutral.  depth 0..SAIP_PLANT_CHAIN_MAX_DEPTH
	void attachActuationChain(const std::vector<double>& table, bool per_instance, int depth) {
		const size_t cols = per_instance ? (size_t)_robot->batchSize() : 1;
		if (!table.empty() && table.size() != (size_t)_robot->dof() * SAIP_PLANT_CHAIN_WORDS * cols)
			throw std::invalid_argument("attachActuationChain: expected a [dof][3] table, or [dof][3][B] per instance");
		check(saip_batch_plant_chain_attach(_batch, table.empty() ? nullptr : table.data(), per_instance ? 1 : 0, depth));
	}
	void detachActuationChain() { check(saip_batch_plant_chain_detach(_batch)); }
	ActuationChainInfo actuationChainInfo() {
		ActuationChainInfo i;
		check(saip_batch_plant_chain_info(_batch, &i.attached, &i.per_instance, &i.depth, &i.state_bytes));
		return i;
	}
	void setActuationChainTable(const std::vector<double>& table) {
		const ActuationChainInfo i = actuationChainInfo();
		if (table.size() != (size_t)_robot->dof() * SAIP_PLANT_CHAIN_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setActuationChainTable: the shape of the attached chain table expected");
		check(saip_batch_plant_chain_set_table_host(_batch, table.data()));
	}
	// the per-instance table drawn on the device between two [dof][3] tables; delay rounded and clamped after the draw
	void actuationChainRandomize(unsigned long long seed, long long round, const std::vector<double>& lo, const std::vector<double>& hi) {
		const size_t w = (size_t)_robot->dof() * SAIP_PLANT_CHAIN_WORDS;
		if (lo.size() != w || hi.size() != w) throw std::invalid_argument("actuationChainRandomize: expected [dof][3] bounds");
		check(saip_batch_plant_chain_randomize(_batch, seed, round, lo.data(), hi.data()));
	}
	// the next period primes the chain again (enqueued, no wait)
	void resetActuationChain() { check(saip_batch_plant_chain_reset(_batch)); }
	// for tests and debugging; waits for the stream
	ActuationChainState actuationChainState() {
		const ActuationChainInfo i = actuationChainInfo();
		const size_t n = _robot->dof(), B = _robot->batchSize();
		ActuationChainState s;
		s.taps.resize(n * i.depth * B);
		s.filt.resize(n * 3 * B);
		s.primed.resize(n * B);
		check(saip_batch_plant_chain_state_host(_batch, s.taps.empty() ? nullptr : s.taps.data(), s.filt.data(), s.primed.data()));
		return s;
	}
	// the state arrays, [rows][ld]: taps [dof][depth] rows (nullptr at depth 0), filt [dof][3] rows, primed [dof] rows
	void actuationChainStateDevice(double** taps, double** filt, int** primed) { check(saip_batch_plant_chain_state_device(_batch, taps, filt, primed)); }
	double* actuationChainTableDevice() { return saip_batch_plant_chain_table_device(_batch); }  // [dof][3] or [dof][3][ld]

	// ---- sensing model: offset, noise and quantisation between the resident simulator and what the controller reads of it (saip.h).
	// While attached, every control cycle, per-task entry and internal OTG reads the measured q, dq; the simulator, the recorder and the
	// model queries keep the true state.  The period counter of the noise advances once per integrate() and once per rollout period.
	struct SensingWrench {
		int task;                      // id of a motion-force task
		std::vector<double> table;     // [6][3] rows { off, res, sigma } per axis, F then M; [6][3][B] with per_instance
	};
	struct SensingInfo {
		int per_instance_joints = 0, n_wrench_tasks = 0, per_instance_wrenches = 0;
		long long period = 0;          // the period the next measurement belongs to
	};
	// joints: [dof][6] rows { q_off, q_res, q_sigma, dq_off, dq_res, dq_sigma }, or [dof][6][B] with per_instance; empty: neutral (zeros).
	// wrenches: up to SAIP_SENSE_MAX_WRENCH_TASKS
	void attachSensing(const std::vector<double>& joints = {}, const std::vector<SensingWrench>& wrenches = {}, bool per_instance = false,
					   unsigned long long seed = 0) {
		const size_t cols = per_instance ? (size_t)_robot->batchSize() : 1;
		if (!joints.empty() && joints.size() != (size_t)_robot->dof() * SAIP_SENSE_JOINT_WORDS * cols)
			throw std::invalid_argument("attachSensing: expected [dof][6] joints, or [dof][6][B] per instance");
		std::vector<int> tasks;
		std::vector<double> table(wrenches.size() * SAIP_SENSE_WRENCH_WORDS * cols);
		for (size_t k = 0; k < wrenches.size(); k++) {
			const SensingWrench& w = wrenches[k];
			if (w.table.size() != SAIP_SENSE_WRENCH_WORDS * cols) throw std::invalid_argument("attachSensing: expected [6][3] words per wrench, or [6][3][B] per instance");
			tasks.push_back(w.task);
			std::copy(w.table.begin(), w.table.end(), table.begin() + k * SAIP_SENSE_WRENCH_WORDS * cols);
		}
		check(saip_batch_sensing_attach(_batch, joints.empty() ? nullptr : joints.data(), per_instance ? 1 : 0, (int)wrenches.size(), tasks.data(), table.data(),
										per_instance ? 1 : 0, seed));
	}
	void detachSensing() { check(saip_batch_sensing_detach(_batch)); }
	SensingInfo sensingInfo() {
		SensingInfo i;
		check(saip_batch_sensing_info(_batch, &i.per_instance_joints, &i.n_wrench_tasks, &i.per_instance_wrenches, &i.period));
		return i;
	}
	void setSensingJoints(const std::vector<double>& joints) {
		const SensingInfo i = sensingInfo();
		if (joints.size() != (size_t)_robot->dof() * SAIP_SENSE_JOINT_WORDS * (i.per_instance_joints ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setSensingJoints: the shape of the attached joint table expected");
		check(saip_batch_sensing_set_joints_host(_batch, joints.data()));
	}
	void setSensingWrenches(const std::vector<double>& tables) {
		const SensingInfo i = sensingInfo();
		if (tables.size() != (size_t)i.n_wrench_tasks * SAIP_SENSE_WRENCH_WORDS * (i.per_instance_wrenches ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setSensingWrenches: the shape of the attached wrench tables expected");
		check(saip_batch_sensing_set_wrenches_host(_batch, tables.data()));
	}
	void setSensingSeed(unsigned long long seed) { check(saip_batch_sensing_seed(_batch, seed)); }
	// 0 <= period < 2^32; pair it with restoreState: the counter is not part of a snapshot
	void setSensingPeriod(long long period) { check(saip_batch_sensing_set_period(_batch, period)); }
	// per-instance tables drawn on the device, uniform between two batch-uniform tables ([dof][6], [S][6][3]); an empty pair leaves that table alone
	void sensingRandomize(unsigned long long seed, long long round, const std::vector<double>& joint_lo, const std::vector<double>& joint_hi,
						  const std::vector<double>& wrench_lo = {}, const std::vector<double>& wrench_hi = {}) {
		const SensingInfo i = sensingInfo();
		const size_t jw = (size_t)_robot->dof() * SAIP_SENSE_JOINT_WORDS, ww = (size_t)i.n_wrench_tasks * SAIP_SENSE_WRENCH_WORDS;
		if ((!joint_lo.empty() || !joint_hi.empty()) && (joint_lo.size() != jw || joint_hi.size() != jw))
			throw std::invalid_argument("sensingRandomize: expected [dof][6] joint bounds");
		if ((!wrench_lo.empty() || !wrench_hi.empty()) && (wrench_lo.size() != ww || wrench_hi.size() != ww))
			throw std::invalid_argument("sensingRandomize: expected [S][6][3] wrench bounds");
		check(saip_batch_sensing_randomize(_batch, seed, round, joint_lo.empty() ? nullptr : joint_lo.data(), joint_hi.empty() ? nullptr : joint_hi.data(),
										   wrench_lo.empty() ? nullptr : wrench_lo.data(), wrench_hi.empty() ? nullptr : wrench_hi.data()));
	}
	// enqueue the measurement of the resident q, dq now (a host-driven loop's first step; needed after writes through device pointers)
	void measureState() { check(saip_batch_sensing_measure(_batch)); }
	// q_meas and dq_meas, [dof][B] each: what the controller last read; waits for the stream
	void measuredState(std::vector<double>& q, std::vector<double>& dq) {
		q.resize((size_t)_robot->dof() * _robot->batchSize());
		dq.resize(q.size());
		check(saip_batch_sensing_measured_host(_batch, q.data(), dq.data()));
	}
	double* sensingJointsDevice() { return saip_batch_sensing_joints_device(_batch); }      // [dof][6] or [dof][6][ld]
	double* sensingWrenchesDevice() { return saip_batch_sensing_wrenches_device(_batch); }  // [S][6][3] or [S][6][3][ld]; nullptr without wrench tasks
	double* measuredQDevice() { return saip_batch_sensing_measured_q_device(_batch); }      // [dof][ld]
	double* measuredDqDevice() { return saip_batch_sensing_measured_dq_device(_batch); }    // [dof][ld]

	// ---- sensing chain: per joint a delay line, an optional finite-difference velocity and a first-order low-pass behind the sensing model
	// (saip.h).  Needs an attached sensing model (attachSensing() alone is a neutral carrier).  Its state is part of saveState() / restoreState().
	struct SensingChainInfo {
		int attached = 0, per_instance = 0, depth = 0;
		double sample_time = 0;
		size_t state_bytes = 0;                // device bytes of taps, filt and primed
	};
	struct SensingChainState {
		std::vector<double> taps, filt;        // [dof][2][depth][B], [dof][3][B] { q_prev, y_q, y_dq }
		std::vector<int> primed;               // [dof][B]
	};
	// the low-pass coefficient of a first-order filter with cutoff f_c (Hz) sampled every sample_time seconds: for the a_q / a_dq words
	static double sensingChainAlpha(double cutoff_hz, double sample_time) { return 1.0 - std::exp(-2.0 * M_PI * cutoff_hz * sample_time); }
	// table: [dof][4] rows { delay, vel_mode, a_q, a_dq }, or [dof][4][B] with per_instance; empty: neutral.  depth 0..SAIP_SENSE_CHAIN_MAX_DEPTH
	void attachSensingChain(const std::vector<double>& table, bool per_instance, int depth, double sample_time) {
		const size_t cols = per_instance ? (size_t)_robot->batchSize() : 1;
		if (!table.empty() && table.size() != (size_t)_robot->dof() * SAIP_SENSE_CHAIN_WORDS * cols)
			throw std::invalid_argument("attachSensingChain: expected a [dof][4] table, or [dof][4][B] per instance");
		check(saip_batch_sensing_chain_attach(_batch, table.empty() ? nullptr : table.data(), per_instance ? 1 : 0, depth, sample_time));
	}
	void detachSensingChain() { check(saip_batch_sensing_chain_detach(_batch)); }
	SensingChainInfo sensingChainInfo() {
		SensingChainInfo i;
		check(saip_batch_sensing_chain_info(_batch, &i.attached, &i.per_instance, &i.depth, &i.sample_time, &i.state_bytes));
		return i;
	}
	void setSensingChainTable(const std::vector<double>& table) {
		const SensingChainInfo i = sensingChainInfo();
		if (table.size() != (size_t)_robot->dof() * SAIP_SENSE_CHAIN_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setSensingChainTable: the shape of the attached chain table expected");
		check(saip_batch_sensing_chain_set_table_host(_batch, table.data()));
	}
	// the per-instance table drawn on the device between two [dof][4] tables; delay and vel_mode rounded and clamped after the draw
	void sensingChainRandomize(unsigned long long seed, long long round, const std::vector<double>& lo, const std::vector<double>& hi) {
		const size_t w = (size_t)_robot->dof() * SAIP_SENSE_CHAIN_WORDS;
		if (lo.size() != w || hi.size() != w) throw std::invalid_argument("sensingChainRandomize: expected [dof][4] bounds");
		check(saip_batch_sensing_chain_randomize(_batch, seed, round, lo.data(), hi.data()));
	}
	// the next sample primes the chain again (enqueued, no wait)
	void resetSensingChain() { check(saip_batch_sensing_chain_reset(_batch)); }
	// for tests and debugging; waits for the stream
	SensingChainState sensingChainState() {
		const SensingChainInfo i = sensingChainInfo();
		const size_t n = _robot->dof(), B = _robot->batchSize();
		SensingChainState s;
		s.taps.resize(n * 2 * i.depth * B);
		s.filt.resize(n * 3 * B);
		s.primed.resize(n * B);
		check(saip_batch_sensing_chain_state_host(_batch, s.taps.empty() ? nullptr : s.taps.data(), s.filt.data(), s.primed.data()));
		return s;
	}
	// the state arrays, [rows][ld]: taps [dof][2][depth] rows (nullptr at depth 0), filt [dof][3] rows, primed [dof] rows
	void sensingChainStateDevice(double** taps, double** filt, int** primed) { check(saip_batch_sensing_chain_state_device(_batch, taps, filt, primed)); }
	double* sensingChainTableDevice() { return saip_batch_sensing_chain_table_device(_batch); }  // [dof][4] or [dof][4][ld]

	// ---- plant inertia: the masses, centres of mass and inertias the resident integrator reads in place of the model's (saip.h).  While
	// attached, integrate() and rolloutAsync() integrate with the table; everything the controller computes keeps the model.
	struct InertiaInfo {
		int per_instance = 0, n_payloads = 0;
		std::vector<int> payload_bodies;       // the movable body of every payload site
		std::vector<double> payload_frames;    // [P][12]: position (3) and rotation (9, row-major) of every site link in that body
	};
	// rows: [dof][10] of { m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz }, or [dof][10][B] with per_instance; empty: the model's own rows.
	// payload_links: up to SAIP_INERTIA_MAX_PAYLOADS sites of the payloads of setInertiaParts() / randomizeInertia()
	void attachInertia(const std::vector<double>& rows = {}, bool per_instance = false, const std::vector<std::string>& payload_links = {}) {
		const size_t cols = per_instance ? (size_t)_robot->batchSize() : 1;
		if (!rows.empty() && rows.size() != (size_t)_robot->dof() * SAIP_INERTIA_ROW_WORDS * cols)
			throw std::invalid_argument("attachInertia: expected [dof][10] rows, or [dof][10][B] per instance");
		std::vector<int> links;
		for (const std::string& l : payload_links) {
			links.push_back(_robot->linkIndex(l));
			if (links.back() < 0) throw std::invalid_argument("attachInertia: unknown link [" + l + "]");
		}
		check(saip_batch_inertia_attach(_batch, rows.empty() ? nullptr : rows.data(), per_instance ? 1 : 0, (int)links.size(), links.data()));
	}
	void detachInertia() { check(saip_batch_inertia_detach(_batch)); }
	InertiaInfo inertiaInfo() {
		InertiaInfo i;
		int bodies[SAIP_INERTIA_MAX_PAYLOADS] = {};
		double frames[SAIP_INERTIA_MAX_PAYLOADS * 12] = {};
		check(saip_batch_inertia_info(_batch, &i.per_instance, &i.n_payloads, bodies, frames));
		i.payload_bodies.assign(bodies, bodies + i.n_payloads);
		i.payload_frames.assign(frames, frames + 12 * i.n_payloads);
		return i;
	}
	void setInertiaRows(const std::vector<double>& rows) {
		const InertiaInfo i = inertiaInfo();
		if (rows.size() != (size_t)_robot->dof() * SAIP_INERTIA_ROW_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1))
			throw std::invalid_argument("setInertiaRows: the shape of the attached table expected");
		check(saip_batch_inertia_set_rows_host(_batch, rows.data()));
	}
	// the table composed on the device from scaled links plus payloads.  bodies: [dof][4] of { s, dx, dy, dz } or [dof][4][B]; empty: { 1, 0, 0, 0 }.
	// payloads: [P][7] of { m_p, c_p[3], hx, hy, hz } or [P][7][B]; empty: no mass
	void setInertiaParts(const std::vector<double>& bodies, const std::vector<double>& payloads = {}) {
		const InertiaInfo i = inertiaInfo();
		const size_t B = (size_t)_robot->batchSize(), nb = (size_t)_robot->dof() * SAIP_INERTIA_BODY_WORDS, np = (size_t)i.n_payloads * SAIP_INERTIA_PAYLOAD_WORDS;
		if (!bodies.empty() && bodies.size() != nb && bodies.size() != nb * B) throw std::invalid_argument("setInertiaParts: expected [dof][4] bodies, or [dof][4][B]");
		if (!payloads.empty() && payloads.size() != np && payloads.size() != np * B) throw std::invalid_argument("setInertiaParts: expected [P][7] payloads, or [P][7][B]");
		check(saip_batch_inertia_set_parts_host(_batch, bodies.empty() ? nullptr : bodies.data(), B > 1 && bodies.size() == nb * B ? 1 : 0,
												payloads.empty() ? nullptr : payloads.data(), B > 1 && payloads.size() == np * B ? 1 : 0));
	}
	// the parts of every instance drawn on the device, uniform between two batch-uniform tables ([dof][4], [P][7]), and composed; an empty
	// pair stands for the neutral words
	void randomizeInertia(unsigned long long seed, long long round, const std::vector<double>& body_lo, const std::vector<double>& body_hi,
						  const std::vector<double>& payload_lo = {}, const std::vector<double>& payload_hi = {}) {
		const InertiaInfo i = inertiaInfo();
		const size_t nb = (size_t)_robot->dof() * SAIP_INERTIA_BODY_WORDS, np = (size_t)i.n_payloads * SAIP_INERTIA_PAYLOAD_WORDS;
		if ((!body_lo.empty() || !body_hi.empty()) && (body_lo.size() != nb || body_hi.size() != nb))
			throw std::invalid_argument("randomizeInertia: expected [dof][4] body bounds");
		if ((!payload_lo.empty() || !payload_hi.empty()) && (payload_lo.size() != np || payload_hi.size() != np))
			throw std::invalid_argument("randomizeInertia: expected [P][7] payload bounds");
		check(saip_batch_inertia_randomize(_batch, seed, round, body_lo.empty() ? nullptr : body_lo.data(), body_hi.empty() ? nullptr : body_hi.data(),
										   payload_lo.empty() ? nullptr : payload_lo.data(), payload_hi.empty() ? nullptr : payload_hi.data()));
	}
	// the resident table read back: [dof][10], or [dof][10][B] when attached per instance; waits for the stream
	std::vector<double> inertiaRows() {
		const InertiaInfo i = inertiaInfo();
		std::vector<double> out((size_t)_robot->dof() * SAIP_INERTIA_ROW_WORDS * (i.per_instance ? (size_t)_robot->batchSize() : 1));
		check(saip_batch_inertia_rows_host(_batch, out.data()));
		return out;
	}
	double* inertiaRowsDevice() { return saip_batch_inertia_rows_device(_batch); }      // [dof][10] or [dof][10][ld]; nullptr when detached

private:
	void restored(saip_status st) {
		check(st);
		for (auto& a : _robot->_attached)
			if (a.batch == _batch) a.pushed = _robot->_version;  // the device holds the restored state, not the SaiModel mirror (pullState reads it back)
	}
	template <typename T>
	std::shared_ptr<T> byName(const std::string& name, TaskType type, const char* what) {
		for (auto& t : _tasks)
			if (t->getTaskName() == name) {
				if (t->getTaskType() != type)
					throw std::invalid_argument("Task " + name + " is not a " + what + ", and cannot be casted as such in RobotController::GetTaskByName");
				return std::dynamic_pointer_cast<T>(t);
			}
		throw std::invalid_argument("Task " + name + " not found in RobotController::GetTaskByName");
	}
	std::shared_ptr<SaiModel> _robot;
	std::vector<std::shared_ptr<TemplateTask>> _tasks;
	std::vector<std::string> _task_names;
	std::vector<uint8_t> _status;
	saip_batch* _batch = nullptr;
};

}  // namespace SaiPrimitivesBatched
