// What the engine's host units (saip_engine*.cpp) share: the kernel launchers they call, the model and batch structs behind the opaque
// handles of include/saip.h, and the helpers that cross a unit boundary (namespace saip::eng, so that the shared object exports them
// as mangled names only).  Host-only; included by those units and by nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/saip.h"
#include "saip_device.h"
#include "saip_cycle_plan.h"
#include "saip_period_plan.h"
#include "saip_state_snapshot.h"
#include "saip_sampler.h"
#include "saip_contact.h"
#include "saip_contact_patch.h"
#include "saip_clearance.h"
#include "saip_link_contact.h"
#include "saip_link_object.h"
#include "saip_env_schedule.h"
#include "saip_plant.h"
#include "saip_plant_chain.h"
#include "saip_inertia.h"
#include "saip_sense.h"
#include "saip_sense_chain.h"
#include "saip_guard.h"

namespace saip {
hipError_t launch_cycle_wg(const CycleParams& P, bool tree, hipStream_t stream);
hipError_t launch_cycle_wg_list(const CycleParams& P, hipStream_t stream);
hipError_t launch_reinit(const CycleParams& P, bool tree, hipStream_t stream);
hipError_t launch_cycle_lane(const CycleParams& P, hipStream_t stream, bool* supported);
hipError_t launch_cycle_oct(const CycleParams& P, hipStream_t stream);
hipError_t launch_cycle_wave(const CycleParams& P, hipStream_t stream);
hipError_t launch_cycle_octjf(const CycleParams& P, hipStream_t stream);
hipError_t launch_pose(const CycleParams& P, int task, double* out, bool tree, hipStream_t stream);
hipError_t launch_task_diag(const CycleParams& P, int task, const double* goal, const double* desired, int gcomps, double* out, bool tree, hipStream_t stream);
hipError_t launch_model_frames(const saip::FrameQuery& Q, bool tree, hipStream_t stream);
hipError_t launch_model_dynamics(const saip::DynQuery& Q, bool tree, hipStream_t stream);
hipError_t launch_otg_joints(const OtgDev& O, int B, int ld, int mode, hipStream_t stream);
hipError_t launch_otg_cartesian(const OtgDev& O, int B, int ld, int mode, bool tree, hipStream_t stream);
hipError_t launch_otg_pair(const OtgDev& Oc, const OtgDev& Oj, int B, int ld, hipStream_t stream);
hipError_t launch_integrate_otg_pair(const SimParams& S, const OtgDev& Oc, const OtgDev& Oj, int B, int ld, hipStream_t stream);
int otg_state_fields();
hipError_t launch_integrate(const SimParams& S, bool tree, hipStream_t stream);
hipError_t launch_rollout_record(const RecordParams& P, bool tree, hipStream_t stream);
hipError_t launch_goal_schedule(const ScheduleParams& P, hipStream_t stream);
hipError_t launch_state_gather(const SnapSeg* table, const int* unit_seg, int units, int B, const int* map, int save, hipStream_t stream);
hipError_t launch_sampler_perturb(const SamplerParams& P, hipStream_t stream);
hipError_t launch_sampler_cost(const SamplerCostParams& P, hipStream_t stream);
hipError_t launch_sampler_update(const SamplerParams& P, const double* cost, double temperature, double* w, SamplerResult* res, int* best_map, hipStream_t stream);
hipError_t launch_sampler_update_grouped(const SamplerParams& P, const double* cost, int risk, int tail, double* group, double temperature, double* w, SamplerResult* res,
										 int* best_map, hipStream_t stream);
hipError_t launch_sampler_share_columns(double* a, int rows, int B, int ld, int C, hipStream_t stream);
hipError_t launch_sampler_shift(const SamplerParams& P, int n, hipStream_t stream);
hipError_t launch_contact_apply(const ContactParams& P, bool tree, hipStream_t stream);
hipError_t launch_contact_patch_apply(const ContactPatchParams& P, bool tree, hipStream_t stream);
hipError_t launch_contact_apply_moving(const ContactMovingParams& P, bool tree, hipStream_t stream);
hipError_t launch_contact_patch_apply_moving(const ContactPatchMovingParams& P, bool tree, hipStream_t stream);
hipError_t launch_env_schedule(const EnvScheduleParams& P, hipStream_t stream);
hipError_t launch_clearance_eval(const ClearanceParams& P, bool tree, hipStream_t stream);
hipError_t launch_clearance_add_cost(int B, int ld, const double* summary, double* cost, double w_penalty, double w_collision, double d_safe, hipStream_t stream);
hipError_t launch_clearance_summary_reset(int B, int ld, double* summary, hipStream_t stream);
hipError_t launch_link_contact_apply(const LinkContactParams& P, bool tree, hipStream_t stream);
hipError_t launch_link_contact_summary_reset(int B, int ld, double* summary, hipStream_t stream);
hipError_t launch_link_contact_add_cost(int B, int ld, const double* summary, double* cost, double w_impulse, double w_peak, hipStream_t stream);
hipError_t launch_link_object_apply(const LinkObjectParams& Q, bool tree, hipStream_t stream);
hipError_t launch_link_object_add_cost(int B, int ld, const double* state, double* cost, const double* tp, double w_pos, const double* tq, double w_ori, hipStream_t stream);
hipError_t launch_plant_apply(const PlantParams& P, bool tree, hipStream_t stream);
hipError_t launch_plant_randomize(const PlantRandomParams& P, hipStream_t stream);
hipError_t launch_plant_chain_apply(const PlantChainParams& C, bool tree, hipStream_t stream);
hipError_t launch_plant_chain_randomize(const PlantChainRandomParams& P, hipStream_t stream);
hipError_t launch_inertia_compose(const InertiaComposeParams& P, hipStream_t stream);
hipError_t launch_sense_apply(const SenseParams& P, hipStream_t stream);
hipError_t launch_sense_randomize(const SenseRandomParams& P, hipStream_t stream);
hipError_t launch_sense_chain_apply(const SenseChainParams& C, hipStream_t stream);
hipError_t launch_sense_chain_randomize(const SenseChainRandomParams& P, hipStream_t stream);
hipError_t launch_guard_apply(const GuardParams& P, bool tree, hipStream_t stream);
hipError_t launch_guard_reset(const GuardParams& P, hipStream_t stream);
hipError_t launch_guard_add_cost(int B, const int* entry_row, double* cost, double w_time, double w_miss, hipStream_t stream);
}  // namespace saip

using saip::CycleParams;
using saip::ModelDev;
using saip::OtgDev;
using saip::SimParams;
using saip::TaskDev;
#define HIP_TRY(expr)                                                                                        \
	do {                                                                                                     \
		hipError_t e_ = (expr);                                                                              \
		if (e_ != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

// ------------------------------------------------------------------ model
struct LinkInfo {
	std::string name;
	int body;        // movable body this link is rigidly attached to (-1: attached to the fixed base)
	double R[9], p[3];  // link frame in the body frame
};
struct saip_model {
	int n = 0;
	std::vector<LinkInfo> links;
	ModelDev dev;
	double q_lower[SAIP_MAXN], q_upper[SAIP_MAXN], vel[SAIP_MAXN], effort[SAIP_MAXN];
};

// ------------------------------------------------------------------ batch
struct TaskHost {
	std::string name;
	TaskDev dev;
	double P[36];
	bool otg_enabled = true;  // reference default (MotionForceTask.h:67, JointTask.h:38)
	// internal OTG of a joint task (saip_otg.hip): acceleration-limited, defaults JointTask.h:39-41
	bool otg_alloc = false, otg_inited = false, otg_limits_dirty = true;
	OtgDev otg;
	double otg_limits[3 * SAIP_MAXN];  // max velocity, max acceleration, max jerk per task dof (the jerk row only in jerk-limited mode)
	double* otg_limits_dev = nullptr;
	double* desired_dev = nullptr;
	bool vel_sat = false;
	bool full_joint = false;
	double* goal_dev = nullptr;
	double* integ_dev = nullptr;
	double* integ_new_dev = nullptr;
	double* diag_dev = nullptr;
	int integ_rows = 0;
	// per-task entry points (TemplateTask::updateTaskModel(N_prec) / computeTorques): the N_prec the task was last updated with, its
	// nullspaces N and N N_prec, its own torques and status; allocated on first use
	double *nprec_dev = nullptr, *ntask_dev = nullptr, *ntot_dev = nullptr, *ttau_dev = nullptr, *tprec_dev = nullptr;
	uint8_t* tstatus_dev = nullptr;
	bool nprec_identity = true;
	long model_epoch = -1;  // state epoch of the last updateTaskModel (-1: never)
	int sh_cycle = 0;       // how many times this task's model has been updated (CycleParams::task_cycle; ShState::last_cycle)
};
struct saip_snapshot;
struct saip_batch {
	const saip_model* model = nullptr;
	int B = 0, ld = 0, device = -1;
	bool finalized = false, models_valid = false, config_dirty = true, state_pushed = false;
	bool gravity_comp = false, torque_sat = false, integ_always = false, jla = false;
	KernelChoice kernel_choice = KernelChoice::Auto;
	std::string kernel_name = "none";
	std::vector<TaskHost> tasks;
	hipStream_t stream = nullptr;
	double *q = nullptr, *dq = nullptr, *tau = nullptr, *tau_bound = nullptr;
	uint8_t* status = nullptr;
	ModelDev* model_dev = nullptr;
	TaskDev* tasks_dev = nullptr;
	std::vector<void*> allocs;
	double* pose_dev = nullptr;              // [12][ld] scratch of saip_batch_get_current_pose_host
	double* task_diag_dev = nullptr;         // [24][ld] scratch of saip_batch_get_task_diagnostics_host
	bool model_only = false;                 // saip_batch_finalize_model_only: no tasks, state and model queries only
	double base_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base_p[3] = {0, 0, 0};  // saip_batch_set_robot_base (T_world_robot)
	double* query_dev = nullptr;             // scratch of the _host model queries, query_rows x ld
	size_t query_rows = 0;
	long state_epoch = 0;                    // bumped whenever the resident state changes (per-task models become stale)
	double* diag_tau = nullptr;              // scratch torques / status of diagnostic launches (the last cycle's results stay intact)
	uint8_t* diag_status = nullptr;
	hipEvent_t sync_event = nullptr;         // saip_batch_wait_for
	hipEvent_t time_ev[2] = {nullptr, nullptr};  // saip_batch_time_steps (created once: event creation is not part of a timed region)
	bool flag_nan = false;                   // saip_batch_set_flagged_torque_policy
	bool flagged_on_list = false;            // saip_batch_set_flagged_recompute: eight-lane kernels hand flagged instances to the list launch instead of their slow tail
	FlagList flags;                          // the device-side work list of the slow path
	bool otg_prelaunched = false;            // rollouts: the paired OTG step of the coming cycle already ran, fused with the previous integrate
	// saip_batch_rollout_recorder_attach: the observer of the rollout periods (saip_rollout_record.hip).  Its arrays are its own (freed by
	// _detach), not part of `allocs`.
	struct Recorder {
		bool attached = false;
		int capacity = 0, stride = 1, task = -1, rows = 0;
		unsigned channels = 0;
		long long period = 0;                // recorded periods so far: the global period counter p
		double* log = nullptr;               // [capacity][rows][ld], a ring over the samples (nullptr: empty channel mask)
		uint8_t* status_log = nullptr;       // [capacity][ld]
		double* summary = nullptr;           // [8][ld] (nullptr: summaries off)
	} rec;
	// saip_batch_goal_schedule_attach: time-varying goals of the rollout periods (saip_goal_schedule.hip), at most one per task.  The
	// keyframes are the schedule's own allocation (freed by _detach), not part of `allocs`.
	struct Schedule {
		bool attached = false;
		int first = 0, count = 0, K = 0, stride = 1, mode = 0, per_instance = 0, rot = 0;
		double* key = nullptr;               // [K][count][ld] (per instance) or [K][count] (batch-uniform)
	};
	std::vector<Schedule> sched;             // one slot per task once a schedule has been attached
	int n_sched = 0;                         // attached schedules
	long long sched_period = 0;              // rollout periods since the last attach / rewind: the counter c every schedule shares
	std::vector<saip_snapshot*> snapshots;   // saip_batch_snapshot_create: the live snapshots of this batch (their device memory goes with the batch)
	// saip_batch_sampler_attach: the resident rollout sampler (saip_sampler.hip), at most one per scheduled task.  It rewrites the task's
	// resident keyframes in place around a nominal plan; cost, weights, result and best map are the batch's, allocated by the first
	// attach and freed by the last detach.
	struct Sampler {
		bool attached = false;
		int d = 0, rot = 0, r_rot = 0, exempt = 0;
		double* nominal = nullptr;           // device: [K][count] the nominal plan, then [d] sigma
	};
	std::vector<Sampler> samp;               // one slot per task once a sampler has been attached
	int n_samp = 0;
	unsigned long long samp_seed = 0;
	long long samp_round = 0;
	double* samp_cost = nullptr;             // [ld]
	double* samp_w = nullptr;                // [ld] softmin weights of the last update
	int* samp_best_map = nullptr;            // [ld]
	saip::SamplerResult* samp_result = nullptr;
	// saip_batch_sampler_set_scenarios: B = C M instances are M scenario blocks of C candidates (instance i = s C + c); M = 1 is the
	// ungrouped sampler.  Back to M = 1 when the last sampler is detached.
	int samp_scenarios = 1, samp_risk = 0, samp_tail = 0;
	double* samp_group = nullptr;            // [ld] group cost of the last grouped update, columns 0 .. C - 1
	// saip_batch_contact_attach: contact planes and the simulated force sensor of the resident simulator (saip_contact.hip), at most one
	// per batch.  Its arrays are configuration, scratch and readout: its own (freed by _detach), not part of `allocs` or of a snapshot.
	struct Contact {
		bool attached = false;
		int task = -1, n_planes = 0, per_instance = 0, sensor = 0;
		double rc[3] = {0, 0, 0};
		double* planes = nullptr;            // [P][8] (batch-uniform) or [P][8][ld]
		double* tau_sim = nullptr;           // [n][ld] commanded + contact torques of the substep being integrated
		double* readout = nullptr;           // [8][ld]
		double* summary = nullptr;           // [4][ld]
	} contact;
	// saip_batch_contact_patch_attach: contact patches (saip_contact_patch.hip), at most saip::PATCH_MAX per batch, on different motion-force
	// tasks, in the order they were attached (a detach closes the gap).  Never together with `contact`.  Their arrays are their own, like
	// those of `contact`; tau_sim is shared by the patches.
	struct ContactPatch {
		int task = -1, n_points = 0, n_planes = 0, per_instance = 0, sensor = 0;
		double r[saip::PATCH_MAX_POINTS][3] = {};
		double* planes = nullptr;            // [P][8] (batch-uniform) or [P][8][ld]
		double* readout = nullptr;           // [20][ld]
		double* summary = nullptr;           // [6][ld]
	} patch[saip::PATCH_MAX];
	int n_patch = 0;
	double* patch_tau_sim = nullptr;         // [n][ld], while n_patch > 0
	// saip_batch_clearance_attach: link spheres against obstacles and each other (saip_clearance.hip), at most one per batch.  Its arrays
	// are configuration, scratch and readout: its own (freed by _detach), not part of `allocs` or of a snapshot.
	struct Clearance {
		bool attached = false;
		int per_instance = 0, keep_centres = 0;
		double margin = 0;
		long long period = 0;                // monitored periods since the last _summary_reset
		saip::ClearanceGeom geom;            // the host copy of *geom_dev (zeroed by _attach)
		saip::ClearanceGeom* geom_dev = nullptr;
		double* obst = nullptr;              // [O][8] (batch-uniform) or [O][8][ld]
		double* readout = nullptr;           // [8][ld]
		double* summary = nullptr;           // [4][ld]
		double* centres = nullptr;           // [3 S][ld], keep_centres only
	} clearance;
	// saip_batch_link_contact_attach: obstacles push back on link spheres (saip_link_contact.hip), at most one per batch, in front of every
	// integration substep.  Nothing in it is state: its arrays are configuration, scratch, readout and summaries, its own copies (it does not
	// alias the clearance monitor's tables), freed by _detach, not part of `allocs` or of a snapshot.
	struct LinkContact {
		bool attached = false;
		int per_instance = 0, keep = 0;
		saip::LinkContactGeom geom;          // the host copy of *geom_dev (zeroed by _attach)
		saip::LinkContactGeom* geom_dev = nullptr;
		double* obst = nullptr;              // [O][8] (batch-uniform) or [O][8][ld]
		double* mat = nullptr;               // [O][4]
		double* tau_sim = nullptr;           // [n][ld] commanded (or actuated) + link-contact torques of the substep being integrated
		double* readout = nullptr;           // [8][ld]
		double* summary = nullptr;           // [4][ld]
		double* keep_dev = nullptr;          // [9 S][ld], keep only
	} link_contact;
	// saip_batch_link_object_attach: the pushed object, the optional second stage of link contact (saip_link_object.h), at most one per
	// batch; detached with link contact.  `state` is state: on the snapshot directory while attached (segment link_object.state).  The other
	// arrays are configuration, readout and summaries, its own (freed by _detach), not part of `allocs`.
	struct LinkObject {
		bool attached = false;
		int per_instance = 0;                // of the inertial words
		saip::LinkObjectGeom geom;           // the host copy of *geom_dev (zeroed by _attach)
		saip::LinkObjectGeom* geom_dev = nullptr;
		double* inertial = nullptr;          // [4] (batch-uniform) or [4][ld]
		double* state = nullptr;             // [13][ld]
		double* readout = nullptr;           // [12][ld]
		double* summary = nullptr;           // [4][ld]
	} link_object;
	// saip_batch_env_schedule_attach: time-varying obstacle and plane tables of the rollout periods (saip_env_schedule.hip), at most one per
	// table.  Keyframes and plane velocities are the schedule's own allocations (freed by _detach, or with the attachment whose table it
	// writes), not part of `allocs` or of a snapshot: tables are configuration.
	struct EnvSchedule {
		bool attached = false;
		int target = 0, task = -1, first = 0, n_items = 0, K = 0, stride = 1, mode = 0, per_instance = 0;
		double* key = nullptr;               // [K][n_items][W] or [K][n_items][W][ld]
		double* vel = nullptr;               // planes: [P][4] or [P][4][ld] over the whole table (zero outside the scheduled items)
	} env[saip::ENV_MAX_SCHEDULES];
	int n_env = 0;                           // attached environment schedules
	long long env_period = 0;                // the rollout period c the next scheduled period belongs to (_rewind sets it)
	// The optional second stage of the sensing model and of the plant model: per joint a delay line and filters, W words per joint (a
	// ChainKind below says which).  The only attachments with state: taps, filt and primed are on the snapshot directory while attached;
	// the table is configuration.  Nothing of a chain lives in a host scalar but the sensing chain's sample time, which its carrier keeps.
	struct Chain {
		bool attached = false;
		int per_instance = 0, depth = 0;
		double* table = nullptr;             // [n][W] (batch-uniform) or [n][W][ld]
		double* taps = nullptr;              // [n][tap_rows][depth][ld] (nullptr at depth 0)
		double* filt = nullptr;              // [n][filt_rows][ld]: q_prev, y_q, y_dq (sensing); x_held, y_rate, y_lag (actuation)
		int* primed = nullptr;               // [n][ld]
		double* bounds = nullptr;            // lo [n][W], hi of the chain's _randomize (per-instance table only)
	};
	// saip_batch_plant_attach: the plant model of the resident simulator (saip_plant.hip), at most one per batch: actuator limits, friction,
	// joint stops and external wrenches in front of every integration substep.  Nothing in it but the `chain` sub-block is state: its
	// arrays are configuration, scratch and summaries, its own (freed by _detach), not part of `allocs` or of a snapshot; `period` is a
	// host-side counter.
	struct Plant {
		bool attached = false;
		int per_instance_joints = 0, n_wrenches = 0, per_instance_wrenches = 0;
		long long period = 0;                // the period the next integration belongs to (wrench windows)
		saip::PlantSite site[saip::PLANT_MAX_WRENCHES] = {};
		double* joints = nullptr;            // [n][10] (batch-uniform) or [n][10][ld]
		double* wrenches = nullptr;          // [W][8] or [W][8][ld] (nullptr: no wrench)
		double* tau_act = nullptr;           // [n][ld] what the actuators, friction, stops and wrenches make of the commanded torques
		double* summary = nullptr;           // [4][ld]
		double* bounds = nullptr;            // joint lo [n][10], joint hi, wrench lo [W][8], wrench hi of saip_batch_plant_randomize (per-instance tables only)
		Chain chain;                         // saip_batch_plant_chain_attach: the actuation chain (saip_plant_chain.h), snapshot segments plant.chain.*
	} plant;
	// saip_batch_inertia_attach: the inertial parameters of the simulated robot (saip_inertia.hip), at most one per batch: the table the
	// resident integrator reads in place of the model's masses, centres of mass and inertias.  Configuration only: its arrays are its own
	// (freed by _detach), not part of `allocs` or of a snapshot.
	struct Inertia {
		bool attached = false;
		int per_instance = 0, n_payloads = 0;
		saip::InertiaSite site[saip::INERTIA_MAX_PAYLOADS] = {};
		double* rows = nullptr;              // [n][10] (batch-uniform) or [n][10][ld]
		double* parts = nullptr;             // staging of _set_parts_host: bodies [n][4] or [n][4][ld], then payloads [P][7] or [P][7][ld]
		double* bounds = nullptr;            // body lo [n][4], body hi, payload lo [P][7], payload hi of _randomize (per-instance tables only)
	} inertia;
	// saip_batch_sensing_attach: the sensing model of the resident simulator (saip_sense.hip), at most one per batch: offset, noise and
	// quantisation on what the controller reads of the state and of the simulated force sensor.  Nothing in it is state: its arrays are
	// configuration and a measured copy of q, dq, its own (freed by _detach), not part of `allocs` or of a snapshot; `period` is a
	// host-side counter, `epoch` the state_epoch the measured copy was last taken at (-1: stale whatever the state).
	struct Sensing {
		bool attached = false;
		int per_instance_joints = 0, n_wrench_tasks = 0, per_instance_wrenches = 0;
		int task[saip::SENSE_MAX_WRENCH_TASKS] = {-1, -1};
		unsigned long long seed = 0;
		long long period = 0;                // the period the next measurement belongs to (noise counter)
		long epoch = -1;
		double* joints = nullptr;            // [n][6] (batch-uniform) or [n][6][ld]
		double* wrenches = nullptr;          // [S][6][3] or [S][6][3][ld] (nullptr: no wrench task)
		double* q_meas = nullptr;            // [n][ld] what every non-diagnostic cycle, per-task and OTG launch reads in place of q
		double* dq_meas = nullptr;           // [n][ld]
		double* bounds = nullptr;            // joint lo [n][6], joint hi, wrench lo [S][18], wrench hi of saip_batch_sensing_randomize
		Chain chain;                         // saip_batch_sensing_chain_attach: the sensing chain (saip_sense_chain.hip), snapshot segments sense.chain.*
		double chain_sample_time = 0;        // what its finite-difference velocity divides by; 0 while no chain is attached
	} sensing;
	// saip_batch_guard_attach: event-triggered phases of the rollout periods (saip_guard.hip), at most one per batch, on one motion-force
	// task.  The tables are configuration and the readout is scratch; phase, since, clock, run, entry, fires and latch are state: on the
	// snapshot directory while attached (segments guard.*).  Nothing of it lives in a host scalar: the period counter `clock` is a
	// per-instance device word.  Its arrays are its own (freed by _detach), not part of `allocs`.
	struct Guard {
		bool attached = false;
		int task = -1, G = 0, P = 0, per_instance = 0;
		int need_guards = 0, need_phases = 0;  // GUARD_NEED_* bits of the guard table's signals and of the phase table's modes
		double* guards = nullptr;            // [G][8] (batch-uniform) or [G][8][ld]
		double* phases = nullptr;            // [P][4]
		int* ints = nullptr;                 // [3 + 2 G + P][ld]: phase, since, clock, run [G], entry [P], fires [G]
		double* latch = nullptr;             // [12][ld]
		double* readout = nullptr;           // [8][ld]
	} guard;
};

namespace saip {
saip_status fail_external(saip_status st, const char* fmt, ...);  // saip_engine.cpp: sets saip_last_error(); the name saip_comm.cpp declares
namespace eng {
inline constexpr auto& fail = fail_external;
// ---- saip_engine.cpp
inline bool has_device(const saip_batch* b) { return b->device >= 0; }
inline double* commanded_tau(const saip_batch* b) { return b->tau_bound ? b->tau_bound : b->tau; }  // the caller's bound buffer or the batch's own
// the state the controller reads: the measured copy while a sensing model is attached, else the resident state itself
inline const double* controller_q(const saip_batch* b) { return b->sensing.attached ? b->sensing.q_meas : b->q; }
inline const double* controller_dq(const saip_batch* b) { return b->sensing.attached ? b->sensing.dq_meas : b->dq; }
saip_status check_batch(const saip_batch* b, int task, const char* fn);
saip_status need_state(saip_batch* b, const char* fn);
saip_status need_ready(saip_batch* b, const char* fn);
saip_status need_controller(const saip_batch* b, const char* fn);
saip_status copy_h2d(saip_batch* b, double* dev, const double* host, int comps);
saip_status copy_d2h(saip_batch* b, double* host, const double* dev, int comps);
// a zeroed device array of the batch's arena (`allocs`: freed with the batch)
template <typename Tp>
saip_status dev_alloc(saip_batch* b, Tp** p, size_t count) {
	void* v = nullptr;
	HIP_TRY(hipMalloc(&v, count * sizeof(Tp)));
	HIP_TRY(hipMemset(v, 0, count * sizeof(Tp)));
	// the fill runs on the null stream and need not be done when the call returns; the batch's stream is non-blocking and does not wait for
	// it: without this a kernel launched on it right away (the first model query into a grown scratch) had its results zeroed now and then
	HIP_TRY(hipStreamSynchronize(nullptr));
	b->allocs.push_back(v);
	*p = (Tp*)v;
	return SAIP_OK;
}
saip_status upload_table(saip_batch* b, double* dev, const double* host, size_t rows, int per_instance, const char* what, const char* fn);
// the plumbing every attachment uses on arrays of its own (not part of `allocs`): count elements, zeroed on the batch's stream
template <typename Tp>
saip_status alloc_zero(saip_batch* b, Tp** p, size_t count) {
	HIP_TRY(hipMalloc((void**)p, count * sizeof(Tp)));
	const hipError_t e = hipMemsetAsync(*p, 0, count * sizeof(Tp), b->stream);
	if (e != hipSuccess) {
		(void)hipFree(*p);
		*p = nullptr;
		return fail(SAIP_ERR_DEVICE, "hipMemsetAsync failed: %s", hipGetErrorString(e));
	}
	return SAIP_OK;
}
// The two bound tables of a _randomize entry that draws per-instance tables between them.  The entries share the order: pairing, the
// attachment's own conditions, every pair checked, need_ready, every pair uploaded.
// ... either pair may be absent, but whole and not both
inline saip_status check_bound_pairs(const char* fn, const double* lo_a, const double* hi_a, const double* lo_b, const double* hi_b) {
	if ((lo_a == nullptr) != (hi_a == nullptr) || (lo_b == nullptr) != (hi_b == nullptr))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a lower table without its upper table (or the reverse)", fn);
	if (!lo_a && !lo_b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to draw: both pairs are null", fn);
	return SAIP_OK;
}
// ... both bounds pass the table's checker `bool check(const double* table, char* msg, size_t len)`
template <typename Check>
saip_status check_bound_pair(const char* fn, const double* lo, const double* hi, Check check) {
	char msg[200];
	for (const double* t : {lo, hi})
		if (!check(t, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s bound: %s", fn, t == lo ? "lower" : "upper", msg);
	return SAIP_OK;
}
// ... where a word may be infinite: the `words` words of one unit ("joint 3", "wrench 0") differ between the bounds only where both are finite
saip_status check_bound_infinities(const char* fn, const char* what, size_t unit, const double* lo, const double* hi, int words, const char* const* names);
// ... lo then hi, [rows] each, to dst
saip_status upload_bound_pair(saip_batch* b, double* dst, const double* lo, const double* hi, size_t rows, const char* fn);
saip_status rows_to_host(saip_batch* b, saip_status st, double* out, const double* dev, int rows, const char* fn);
saip_status zero_rows(saip_batch* b, double* dev, int rows);
saip_status ensure_lazy_state(saip_batch* b);
saip_status ensure_task_constants(saip_batch* b);
saip_status launch_cycle(saip_batch* b, bool diag, const SimRequest* sim = nullptr, bool* integrated = nullptr);
bool otg_pair_ready(saip_batch* b);
// ---- saip_engine_model.cpp
void m3_mul(const double* A, const double* B, double* C);
void m3_vec(const double* A, const double* v, double* o);
void m3_T(const double* A, double* B);
void m3_eye(double* A);
int range_basis_3(const double* dirs, int cnt, double* basis);
// ---- saip_engine_contact.cpp
inline bool contact_rows_overlap(int first, int count) { return first < 36 && first + count > 30; }  // the sensed-wrench rows of a goal block
void contact_free(saip_batch* b);
void patch_free(saip_batch* b, int slot);
saip_status contact_launch(saip_batch* b, int mode, double dt);
saip_status patch_launch(saip_batch* b, int mode, double dt);
bool patch_any_sensor(const saip_batch* b);
const char* contact_check_planes(const double* planes, int P, size_t cols, std::vector<double>& out);
// ---- saip_engine_env.cpp
int env_slot(const saip_batch* b, int target, int task);            // the schedule on that table (task: ENV_TARGET_PATCH only), -1: none
void env_release(saip_batch* b, int target, int task);              // ... freed, if there is one; the stream is idle
const double* env_plane_velocity(const saip_batch* b, int target, int task);  // nullptr: those planes have no schedule
saip_status env_apply(saip_batch* b, double T);
// ---- saip_engine_clearance.cpp
void clearance_free(saip_batch* b);
saip_status clearance_launch(saip_batch* b, int mode, double dt);
bool clearance_check_obstacles(const double* obst, int O, size_t cols, char* msg, size_t len);  // false: `msg` says what is wrong with which entry
// ---- saip_engine_link_contact.cpp
void link_contact_free(saip_batch* b);
saip_status link_contact_launch(saip_batch* b, int mode, double dt, const double* gravity = nullptr);  // gravity: of the substep (the pushed object's weight)
void link_object_free(saip_batch* b);
// ---- saip_engine_chain.cpp: the host side of a chain (saip_batch::Chain), written once.  What differs between the two is a ChainKind;
// the extern "C" entries stay with the carriers (saip_engine_sensing.cpp, saip_engine_plant.cpp), which pick the struct and the kind
struct ChainKind {
	int words, filt_rows, tap_rows, max_depth;  // words per joint; taps is [n][tap_rows][depth][ld]
	const char* const* names;                   // of the words
	const double* neutral;                      // the row a null table stands for
	const char *article, *noun, *entry;         // "a", "sensing chain", "saip_batch_sensing_chain": the messages' vocabulary
	const char *carrier, *carrier_hint;         // "sensing model", and what the attach entry says when it is missing
	const char* snapshot;                       // prefix of the snapshot segments
	bool scan_infinities;                       // _randomize refuses a word that is infinite in one bound only
	// one word that is not NaN: nullptr when fine, else what is wrong with it, rendered into buf.  bounds: the two tables of a draw, whose
	// integer words are rounded and clamped afterwards and only have to be finite
	const char* (*rule)(int k, double v, const char* name, int depth, bool bounds, char* buf, size_t len);
};
const ChainKind& sense_chain_kind();  // functions: a constant object with host function pointers would be emitted for the device as well
const ChainKind& plant_chain_kind();
using Chain = saip_batch::Chain;
void chain_free(Chain& H);
saip_status chain_need(const ChainKind& K, const Chain& H, const char* fn);  // behind the carrier's own need-check
saip_status chain_attach_depth(const ChainKind& K, const saip_batch* b, int depth, const char* fn);  // attach, first half: need_controller and the depth
saip_status chain_attach(const ChainKind& K, saip_batch* b, Chain& H, bool carrier_attached, const double* table, int per_instance, int depth, const char* fn);
saip_status chain_detach(saip_batch* b, Chain& H, const char* fn);
void chain_info(const ChainKind& K, const saip_batch* b, const Chain& H, int* attached, int* per_instance, int* depth, size_t* state_bytes);
saip_status chain_set_table(const ChainKind& K, saip_batch* b, Chain& H, const double* table, const char* fn);
saip_status chain_randomize_bounds(const ChainKind& K, saip_batch* b, Chain& H, const double* lo, const double* hi, const char* fn);  // all of _randomize but the launch
saip_status chain_reset(saip_batch* b, Chain& H, const char* fn);
saip_status chain_state_device(const Chain& H, double** taps, double** filt, int** primed);
saip_status chain_state_host(const ChainKind& K, saip_batch* b, const Chain& H, double* taps, double* filt, int* primed, const char* fn);
// ---- saip_engine_plant.cpp
void plant_free(saip_batch* b);
saip_status plant_launch(saip_batch* b, double dt, int substep);
// ---- saip_engine_inertia.cpp
void inertia_free(saip_batch* b);
// ---- saip_engine_sensing.cpp
void sensing_free(saip_batch* b);
int sensing_sensor_slots(const saip_batch* b, bool planes, bool patches);
saip_status sensing_launch(saip_batch* b, int mode, int slot_mask);
saip_status sensing_refresh(saip_batch* b);
// ---- saip_engine_guard.cpp
void guard_free(saip_batch* b);
saip_status guard_launch(saip_batch* b);
void guard_segments(const saip_batch* b, saip::GuardParams* P);  // where the state arrays live (the snapshot directory)
// ---- saip_engine_rollout.cpp
saip::SimPlan sim_plan(const saip_batch* b);                // plan_sim of the batch's attach flags, as they are now
double* tau_buffer(const saip_batch* b, saip::TauBuf which);  // the one place that knows which array a name of the torque chain is
void record_free(saip_batch* b);
void schedule_release(saip_batch* b, int task);
inline double sched_max_abs(const double* a, int n) {
	double m = 0;
	for (int i = 0; i < n; i++) m = std::fmax(m, std::fabs(a[i]));
	return m;
}
// LINEAR over the rotation rows: every keyframe orthonormal to 1e-6, consecutive keyframes less than pi - 1e-3 apart.  `at(k, r)`: row r
// (3..11 of the goal block) of keyframe k for the instance under test
template <typename At>
const char* sched_check_rotations(int K, At at) {
	double prev[9];
	for (int k = 0; k < K; k++) {
		double R[9], G[9];
		for (int e = 0; e < 9; e++) R[e] = at(k, e);
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) G[3 * i + j] = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0);
		if (!(sched_max_abs(G, 9) <= 1e-6)) return "a rotation keyframe is not orthonormal (max |R^T R - I| > 1e-6)";
		if (k > 0) {
			double M[9];
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) M[3 * i + j] = prev[i] * R[j] + prev[3 + i] * R[3 + j] + prev[6 + i] * R[6 + j];
			const double w[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};
			const double angle = std::atan2(std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), 0.5 * (M[0] + M[4] + M[8] - 1.0));
			if (!(angle <= M_PI - 1e-3)) return "two consecutive rotation keyframes are more than pi - 1e-3 rad apart (the geodesic is ill-defined)";
		}
		for (int e = 0; e < 9; e++) prev[e] = R[e];
	}
	return nullptr;
}
// ---- saip_engine_snapshot.cpp
void snapshot_release_device(saip_snapshot* s);
// ---- saip_engine_sampler.cpp
void sampler_release(saip_batch* b, int task);
}  // namespace eng
}  // namespace saip
using namespace saip::eng;
