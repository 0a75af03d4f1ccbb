// Device-visible constant blocks shared by the host engine and the HIP kernels.
// Layout notes: everything here is batch-uniform (wave-uniform), read through scalar loads.
#pragma once
#include <stdint.h>

#define SAIP_MAXN 32
#define SAIP_MAXT 8

namespace saip {

// everything the forward-kinematics loop needs about ONE joint/body, packed into four consecutive 64-byte lines so that the
// rolled loop of the lane kernel issues one burst of scalar loads per iteration (and a prewarm pass can touch all of it up front)
struct alignas(256) JointRec {
	double R0[9], p0[3], axis[3], com[3], inertia[6], mass;
	int jtype, axis_is_z, iso_inertia, pad_;
	double pad2_[5];
};
static_assert(sizeof(JointRec) == 256, "JointRec must be exactly four cache lines");

// the movable bodies of one robot (fixed links already merged on the host, saip_engine_model.cpp: saip_model_create_tree)
struct ModelDev {
	int n;
	int all_axis_z;              // every joint axis == (0,0,1) (the usual URDF convention): the eight-lane kernels build R0 Rz(q) from two columns
	int jtype[SAIP_MAXN];        // 1 revolute, 2 prismatic
	int axis_is_z[SAIP_MAXN];    // joint axis == (0,0,1) exactly: the joint rotation touches two columns only
	int iso_inertia[SAIP_MAXN];  // body inertia tensor = i * identity: invariant under rotation
	double R0[SAIP_MAXN][9];     // joint origin rotation (parent body frame -> joint frame at q=0), row-major
	double p0[SAIP_MAXN][3];     // joint origin translation in the parent body frame
	double axis[SAIP_MAXN][3];   // unit joint axis in the body frame
	double mass[SAIP_MAXN];
	double com[SAIP_MAXN][3];    // body frame
	double inertia[SAIP_MAXN][6];// about the COM, body axes: xx yy zz xy xz yz
	double effort[SAIP_MAXN];
	double q_lower[SAIP_MAXN], q_upper[SAIP_MAXN], vel_limit[SAIP_MAXN];  // jointLimits(), used by the joint-limit-avoidance wrap
	double gravity[3];
	double pad_align_[5];
	JointRec jrec[SAIP_MAXN];    // packed copy of the per-joint constants above (lane kernel FK loop)
	// Topology, read by the tree instantiations only (the serial ones compile to what they compiled to before these fields existed).
	// A model whose movable bodies form a chain after fixed-link merging has is_tree = 0 and runs the serial code everywhere.
	int is_tree;
	int parent[SAIP_MAXN];       // movable parent body (-1: the fixed base); parent[j] < j
	uint32_t anc[SAIP_MAXN];     // bit i set: body i is an ancestor of body j or j itself
	uint32_t desc[SAIP_MAXN];    // bit i set: body i is a descendant of body j or j itself
	int jump[5][SAIP_MAXN];      // the 2^r-th ancestor of body j (-1: none): pointer jumping of the general kernel's prefix-product FK
};

enum { TASK_JOINT = 2, TASK_MOTION_FORCE = 3 };

// SingularityHandler state of one instance of one motion-force task with the blended strategies on (SingularityHandler.h:226-243):
// entering posture, type-2 torque direction (bit i set = -1), type counters and their 200-cycle window.  Zero-initialised.
enum { SH_BUFFER = 200 };
struct ShState {
	double q_prior[SAIP_MAXN];
	unsigned dir_neg;
	int ntypes, c1, c2, head, size;
	int last_cycle;    // cycle number (CycleParams::task_cycle) of the last cycle this instance had singular directions: the counters and the
	                   // window above are void unless that was the previous cycle (SingularityHandler.cpp:238-244 clears them whenever a cycle
	                   // finds none) -- instances outside the singular region never have to touch their state
	unsigned char hist[SH_BUFFER];
};

enum { DEC_FULL = 0, DEC_BIE = 1, DEC_IMPEDANCE = 2 };

struct TaskDev {
	int type;
	int body;          // motion force: movable body the control frame is attached to
	int k;             // motion force: task rank = pos_range + ori_range
	int m;             // joint: rows of S
	int decoupling;
	int s_identity;    // joint: S == I
	int has_ki;        // any integral gain != 0
	int goal_comps;
	int bm_identity;   // motion force: Bm == I6 (full task)
	int sing_handling; // motion force: SingularityHandler::_enforce_handling_strategy (1 = reference default)
	int sing_strategies; // motion force: blended type-1 / type-2 strategies on the device (general kernel) instead of flagging
	int sh_force_type1;  // handleAllSingularitiesAsType1 (SingularityHandler.h:131)
	double dt, bie_threshold, s_min, s_max, s_abs_tol;
	double sh_kp1, sh_kv1, sh_kv2;  // setSingularityHandlingGains (SingularityHandler.h:119; defaults 50, 14, 5)
	double cert_kroot; // k^(-1/8): lower/upper bound ratio of the trace-power bound on lambda_max (singular-value certificate)
	double pos[3];     // control point in the body frame
	double rot[9];     // control frame rotation in the body frame
	double Bm[36];     // 6 x 6 row-major, first k columns = orthonormal basis of range(P)
	double Ppos[9], Pori[9];   // diagonal blocks of the partial task projection P
	double sig_p[9], sig_o[9]; // sigmaPosition / sigmaOrientation (force & moment space dimension 0)
	double kp_pos[3], kv_pos[3], ki_pos[3], kp_ori[3], kv_ori[3], ki_ori[3];
	double kp[SAIP_MAXN], kv[SAIP_MAXN], ki[SAIP_MAXN];
	// velocity saturation, force / moment spaces (open-loop force control): MotionForceTask.cpp:306-383, 416-430, 449-462, 892-971; JointTask.cpp:327-341
	int general_law;   // 0: defaults (no velocity saturation, force and moment space dimension 0) -> short control-law path
	int vel_sat, force_dim, moment_dim, param_in_compliant_frame;
	int law_identity;  // motion force: Bm, Ppos, Pori, sigmaPosition, sigmaOrientation are all EXACTLY the identity and the short control law applies (the
	                   // full 6-dof task without force / moment space: the reference default) -- set at upload; the wavefront kernel skips the products
	int pad1_[2];
	double lin_sat, ang_sat, kv_force, kv_moment;
	double force_axis[3], moment_axis[3];      // unit axes
	// closed-loop force / moment control (MotionForceTask.cpp:327-349, 357-378, 484-487), passivity controller off (POPC default)
	int cl_force, cl_moment;
	int popc_enabled, popc_cap;                // POPCExplicitForceControl around the force loop; capacity of the energy window ring
	double kp_force, ki_force, kp_moment, ki_moment, kff_force, kff_moment, max_force_fb, max_moment_fb;
	double Rcs[9], tcs[3];                     // _T_control_to_sensor (MotionForceTask.cpp:94, 802)
	double kvinv_pos[3], kvinv_ori[3];         // pseudo-inverse of the diagonal kv gains (computePseudoInverse)
	double kvinv[SAIP_MAXN], sat[SAIP_MAXN];   // joint task
	double S[SAIP_MAXN * SAIP_MAXN]; // m x n row-major
	double* goal;      // [goal_comps][ld]
	double* integ;     // [12 or m][ld]
	double* integ_new; // same shape: what this cycle's control law advanced the integrators to; committed to `integ` at the end of the
	                   // cycle unless the instance ends flagged (status 1) -- a flagged instance advances nothing, whichever kernel ran
	double* diag_N;    // optional [n*n][ld] task nullspace dump (diagnostic variant), else nullptr
	ShState* sh;       // [B] handler states when sing_strategies, else nullptr
	double* popc;      // [7 + popc_cap][ld] passivity observer state: PO, E_correction, Rc, sum |vcl|^2, counter, ring head, ring size, ring
};

struct CycleParams {
	int B, ld, n, nt;
	// rollouts without internal OTGs: the eight-lane kernel integrates the state under the torques it has just written (0 = off)
	int sim_substeps;
	double sim_dt, sim_damping, sim_gravity[3];
	int gravity_comp, torque_sat, integ_always, diag;
	int jla;           // RobotController::enableJointLimitAvoidance
	int only_flagged;  // general kernel as the slow path behind the lane kernel: workgroups whose instance has status 0 exit at once
	const double* q;   // [n][ld]
	const double* dq;  // [n][ld]
	double* tau;       // [n][ld]
	uint8_t* status;   // [ld]
	const ModelDev* model;
	const TaskDev* tasks;
	// lane-per-instance kernel only
	int mf_task[2];               // task ids of the (at most two) motion-force tasks, -1 when absent
	int rank_bound[SAIP_MAXT];    // batch-uniform upper bound on the rank of each task in the hierarchy
	int lane_task_is_joint[SAIP_MAXT];
	int lane_prefetch_ok;         // stack is {motion-force, full joint task}: the prefetch layout of the latency variant applies
	int wave_general_joint;       // wavefront kernel: some joint task needs a range basis (anything but one full joint task closing the hierarchy)
	int lane_general;             // some task needs the general control laws (velocity saturation / force or moment space)
	int oct_general_joint;        // eight-lane kernel, joint task: 0 rank <= 1 behind a 6-dof task, 1 Gram path (<= 4 rows), 2 full task behind a partial one
	int reinit_task, reinit_mask; // reinit kernel: task (-1 = all) and parts (1 linear/joint, 2 angular, 4 goal force+moment)
	int any_bie;
	int oct_partial_mf;           // eight-lane kernel: the motion-force task is partial (k < 6)
	int oct_truncate;             // eight-lane kernel: singularity handling disabled -> near-singular instances are reduced in the kernel
	double bie_thr;
	// per-task entry points of the general kernel (TemplateTask::updateTaskModel(N_prec) / computeTorques() / computeTorques(tau_prec),
	// TemplateTask.h:43-60): evaluate ONE task with a caller-supplied N_prec instead of walking the hierarchy
	int single_task;              // -1: the whole hierarchy (RobotController); >= 0: this task only, no RobotController post-processing
	int phase;                    // 0: model + torques fused; 1: model only (updateTaskModel: nullspaces out, handler classification state
	                              // advanced, no control law); 2: torques only (computeTorques: control law, integrators, no classification)
	const double* ext_nprec;      // [n*n][ld] row-major per instance, nullptr = identity
	const double* ext_tau_prec;   // [n][ld] torques of the previous tasks (disturbance compensation), nullptr = none
	double* out_N;                // [n*n][ld] task nullspace N (getTaskNullspace), optional
	double* out_Ntot;             // [n*n][ld] N N_prec (getTaskAndPreviousNullspace), optional
	int task_cycle[SAIP_MAXT];    // per task: how many times its model has been updated (SingularityHandler state: see ShState::last_cycle)
	int flag_nan;                 // torques of an instance that ends flagged (status 1): 0 = left as they were (the last valid torque is held), 1 = NaN
	// instances the lane / eight-lane kernel could not finish (status 1) are appended here; the general kernel launched behind as the
	// device-side slow path (a fixed grid striding over the list) recomputes them.  Two count / list pairs used alternately: the lane /
	// eight-lane kernel of a cycle appends to `flag_count` / `flag_list` and zeroes `flag_count_next` (whose readers -- the slow path of the
	// previous cycle -- are done by stream order), so an empty list costs the slow path one load per workgroup and no atomic at all
	int* flag_count;
	int* flag_list;
	int* flag_count_next;
	// eight-lane kernels: the wavefront that could not finish an instance recomputes it itself, right behind its epilogue, with the general
	// kernel's body on its own (by then dead) LDS block -- no list, no second launch (round 4; 0: flagged instances go to the list / stay flagged)
	int slow_tail;
	// eight-lane kernels: TaskDev::goal / ::integ of the stack's two tasks once more, as kernel arguments.  Read from the task block they are
	// a pointer chase at the very start of every wavefront -- kernel arguments, then the pointer, then the data: one memory round trip more
	// in front of the goals than in front of anything else the wavefront asks for.
	const double* goal2[2];
	double* integ2[2];
	// eight-lane kernels: the batch-uniform words of the model, of the stack's first motion-force task and of its first joint task that the
	// ordinary path reads behind its fences and LDS stores, once more, as kernel arguments (launch words).  Read from the model / task block there they are vector loads
	// of a uniform word at the point of use -- the compiler can no longer prove the blocks unclobbered -- each with its memory round trip on
	// the dependent chain; kernel arguments arrive with the scalar loads that fetch the pointers.  The blocks keep their fields (the general
	// kernel, the slow tail and the queries read those); make_params derives these from the same host copies at every launch, so a setter
	// shows in both at the next launch.  Appended at the end: the other kernels take this struct by value and do not notice.
	struct LaunchWords {
		int all_axis_z;        // ModelDev::all_axis_z
		int body;              // TaskDev::body
		int sing_handling;     // TaskDev::sing_handling
		int strategies_on;     // sing_handling && sing_strategies && sh != nullptr: the blended strategies run in the kernel
		int mf_dec, mf_has_ki; // motion-force task: TaskDev::decoupling, ::has_ki
		int jt_dec, jt_has_ki, jt_vel_sat, pad_;  // joint task: TaskDev::decoupling, ::has_ki, ::vel_sat
		double dt, s_max, s_abs_tol, cert_kroot;  // motion-force task
		double jt_dt;
		double pos[3], rot[9];
		double gain[18];       // motion-force task: kp_pos, kv_pos, ki_pos, kp_ori, kv_ori, ki_ori (the run of the task block, in its order)
	} lw;
};

// forward dynamics + semi-implicit Euler step (saip_dynamics.hip)
struct SimParams {
	int B, ld, n, substeps;
	double dt, damping;    // viscous joint damping coefficient (0 = none)
	double gravity[3];
	const ModelDev* model;
	double* q;             // [n][ld] in/out
	double* dq;            // [n][ld] in/out
	const double* tau;     // [n][ld] joint torques held over the call (NaN = coast)
	double* ddq;           // optional [n][ld] joint accelerations of the last substep
	// the resident inertia table (saip_inertia.h), read by the INERTIA instantiations of the integrators only: ten words { m, c (3), I (6) }
	// per movable body in place of the model's; word k of body j is inertia[(10 j + k) inertia_stride + column], a batch-uniform table
	// [n][10] has stride 1 and column 0, a per-instance table [n][10][ld] stride ld and the instance as its column.  nullptr: none.
	const double* inertia = nullptr;
	long long inertia_stride = 0;
};

// one observed rollout period (saip_rollout_record.hip).  Passed to the kernel by value.
enum { REC_Q = 1, REC_DQ = 2, REC_TAU = 4, REC_POSE = 8, REC_ERROR = 16, REC_ALL = 31, REC_SUMMARY_ROWS = 8 };
struct RecordParams {
	int B, ld, n;
	int slot;                    // log slot of this period's sample, -1: not a sampled period (summaries only)
	unsigned channels;           // REC_* bits: the rows of a sample, in that order
	int rows;                    // rows of one sample = what `channels` adds up to
	int task;                    // motion-force task of the pose / error rows and of summary rows 1..4, -1: none
	int pad_;
	double T;                    // length of the period (sim_dt * substeps): weight of the summary integrals
	const ModelDev* model;
	const TaskDev* tasks;
	const double* q;             // [n][ld] the state as the period's integration left it
	const double* dq;            // [n][ld]
	const double* tau;           // [n][ld] the torques applied during the period
	const uint8_t* status;       // [ld] status of the period's cycle
	const double* goal;          // [goal_comps][ld] user goal block of `task`
	double* log;                 // [capacity][rows][ld]
	uint8_t* status_log;         // [capacity][ld]
	double* summary;             // [REC_SUMMARY_ROWS][ld] running summaries, nullptr: off
};

// the goal schedules of one rollout period (saip_goal_schedule.hip): one entry per scheduled task.  Passed to the kernel by value.
enum { SCHED_HOLD = 0, SCHED_LINEAR = 1 };
struct ScheduleEntry {
	double* goal;                // [goal_comps][ld] user goal block of the task
	const double* key;           // the resident keyframes: [K][count][ld] (per_instance) or [K][count] (batch-uniform)
	int first, count;            // the scheduled goal rows [first, first + count)
	int K;                       // keyframes
	int i;                       // keyframe of this period, already clamped to K - 1 on the host
	int mode;                    // SCHED_*
	int per_instance;
	int rot;                     // SCHED_LINEAR over rows 3..11 of a motion-force task: those nine rows are interpolated on SO(3)
	int pad_;
	double s;                    // fraction towards keyframe i + 1, in [0, 1); 0 on a keyframe period and past the last keyframe
};
struct ScheduleParams {
	int B, ld, n, pad_;          // n: entries in use
	ScheduleEntry e[SAIP_MAXT];
};

// robot-model queries (saip_model_query.hip).  Passed to the kernels by value.
enum { SAIP_MAXQF = 8 };         // = SAIP_MAX_QUERY_FRAMES
struct FrameQuery {
	int B, ld, n, nf;
	int rows;                    // rows per frame: 18, or 18 + 6n with the Jacobian
	int jac, world, pad_;
	int body[SAIP_MAXQF];        // movable body of each frame, ascending (-1: welded to the fixed base)
	int slot[SAIP_MAXQF];        // output block of each frame (the caller's order)
	double pos[SAIP_MAXQF][3];   // frame origin in its body frame (the link's fixed transform composed)
	double rot[SAIP_MAXQF][9];   // frame rotation in its body frame, row-major
	double Rwb[9], pwb[3];       // T_world_robot (world = 1)
	const ModelDev* model;
	const double* q;             // [n][ld]
	const double* dq;            // [n][ld]
	double* out;                 // [nf][rows][ld]
};
struct DynQuery {
	int B, ld, n, pad_;
	const ModelDev* model;
	const double* q;             // [n][ld]
	const double* dq;            // [n][ld]
	double* M;                   // [n*n][ld] or nullptr (skipped)
	double* Minv;                // [n*n][ld] or nullptr
	double* g;                   // [n][ld] or nullptr
	double* h;                   // [n][ld] or nullptr: C(q, dq) dq
};

// Internal OTG of one joint task (saip_otg.hip).  Passed to the kernel by value.
enum { OTG_FLAG_GOAL_REACHED = 1, OTG_FLAG_RUCKIG_INIT = 2, OTG_FLAG_STATE_VALID = 4, OTG_FLAG_ERROR = 8, OTG_FLAG_FINISHED_MOVING = 16,
	   OTG_FLAG_GOAL_ORI_VALID = 32, OTG_FLAG_INVALID_GOAL = 64 };
struct OtgDev {
	int m, gs;             // task dof; lanes per robot (8 or 32)
	int epoch, jerk;       // epoch: bumped when the limits change (forces a new trajectory like InputParameter::operator!= does); jerk: 1 =
	                       // jerk-limited mode (third-order profiles, OTG_joints::setMaxJerk), 0 = acceleration-limited (the reference default)
	long long lanes;       // B * gs = stride of one state field
	double dt;             // control period (Ruckig delta_time)
	const double* limits;  // [3][SAIP_MAXN] device copy of the limits: max velocity, max acceleration, max jerk per task dof
	double* state;         // [fields][lanes], lane-major
	double* time;          // [ld] OutputParameter::time
	double* duration;      // [ld] Trajectory::duration
	int* flags;            // [ld] OTG_FLAG_*
	int* seen_epoch;       // [ld]
	int* result;           // [ld] ruckig::Result of the last cycle
	const double* goal;    // [3m][ld] user goal (position, velocity, acceleration rows)
	double* desired;       // [3m][ld] desired state fed to the control law
	const double* q;       // [n][ld] (re-initialisation only)
	const TaskDev* task;   // selection matrix S / control frame (re-initialisation only)
	int n, goal_comps;
	// Cartesian OTG of a motion-force task (OTG_6dof_cartesian): per-instance frames [21][ld] = _reference_frame (9),
	// _goal_orientation_in_base_frame (9), _goal_angular_velocity_in_base_frame (3)
	double* frame;
	const ModelDev* model;
};

}  // namespace saip
