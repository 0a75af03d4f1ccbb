/*
 * saip.h -- C-ABI of the MI355X-native batched operational-space control engine.
 *
 * The reference (manips-sai-org/sai-primitives) has no FFI/plugin layer: its drop-in boundary for the
 * hot path is the public C++ class API
 *     TemplateTask        /root/reference/src/tasks/TemplateTask.h:43-116
 *     MotionForceTask     /root/reference/src/tasks/MotionForceTask.h:96-110, 211-247, 272-300, 423, 670-736
 *     JointTask           /root/reference/src/tasks/JointTask.h:56-75, 140-175, 237-257, 323, 363
 *     RobotController     /root/reference/src/RobotController.h:47-90
 * driven once per control cycle as  robot->updateModel(); updateControllerTaskModels(); <set goals>;
 * computeControlTorques()  (/root/reference/examples/05-using_robot_controller/05-using_robot_controller.cpp:143-196).
 * This header is what a binding for that path would bind: one entry point per reference call, in a batched
 * flavour (B independent robot instances evaluated by one GPU launch).  Plain pointers and sizes only.
 *
 * Conventions
 *   - FP64 everywhere.  All per-instance arrays are struct-of-arrays: field component c of instance b lives
 *     at  ptr[c * ld + b]  where ld = saip_batch_ld(batch) (>= B, padded for alignment) for DEVICE arrays and
 *     ld = B for HOST arrays passed to the *_host setters/getters.
 *   - batch-uniform configuration (gains, flags, task definitions) mirrors the reference setters 1:1.
 *   - errors: status codes; saip_last_error() returns the text the reference would have thrown as
 *     std::invalid_argument (thread-local).  Nothing is computed on the CPU: every compute entry point
 *     fails with SAIP_ERR_NO_DEVICE when no HIP device is usable.
 *
 * Limits (what the reference accepts and this engine does not: every one fails loudly with SAIP_ERR_INVALID_ARGUMENT / _UNSUPPORTED)
 *   - robots are kinematic trees with a fixed base (saip_model_create_tree; no floating base) and at most SAIP_MAX_DOF = 32 movable
 *     joints, revolute or prismatic; fixed links are merged into their movable ancestors.  The fast cycle kernels (lane, eight-lane,
 *     wavefront) cover chains after that merging only; other trees run the general kernel.
 *   - a hierarchy holds at most SAIP_MAX_TASKS = 8 tasks (MotionForceTask / JointTask; RobotController's joint-limit-avoidance task is
 *     the controller option of saip_batch_enable_joint_limit_avoidance, not a ninth task).
 *   - a motion-force task of rank 1 (a single controlled direction) is refused: SingularityHandler's own loop leaves such a task with
 *     stale state in the reference.
 *   - haptic / teleoperation tasks and everything around the control path (Redis, logging, UI) are out of scope.
 */
#ifndef SAIP_H_
#define SAIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAIP_MAX_DOF 32
#define SAIP_MAX_TASKS 8
#define SAIP_NAME_LEN 48

typedef struct saip_model saip_model;
typedef struct saip_batch saip_batch;

typedef enum {
	SAIP_OK = 0,
	SAIP_ERR_INVALID_ARGUMENT = 1, /* what the reference reports by throwing std::invalid_argument */
	SAIP_ERR_UNSUPPORTED = 2,      /* valid in the reference, not (yet) implemented by the engine: fails loudly */
	SAIP_ERR_NO_DEVICE = 3,
	SAIP_ERR_DEVICE = 4,           /* HIP runtime error */
	SAIP_ERR_ORDER = 5             /* call-order contract violated (e.g. compute before update) */
} saip_status;

typedef enum { SAIP_JOINT_FIXED = 0, SAIP_JOINT_REVOLUTE = 1, SAIP_JOINT_PRISMATIC = 2 } saip_joint_type;

/* SaiPrimitives::TaskType, TemplateTask.h:19-24 */
typedef enum { SAIP_TASK_UNDEFINED = 0, SAIP_TASK_JOINT_LIMIT_AVOIDANCE = 1, SAIP_TASK_JOINT = 2, SAIP_TASK_MOTION_FORCE = 3 } saip_task_type;

/* SaiPrimitives::DynamicDecouplingType, helper_modules/SaiPrimitivesCommonDefinitions.h:14-20 (same values) */
typedef enum { SAIP_FULL_DYNAMIC_DECOUPLING = 0, SAIP_BOUNDED_INERTIA_ESTIMATES = 1, SAIP_IMPEDANCE = 2 } saip_decoupling_type;

/* per-instance status written by a cycle (uint8).  SINGULAR excludes the others; TRUNCATED, POPC_OVERFLOW and BLENDED are
 * informational bits on valid torques and may combine. */
enum {
	SAIP_INSTANCE_OK = 0,
	SAIP_INSTANCE_SINGULAR = 1,       /* the engine could not evaluate the instance (blended strategies switched off and the instance outside the
	                                     non-singular branch; sigma_min/sigma_0 < 1e-6; an ambiguous rank gap): its torques are NOT written -- the
	                                     last valid ones are held -- or NaN, see saip_batch_set_flagged_torque_policy; integrators do not advance */
	SAIP_INSTANCE_TRUNCATED = 2,      /* a motion-force task was reduced to its non-singular subspace (handling disabled) or passed through (fully singular) */
	SAIP_INSTANCE_POPC_OVERFLOW = 4,  /* the passivity observer's energy window exceeded the 1024 samples kept on the device */
	SAIP_INSTANCE_BLENDED = 8         /* a motion-force task ran the blended type-1 / type-2 singularity strategies (valid torques) */
};

/* One URDF link + the joint that attaches it to its parent (what sai-model/sai-urdfreader read from a URDF).
 * Link i's parent is link i-1 (serial chain); link 0 hangs off the fixed base.  Fixed links are merged into
 * their parent for dynamics (as RBDL does) and stay addressable by name for kinematics. */
typedef struct saip_link_desc {
	char name[SAIP_NAME_LEN];
	int joint_type;        /* saip_joint_type */
	double origin_xyz[3];  /* <origin xyz> of the joint: child frame in parent frame */
	double origin_rpy[3];  /* <origin rpy>: fixed-axis roll, pitch, yaw */
	double axis[3];        /* <axis xyz>, in the child frame */
	double mass;
	double com[3];         /* <inertial><origin xyz> */
	double inertia[6];     /* ixx iyy izz ixy ixz iyz about the COM, link axes */
	double q_lower, q_upper, velocity_limit, effort_limit; /* <limit> */
} saip_link_desc;

/* ---------------------------------------------------------------- robot model (constants only; replaces the
 * SaiModel constructor + URDF parse; the per-cycle SaiModel::updateModel() is part of the GPU cycle) */
saip_status saip_model_create_serial_chain(const saip_link_desc* links, int n_links, saip_model** out); /* = create_tree(links, NULL, ...) */
/* Kinematic tree: parent[l] is the index in `links` of link l's parent, -1 for the fixed base; every parent comes before its children
 * (parent[l] < l), else SAIP_ERR_INVALID_ARGUMENT naming the link.  parent == NULL means parent[l] = l - 1 (a serial chain).  Fixed links
 * are merged per branch into their movable ancestor (those welded to the base carry no dynamics); a fixed link may have several children.
 * The dof index of a movable link is its rank among the movable links in the given order.  (sai-model orders the joints of a URDF tree
 * the way RBDL adds its bodies [RECALLED, not pinned here]: give the links in that order to reproduce its joint vector.)  A model whose
 * movable bodies form a chain after merging runs exactly as saip_model_create_serial_chain would; any other (forests included) runs the
 * general cycle kernel only (saip_batch_set_kernel(2|3|4) fails with SAIP_ERR_UNSUPPORTED). */
saip_status saip_model_create_tree(const saip_link_desc* links, const int* parent, int n_links, saip_model** out);
int saip_model_joint_parent(const saip_model* model, int joint);          /* movable parent body of joint `joint`; -1 the base, -2 bad index */
void saip_model_destroy(saip_model* model);
int saip_model_dof(const saip_model* model);                               /* SaiModel::dof() */
int saip_model_link_index(const saip_model* model, const char* link_name); /* -1 when absent */
saip_status saip_model_joint_limits(const saip_model* model, double* q_lower, double* q_upper, double* velocity,
									double* effort);                       /* SaiModel::jointLimits() */

/* ---------------------------------------------------------------- batch = B robots + one RobotController each */
/* device: HIP device ordinal.  The engine owns one stream and all device buffers of the batch. */
saip_status saip_batch_create(const saip_model* model, int batch_size, int device, saip_batch** out);
void saip_batch_destroy(saip_batch* batch);
int saip_batch_size(const saip_batch* batch);
int saip_batch_ld(const saip_batch* batch); /* leading dimension (instances) of device SoA arrays */
/* before saip_batch_finalize: a larger leading dimension than the default (B rounded up to 32; must stay a multiple of 32).  The shards of a
 * sharded run that differ by one instance take the largest shard's, so that the final all-gather moves slabs of one shape. */
saip_status saip_batch_set_leading_dimension(saip_batch* batch, int ld);
int saip_batch_dof(const saip_batch* batch);

/* MotionForceTask constructors, MotionForceTask.h:96-110 / MotionForceTask.cpp:16-89.
 * n_trans < 0 && n_rot < 0: full 6-dof task; otherwise dirs_* hold n_* controlled direction vectors (3 doubles
 * each).  rot_in_link may be NULL (identity compliant frame rotation).  Task order = hierarchy order. */
saip_status saip_batch_add_motion_force_task(saip_batch* batch, const char* task_name, const char* link_name,
											 const double pos_in_link[3], const double rot_in_link[9],
											 const double* dirs_trans, int n_trans, const double* dirs_rot, int n_rot,
											 double loop_timestep, int* task_id);
/* JointTask constructors, JointTask.h:56-75 / JointTask.cpp:14-43.  rows == 0: full joint task (S = I). */
saip_status saip_batch_add_joint_task(saip_batch* batch, const char* task_name, const double* joint_selection /*rows x dof*/,
									  int rows, double loop_timestep, int* task_id);
/* RobotController constructor validation, RobotController.cpp:8-66 (>=1 task, equal loop timesteps, unique
 * names, nothing after a full joint task); allocates the device arena.  Must precede any state/goal/cycle call. */
saip_status saip_batch_finalize(saip_batch* batch);

int saip_batch_task_count(const saip_batch* batch);
int saip_batch_task_type(const saip_batch* batch, int task_id);   /* TemplateTask::getTaskType */
const char* saip_batch_task_name(const saip_batch* batch, int task_id); /* TemplateTask::getTaskName / getTaskNames */
int saip_batch_task_by_name(const saip_batch* batch, const char* name); /* get{Joint,MotionForce}TaskByName; -1 when absent */
int saip_batch_task_dof(const saip_batch* batch, int task_id);    /* JointTask::getTaskDof (rows of S); 6-dof projector rank for motion-force */
int saip_batch_goal_components(const saip_batch* batch, int task_id); /* 36 (x3,R9 row-major,v3,w3,a3,alpha3,goal force 3,goal moment 3,sensed force 3,sensed moment 3) or 3*m (q,dq,ddq) */
/* MotionForceTask partial task projection P (6x6 row-major, MotionForceTask.cpp:55-87) and the orthonormal basis of
 * range(P) the engine works in (6x6 row-major, first *rank columns valid; = _current_task_range, :162-168) */
saip_status saip_batch_get_task_projection(const saip_batch* batch, int task_id, double* P36, double* basis36, int* rank);

/* ---- batch-uniform task configuration (reference setters; defaults = the reference DefaultParameters) */
/* MotionForceTask::setPosControlGains / setOriControlGains (.h:272-300): n_gains = 1 (isotropic) or 3 */
saip_status saip_batch_set_pos_control_gains(saip_batch*, int task, const double* kp, const double* kv, const double* ki, int n_gains);
saip_status saip_batch_set_ori_control_gains(saip_batch*, int task, const double* kp, const double* kv, const double* ki, int n_gains);
/* JointTask::setGains (.h:237-257): n_gains = 1 or task dof */
saip_status saip_batch_set_joint_gains(saip_batch*, int task, const double* kp, const double* kv, const double* ki, int n_gains);
/* setDynamicDecouplingType (.h:670 / JointTask.h:363), setBoundedInertiaEstimateThreshold (.h:679 / JointTask.h:372) */
saip_status saip_batch_set_dynamic_decoupling_type(saip_batch*, int task, int type);
saip_status saip_batch_set_bie_threshold(saip_batch*, int task, double threshold);
/* MotionForceTask::enableSingularityHandling / disableSingularityHandling (.h:715-725 -> SingularityHandler.h:146-158).
 * enabled (reference default): instances that leave the fully non-singular branch run the reference's blended singularity
 * strategies (next entry).
 * disabled: the reference then uses only the non-singular part of the task, _N = _N_ns and tau = tau_ns
 * (SingularityHandler.cpp:146-148, 319-330): the task acts on the span of the leading left singular vectors of its projected
 * Jacobian, up to the first sigma_i / sigma_0 < s_max (:100-121); a fully singular task (sigma_0 < 1e-3) is passed through.
 * Implemented: such instances finish with valid torques and status 2 (flagged by the lane kernel, recomputed by the general
 * kernel launched behind it as a device-side slow path). */
saip_status saip_batch_set_singularity_handling(saip_batch*, int task, int enabled);
/* Blended singularity strategies of SingularityHandler (updateTaskModel :100-121, 146-228; classifySingularity :230-295;
 * computeTorques :310-367) for instances inside the bounds (s_min, s_max), with the handling strategy enabled.  ON by default, like in the
 * reference (which has no switch for them); switching them off is an engine extra: such instances are then flagged (status 1) and
 * nothing but the fully non-singular branch is ever evaluated.  On: the task is split into its non-singular and singular directions, the
 * singular ones are blended out by alpha = (sigma_s/sigma_0 - s_min)/(s_max - s_min) in favour of a joint strategy (type 1: hold
 * the entering posture, kp 50 / kv 14; type 2: constant torque 1e-2 x the torque limit along the open direction, damping kv 5),
 * chosen by the majority of the last 200 classifications; status bit 8.  Per-instance handler state (entering posture, type
 * window, type-2 direction) lives on the device and is reset by this call.  Conventions where the reference depends on the sign
 * its SVD happens to return are fixed as DESIGN.md states.  A fully singular task (sigma_0 < 1e-3) is passed through like in the reference
 * (zero torques, N = N_prec, :149-151, 316-317; status bit 2; its classification is skipped); sigma_min/sigma_0 < 1e-6 -> status 1. */
saip_status saip_batch_set_singularity_strategies(saip_batch*, int task, int enabled);
/* MotionForceTask::setSingularityHandlingGains (.h:749 -> SingularityHandler.h:119; defaults 50, 14, 5) */
saip_status saip_batch_set_singularity_gains(saip_batch*, int task, double kp_type_1, double kv_type_1, double kv_type_2);
/* MotionForceTask::handleAllSingularitiesAsType1 (.h:698 -> SingularityHandler.h:131) */
saip_status saip_batch_set_all_singularities_type1(saip_batch*, int task, int flag);
/* MotionForceTask::setType1Posture (.h:707 -> SingularityHandler.h:140): the posture the type-1 strategy holds, q_des[dof]
 * (per_instance = 0) or [B][dof] (1).  As in the reference it lasts until an instance next ENTERS a singular region (:232-235). */
saip_status saip_batch_set_type1_posture(saip_batch*, int task, const double* q_des, int per_instance);
/* MotionForceTask::setSingularityHandlingBounds (.h:736) */
saip_status saip_batch_set_singularity_bounds(saip_batch*, int task, double s_min, double s_max);
/* disableInternalOtg / enableInternalOtg* (MotionForceTask.h:423, JointTask.h:323).  The reference default is ENABLED.
 * The acceleration-limited OTG (the reference default mode; Ruckig second-order position interface with phase
 * synchronisation) runs on the device, one launch ahead of the cycle kernel, and the control law tracks its output:
 * joint tasks OTG_joints.cpp (JointTask.cpp:313-319), motion-force tasks OTG_6dof_cartesian.cpp (MotionForceTask.cpp:394-406). */
saip_status saip_batch_set_internal_otg(saip_batch*, int task, int enabled);
/* JointTask::enableInternalOtgAccelerationLimited(max_velocity, max_acceleration) (JointTask.cpp:358-381): count = 1 (scalar) or
 * task dof; values <= 0 -> SAIP_ERR_INVALID_ARGUMENT (OTG_joints.cpp:44-74).  Defaults pi/3 rad/s, 2 pi rad/s^2 (JointTask.h:40-41).
 * MotionForceTask::enableInternalOtgAccelerationLimited(max_lin_vel, max_lin_acc, max_ang_vel, max_ang_acc)
 * (MotionForceTask.cpp:510-523): count = 2, max_velocity = {linear, angular}, max_acceleration = {linear, angular}; defaults
 * 0.3 m/s, 2 m/s^2, pi/3 rad/s, 2 pi rad/s^2 (MotionForceTask.h:68-71).
 * Enabling a previously disabled OTG re-initialises it at the current task position / pose on the next cycle. */
saip_status saip_batch_set_otg_acceleration_limited(saip_batch*, int task, const double* max_velocity, const double* max_acceleration, int count);
/* JointTask::enableInternalOtgJerkLimited(max_velocity, max_acceleration, max_jerk) (JointTask.cpp:383-410; OTG_joints::setMaxJerk,
 * OTG_joints.cpp:73-86): count = 1 or the task dof.  MotionForceTask::enableInternalOtgJerkLimited (MotionForceTask.cpp:525-545): count = 2,
 * {linear, angular} each.  Third-order (jerk-limited) Ruckig profiles on the device (csrc/saip_otg3.h: the reference's vendored Ruckig
 * 0.10.1 position interface, ruckig/src/ruckig/position-third-step{1,2}.cpp); limits must be positive.  The OTG is re-initialised at the
 * current task position / pose on the next cycle when it was off or acceleration-limited (JointTask.cpp:400-402). */
saip_status saip_batch_set_otg_jerk_limited(saip_batch*, int task, const double* max_velocity, const double* max_acceleration, const double* max_jerk, int count);
/* ---- the step after the path: what the reference's examples do with the external simulator,
 * sim->setJointTorques(tau); sim->integrate() (examples/05-using_robot_controller/05-using_robot_controller.cpp:225-231).
 * Forward dynamics M(q) qdd + b(q,dq) + g(q) = tau - damping*dq on the resident state with the torques of the last cycle held,
 * then `substeps` semi-implicit Euler steps of size dt (dq += dt*qdd; q += dt*dq).  gravity = NULL uses the model's gravity
 * (0, 0, -9.81); pass {0,0,0} for the gravity-free worlds of the reference's examples.  Instances whose torque is NaN (flagged
 * as outside the non-singular branch) coast.  The state changed: saip_batch_update_task_models is due before the next
 * saip_batch_compute_control_torques, exactly like after robot->setQ(). */
saip_status saip_batch_integrate(saip_batch*, double dt, int substeps, const double gravity[3], double damping);
/* `steps` closed-loop control periods { internal OTGs -> control cycle -> integrate(sim_dt, substeps) } enqueued back to back on the
 * engine stream without host synchronisation (follow with saip_batch_synchronize); goals stay as they are on the device unless a goal
 * schedule is attached (below). */
saip_status saip_batch_rollout_async(saip_batch*, int steps, double sim_dt, int substeps, const double gravity[3], double damping);
/* ---- goal schedules: time-varying task goals inside rollouts (the reference's example loops call setGoalPosition / setGoalOrientation /
 * setGoalLinearVelocity every cycle as a function of time: examples 02, 03, 06, 09, 10).  A schedule is a list of keyframes for ONE
 * contiguous range [first_component, first_component + n_components) of one task's goal block, in the component numbering of
 * saip_batch_set_goal_field_host / saip_batch_goal_components (36 rows for a motion-force task, sensed force and moment included; 3m for
 * a joint task).  At most one schedule per task; it stays attached across rollout calls until detached.
 *   keyframes: host [n_keyframes][n_components][B] with per_instance = 1, [n_keyframes][n_components] (the same for every instance)
 *        with per_instance = 0; copied to the device by _attach ([K][count][ld] or [K][count]), never inside a rollout.
 *        saip_batch_goal_schedule_device returns the resident copy, to be rewritten in place between rollouts (a sampler on the device:
 *        saip_batch_sampler_* below is one).
 *   timing: a period counter c, shared by every schedule of the batch, starts at 0 at _attach and _rewind and advances with every period
 *        of saip_batch_rollout_async.  Period c uses keyframe i = c / stride and the fraction s = (c % stride) / (double)stride; from
 *        c = (n_keyframes - 1) * stride on, the last keyframe is held.  i and s are computed at enqueue time and passed as launch arguments.
 *   SAIP_SCHEDULE_HOLD   the rows of keyframe i.
 *   SAIP_SCHEDULE_LINEAR a + s * (b - a) per component between keyframes i and i + 1, difference, product and sum each rounded once in
 *        double precision (no fused multiply-add), so a host restatement gives the same bits; at s == 0 the rows of keyframe i exactly.
 *        Rows 3..11 of a motion-force task (the goal rotation, row-major) are interpolated on SO(3) instead:
 *        R(s) = R0 Exp(s Log(R0^T R1)); the range must then cover all nine rows (or none), every keyframe must be a rotation
 *        (max |R^T R - I| <= 1e-6) and consecutive keyframes at most pi - 1e-3 rad apart.  HOLD validates nothing, like
 *        saip_batch_set_goal_field_host.
 * A period with a schedule attached enqueues one small launch that writes the scheduled goal rows of every scheduled task (columns
 * 0..B-1 only), then the usual OTG step, cycle, integration and recorder observation: the OTG step sees the period's goal as it does
 * after a host setGoal...(), and the recorder's error rows are taken against it.  The integration is then never fused with the next
 * period's OTG step.  Without a schedule a rollout enqueues exactly what it did before.  saip_batch_step_async, saip_batch_integrate
 * and saip_batch_compute_control_torques called directly apply no schedule and do not advance c.  After a rollout the goal rows hold
 * the values applied last (saip_batch_get_goal_host).  _detach waits for the stream and frees the keyframes; task = -1 detaches all.
 * SAIP_ERR_ORDER: before saip_batch_finalize, on a model-only batch, a second _attach on a task without _detach, _detach / _info of a
 * task without a schedule.  Argument and order errors are reported before the device is needed. */
enum { SAIP_SCHEDULE_HOLD = 0, SAIP_SCHEDULE_LINEAR = 1 };
saip_status saip_batch_goal_schedule_attach(saip_batch*, int task, int first_component, int n_components, const double* keyframes,
                                            int n_keyframes, int stride, int mode, int per_instance);
saip_status saip_batch_goal_schedule_detach(saip_batch*, int task);
saip_status saip_batch_goal_schedule_rewind(saip_batch*);
/* any pointer may be NULL; period: the counter c */
saip_status saip_batch_goal_schedule_info(saip_batch*, int task, int* first, int* count, int* n_keyframes, int* stride, int* mode, long long* period);
double* saip_batch_goal_schedule_device(saip_batch*, int task);  /* NULL when the task has no schedule */
/* ---- state snapshots: the complete per-instance state of a batch -- robot state, held torques, status, and per task the goal rows,
 * the PID integrators, the internal OTG (profiles, scalars, frames, desired rows), the singularity handler's windows and the passivity
 * observer's ring -- captured on the device and written back through a per-instance source index: instance i takes the state that
 * instance src[i] had at the save.  NULL / the identity restores, src[i] = j broadcasts instance j, anything else resamples or permutes.
 * What a sampling MPC does between two rollouts:
 *     saip_batch_snapshot_save(b, s);                                  (the measured state, once)
 *     { saip_batch_snapshot_restore(b, s, broadcast_of_0); saip_batch_rollout_async(b, K, ...); read the summaries }
 *     saip_batch_snapshot_restore(b, s, best);
 * The recorder and its period counter, the goal schedules and their period counter are NOT part of a snapshot: pair a restore with
 * saip_batch_rollout_recorder_reset / saip_batch_goal_schedule_rewind.  A sampler's nominal plan, round counter and costs are not part
 * of it either.  Configuration (gains, limits, flags) is not part of it either: limits changed after a save still start a new
 * trajectory on the next cycle.  The goal rows are part of it.
 *   _create   allocates a copy of every state array the batch has at that moment (arrays of enabled features that the first cycle would
 *             allocate are allocated here) and fixes the layout: a list of segments { name, rows, elem_bytes, group, kind, offset }.
 *             kind SAIP_SNAPSHOT_SOA: rows x [ld] elements; _GROUPED: rows x [B * group] doubles, instance i owns elements i*group ..
 *             i*group + group - 1 of every row; _AOS: [ld] records of elem_bytes.  offset: of the segment inside the host blob.
 *   _save, _restore, _restore_device   one kernel launch on the engine stream behind whatever is enqueued; they do not wait for the
 *             device.  _restore checks the host map first (every entry in 0 .. B-1, else SAIP_ERR_INVALID_ARGUMENT and nothing
 *             happens) and uploads it from a staging buffer the snapshot owns.  _restore_device reads the map [B] (int) from device
 *             memory in stream order; an entry outside 0 .. B-1 leaves that instance untouched.  Only columns 0 .. B-1 are written.
 *             A restored state is a new state (like saip_batch_set_state_host): the task models are due.
 *   refusals  a snapshot works with the batch that created it only (SAIP_ERR_INVALID_ARGUMENT otherwise).  SAIP_ERR_ORDER: the state
 *             layout of the batch no longer matches (an internal OTG enabled for the first time, passivity or singularity state
 *             allocated, torques bound to another buffer after _create -- the message names the first segment that differs; create a
 *             new snapshot), a restore of a snapshot nothing was saved into, a batch before saip_batch_finalize or finalized for
 *             model queries only.  A configuration-only batch: SAIP_ERR_NO_DEVICE, after the argument errors.  A failed call writes
 *             nothing to its outputs.
 *   host blob _export_host / _import_host copy a snapshot to / from host memory (they wait for the stream): saip_snapshot_bytes bytes =
 *             a 256-byte header { char magic[8] = "SAIPSNAP"; uint32 version, n_segments; uint64 fingerprint, bytes; int32
 *             otg_prelaunched, n_tasks; { int32 sh_cycle, otg_inited } [8]; zero padding } and the segments at their offsets.  The
 *             fingerprint hashes dof, B, ld and every segment's name, rows, elem_bytes and group.  _import_host refuses a short
 *             buffer, a bad magic, another version and another fingerprint with SAIP_ERR_INVALID_ARGUMENT before it touches the
 *             device (with a NULL snapshot the blob is checked against the layout of the batch, then refused).  The format is not
 *             stable across versions of the library; the header is what detects that. */
typedef struct saip_snapshot saip_snapshot;
enum { SAIP_SNAPSHOT_SOA = 0, SAIP_SNAPSHOT_GROUPED = 1, SAIP_SNAPSHOT_AOS = 2 };
saip_status saip_batch_snapshot_create(saip_batch*, saip_snapshot** out);
void saip_snapshot_destroy(saip_snapshot*);  /* waits for the batch's stream; also valid after saip_batch_destroy of its batch */
saip_status saip_batch_snapshot_save(saip_batch*, saip_snapshot*);
saip_status saip_batch_snapshot_restore(saip_batch*, const saip_snapshot*, const int* src_host /* [B], NULL = identity */);
saip_status saip_batch_snapshot_restore_device(saip_batch*, const saip_snapshot*, const int* src_dev /* [B] */);
int saip_snapshot_segments(const saip_snapshot*);
/* any output pointer may be NULL; name stays valid as long as the snapshot */
saip_status saip_snapshot_segment_info(const saip_snapshot*, int i, const char** name, int* rows, int* elem_bytes, int* group, int* kind, size_t* offset);
size_t saip_snapshot_bytes(const saip_snapshot*);
saip_status saip_snapshot_export_host(saip_batch*, const saip_snapshot*, void* out, size_t bytes);
saip_status saip_snapshot_import_host(saip_batch*, saip_snapshot*, const void* in, size_t bytes);
/* ---- resident rollout sampler: the three steps of a sampling-MPC round that complete the loop above on the device -- make the B
 * candidates differ, turn the recorded rollout into one cost per candidate, fold the costs back into the plan (MPPI, model-predictive
 * path-integral control; a tiny temperature takes the best).  A sampler belongs to ONE task's goal schedule, which must be per-instance
 * (HOLD or LINEAR); it keeps a nominal plan [K][count] and rewrites the schedule's resident keyframes in place around it.
 *   coordinates  the rows of the schedule's range in order; when the range covers rows 3..11 of a motion-force task (all nine or none:
 *        a partial cover is refused) those nine rows are replaced by three tangent coordinates, axis-angle in radians in the keyframe's
 *        own frame, applied as R Exp(.).  d = count - 6 with a rotation, d = count without; sigma is [d].
 *   noise  Philox4x32-10 with counter (instance, keyframe, (task << 16) | p, round) and key (seed_lo, seed_hi); words 0, 1 and words 2, 3
 *        make two uniforms u = (((hi >> 5) * 2^26 + (lo >> 6)) + 0.5) * 2^-53, Box-Muller makes the normals of coordinates 2p and 2p + 1
 *        from them.  The noise of an instance depends on (seed, round, task, instance, keyframe, coordinate) only.
 *   _perturb  every sampled task, one launch: key[k][c][i] = nominal[k][c] + sigma * z (product and sum rounded once each), rotations
 *        R_nom Exp(sigma o z); instances 0 .. exempt - 1 get the nominal rows bit for bit.  Uses the round counter, then advances it.
 *   _cost  one launch: cost_i = sum over r < 8 with w_summary[r] != 0 of w_summary[r] * summary[r][i], then + w_path * sum over the
 *        samples of the recorder's ring (oldest first) of |p_i - target|^2, then + w_final * |p_i(last sample) - target|^2, p the position
 *        rows of the POSE channel; every product and sum rounded once, left to right from 0, |e|^2 as ((e0 e0 + e1 e1) + e2 e2).  The
 *        two target terms are present only with a target.  _set_cost_host / _get_cost_host / _cost_device: the cost array [ld] itself.
 *   _update  two launches: beta = the minimum finite cost, best = the lowest index that attains it, w_i = exp(-(cost_i - beta) /
 *        temperature) (0 for a cost that is not finite); per keyframe nominal[k][c] <- sum w_i key[k][c][i] / sum w_i, rotations
 *        R_nom <- R_nom Exp(sum w_i Log(R_nom^T R_i) / sum w_i) (with all the weight on one instance in double precision: that instance's
 *        rotation rows).  No atomics: lane l of 256 adds instances l, l + 256, ... in that order, then a fixed tree over the lanes, so
 *        two runs give the same bits.  It writes the result { best, n_valid, min_cost, sum_w, ess = (sum w)^2 / sum w^2 } and the best map
 *        [B] = best on the device; saip_batch_snapshot_restore_device takes the map as it is.  Without a finite cost the nominal stays,
 *        best = -1 and the map holds -1 (such an entry leaves the instance as it is).
 *   _shift  nominal[k] <- nominal[min(k + n, K - 1)]: the warm start of a receding horizon.
 * Everything is enqueued on the engine stream; only the _host entries wait.  The cost array, the result and the best map belong to the
 * batch: allocated by the first _attach, freed by the last _detach (task = -1 detaches all).  saip_batch_goal_schedule_detach of a
 * sampled task detaches its sampler first.  The nominal plan, the round counter and the costs are NOT part of a state snapshot.
 * A sampled range has at most 36 rows (the goal block of a motion-force task; a longer range of a joint task is refused).  With a LINEAR
 * schedule over the rotation rows the nominal plan is checked like the schedule's keyframes, in _attach and in _set_nominal_host (every
 * keyframe a rotation to 1e-6, consecutive keyframes at most pi - 1e-3 apart); a HOLD schedule's nominal is not checked, like its
 * keyframes.  The perturbed keyframes are not checked: keeping sigma small enough that consecutive perturbed rotations stay inside
 * pi - 1e-3 of each other is the caller's obligation.
 * SAIP_ERR_INVALID_ARGUMENT: a temperature that is not finite or <= 0 and n < 0 (both before anything else is looked at), exempt
 * outside 0 .. B, a negative or non-finite sigma, a batch-uniform schedule, a range over part of rows 3..11 or of more than 36 rows, a
 * nominal plan that fails the check above.  SAIP_ERR_ORDER: a task without a schedule, a second _attach on a
 * task, any other entry without a sampler, _cost with a non-zero summary weight but no recorder summaries, _cost with a target but no
 * POSE channel or no sample yet.  Argument and order errors are reported before the device is needed; a failed call writes nothing.
 *
 * Scenario groups: planning under randomisation.  saip_batch_sampler_set_scenarios(n_scenarios = M, risk, tail) makes the batch of
 * B = C M instances C candidate plans, each rolled out in M scenarios: instance i = s C + c is candidate c = i % C in scenario s = i / C,
 * so the batch is M scenario blocks of C columns and block 0 is what an ungrouped sampler on a batch of C would be, bit for bit.  M = 1,
 * the default, is the sampler described above: the same launches, the same bits.  With M > 1:
 *   _perturb  the noise counter's instance word and the exempt test use the candidate c: the keyframes of candidate c are the same bits
 *        in every scenario block, those of an ungrouped batch of C under the same seed, round and task.
 *   _update  three launches.  First the group cost [C], one lane per candidate over v_s = cost[s C + c]: +inf if any v_s is not finite
 *        (one bad scenario makes the candidate invalid), else by the risk measure
 *          SAIP_SAMPLER_RISK_MEAN  (((0.0 + v_0) + v_1) + ... + v_{M-1}) / M
 *          SAIP_SAMPLER_RISK_MAX   the largest v_s (as 0.0 + v: a largest value of -0.0 is reported as +0.0)
 *          SAIP_SAMPLER_RISK_CVAR  the `tail` largest v_s added in descending order from 0.0, divided by tail; tail = 1 is MAX bit for bit
 *        then weights and update as above over the C group costs and columns 0 .. C - 1 of the keyframes: best is the best candidate
 *        (also the index of its scenario-0 instance), n_valid, min_cost, sum_w and ess are over candidates, and the best map is
 *        map[i] = (i / C) C + best, every scenario block taking its own copy of the best candidate (-1 everywhere without a finite
 *        group cost).  The weights [ld] hold C entries.
 *   _cost, _set_cost_host, _get_cost_host and saip_batch_clearance_add_cost keep working on the B per-instance costs; _shift and the
 *        nominal accessors are unchanged.
 *   _get_group_cost_host / _group_cost_device  the group cost [C] the last _update formed.  With M = 1 no group cost is formed: both give
 *        the cost array itself ([B] = [C]), not a copy.
 *   _share_scenario_tables  makes scenario s the same simulated robot for every candidate: in every resident per-instance table that a
 *        _randomize entry can fill, column i takes the bits of column (i / C) C.  One launch per array, enqueued on the engine stream;
 *        *n_arrays is the number of arrays touched, at most 8: the plant's joint table, its wrench table, the actuation chain's table, the
 *        inertia's part staging (bodies and payloads, one array), the composed inertia rows the integrator reads (composition is a
 *        per-column function of the parts), the sensing model's joint table, its wrench tables, the sensing chain's table -- each only
 *        while attached per instance; batch-uniform tables are skipped and not counted.  Source columns and columns B .. ld - 1 are not
 *        written.  State is not shared: chain taps, filters and primed flags stay per instance, and the sensing model's noise stays keyed
 *        by the instance.
 * SAIP_ERR_INVALID_ARGUMENT of _set_scenarios, before anything else is looked at: n_scenarios outside 1 .. SAIP_SAMPLER_MAX_SCENARIOS, an
 * unknown risk, a tail outside 1 .. n_scenarios with CVAR or other than 0 without, B no multiple of n_scenarios.  Then SAIP_ERR_ORDER
 * without a sampler, then SAIP_ERR_INVALID_ARGUMENT if an attached sampler's exempt exceeds C; a later _attach refuses exempt > C likewise.
 * Detaching the last sampler resets the setting to M = 1.  _share_scenario_tables: SAIP_ERR_ORDER without a sampler or with M = 1.  A
 * failed call changes nothing. */
#define SAIP_SAMPLER_MAX_SCENARIOS 64
#define SAIP_SAMPLER_RISK_MEAN 0
#define SAIP_SAMPLER_RISK_MAX 1
#define SAIP_SAMPLER_RISK_CVAR 2
saip_status saip_batch_sampler_attach(saip_batch*, int task, const double* sigma /* [d] */, const double* nominal /* [K][count], NULL = column 0 of the resident keyframes */, int exempt);
saip_status saip_batch_sampler_detach(saip_batch*, int task /* -1: all */);
saip_status saip_batch_sampler_seed(saip_batch*, unsigned long long seed);  /* also sets round = 0 */
saip_status saip_batch_sampler_perturb(saip_batch*);                        /* every sampled task; round += 1 */
saip_status saip_batch_sampler_cost(saip_batch*, const double w_summary[8] /* NULL = none */, const double target[3] /* NULL = none */, double w_path, double w_final);
saip_status saip_batch_sampler_set_cost_host(saip_batch*, const double* cost /* [B] */);
saip_status saip_batch_sampler_get_cost_host(saip_batch*, double* cost /* [B] */);  /* synchronous */
double* saip_batch_sampler_cost_device(saip_batch*);                        /* [ld]; NULL without a sampler */
saip_status saip_batch_sampler_update(saip_batch*, double temperature);     /* every sampled task */
saip_status saip_batch_sampler_shift(saip_batch*, int n);
saip_status saip_batch_sampler_result_host(saip_batch*, int* best, int* n_valid, double* min_cost, double* sum_w, double* ess);  /* synchronous; any NULL */
const int* saip_batch_sampler_best_map_device(saip_batch*);                 /* [ld]; NULL without a sampler */
saip_status saip_batch_sampler_get_nominal_host(saip_batch*, int task, double* out /* [K][count] */);
saip_status saip_batch_sampler_set_nominal_host(saip_batch*, int task, const double* in);
saip_status saip_batch_sampler_info(saip_batch*, int task, int* d, int* exempt, unsigned long long* seed, long long* round);
saip_status saip_batch_sampler_set_scenarios(saip_batch*, int n_scenarios, int risk, int tail /* CVAR: 1 .. n_scenarios; else 0 */);
saip_status saip_batch_sampler_scenarios_info(saip_batch*, int* n_scenarios, int* n_candidates, int* risk, int* tail);  /* any NULL */
saip_status saip_batch_sampler_get_group_cost_host(saip_batch*, double* out /* [C] */);  /* synchronous */
double* saip_batch_sampler_group_cost_device(saip_batch*);                  /* [ld]; NULL without a sampler */
saip_status saip_batch_sampler_share_scenario_tables(saip_batch*, int* n_arrays /* may be NULL */);
const double* saip_batch_sampler_weights_device(saip_batch*);               /* [ld] the softmin weights of the last _update, one per candidate; NULL without a sampler */
/* ---- contact planes and a simulated force sensor: something for the resident simulator to touch, so that a force task (closed-loop
 * force / moment control, the passivity observer, the sensed-wrench diagnostics) can be rolled out with no host in the loop.  One
 * attachment per batch: ONE contact point p = x_c + R_c r_c carried by the body of a motion-force task (x_c, R_c: its control point and
 * control frame in the world, r_c: an offset in the control frame, NULL = 0) against n_planes (1..SAIP_CONTACT_MAX_PLANES) world-fixed
 * half-spaces.  A plane is eight doubles { n[3], o, k, c, mu, v_s }: normal (normalised by the engine), offset, stiffness k > 0,
 * damping c >= 0, friction mu >= 0, slip-regularisation speed v_s > 0.  `planes` is [P][8] (batch-uniform) or [P][8][B] (per_instance).
 * With d = n.p - o and v the velocity of the point, a plane acts only when d < 0:
 *   v_n = n.v    f_n = max(0, -k d - c v_n)    v_t = v - v_n n    f_t = -mu f_n v_t / max(|v_t|, v_s)    f = sum (f_n n + f_t)
 * every product and sum rounded once, in that order (csrc/saip_contact.h; tests/contact_ref.py restates it in NumPy bit for bit).
 *   while attached, every integration of saip_batch_rollout_async and saip_batch_integrate becomes, per SUBSTEP: one launch that writes
 *        tau_sim[j] = (tau[j] is NaN ? 0 : tau[j]) + (J_v^T f)[j] into a buffer of the attachment (a flagged instance still gets pushed
 *        by the wall; a joint that is not an ancestor of the body gets no contact torque), then the integrator with that buffer and one
 *        substep.  The force is an explicit penalty force: it is stable roughly while k dt^2 / m_eff < 1 (dt the substep, m_eff the
 *        effective mass at the point along the normal); this is not enforced.  The torque array of the batch is left as the cycle wrote
 *        it (the recorder keeps logging the commanded torques).  The fused forms of a rollout period are not used while attached.
 *   sensor != 0: a rollout period starts (behind its goal schedules) with one launch that writes the wrench a sensor would report at
 *        the period's state into rows 30..35 of the task's goal block: world F = -f, m = (p - x_c) x F (the wrench the sensor applies
 *        to the environment, MotionForceTask.h:538-553), then FS = R_cs^T R_c^T F, MS = R_cs^T (R_c^T m - t_cs x R_c^T F) -- the exact
 *        inverse of what the control law does with those rows.  saip_batch_contact_sense enqueues the same launch, so the host-driven
 *        loop { _contact_sense, saip_batch_step_async, saip_batch_integrate } leaves the bits of a rollout period.  A goal schedule of
 *        that task that covers any of rows 30..35 cannot coexist with the sensor (SAIP_ERR_ORDER from whichever _attach comes second).
 *   readout [8][ld] (both launches): f (world) 3, p 3, the smallest d over the planes, the number of active planes -- of the LAST launch.
 *   summaries [4][ld], advanced by every substep: sum dt sum f_n, max |f|, max penetration (-d), substeps in contact.  _summary_reset
 *        zeroes them on the stream; _set_planes_host replaces the table (same shape) and waits; _planes_device is the resident table
 *        ([P][8] or [P][8][ld]) for domain randomisation on the device -- what is written there is not checked.
 * The attachment's arrays are configuration, scratch and readout: not part of a state snapshot.  Without an attachment every entry
 * point enqueues exactly what it did before.  SAIP_ERR_INVALID_ARGUMENT: a task that is not a motion-force task, n_planes outside
 * 1..4, NULL planes, a value that is not finite, a zero normal, k <= 0, c < 0, mu < 0, v_s <= 0.  SAIP_ERR_ORDER: before finalize, a
 * model-only batch, a second _attach, any other entry without an attachment, _contact_sense on an attachment without the sensor.
 * Argument and order errors are reported before the device is needed. */
#define SAIP_CONTACT_MAX_PLANES 4
#define SAIP_CONTACT_PLANE_WORDS 8
#define SAIP_CONTACT_READOUT_ROWS 8
#define SAIP_CONTACT_SUMMARY_ROWS 4
saip_status saip_batch_contact_attach(saip_batch*, int task, const double r_c[3] /* NULL = 0 */, int n_planes, const double* planes, int per_instance, int sensor);
saip_status saip_batch_contact_detach(saip_batch*);
saip_status saip_batch_contact_info(saip_batch*, int* task, int* n_planes, int* per_instance, int* sensor, double* r_c /* [3] */);  /* any NULL */
saip_status saip_batch_contact_set_planes_host(saip_batch*, const double* planes);
double* saip_batch_contact_planes_device(saip_batch*);   /* NULL when detached */
saip_status saip_batch_contact_sense(saip_batch*);
saip_status saip_batch_contact_readout_host(saip_batch*, double* out /* [8][B] */);  /* synchronous */
double* saip_batch_contact_readout_device(saip_batch*);  /* [8][ld]; NULL when detached */
double* saip_batch_contact_torques_device(saip_batch*);  /* [dof][ld] tau_sim of the last integrated substep; NULL when detached */
saip_status saip_batch_contact_summary_host(saip_batch*, double* out /* [4][B] */);  /* synchronous */
double* saip_batch_contact_summary_device(saip_batch*);  /* [4][ld]; NULL when detached */
saip_status saip_batch_contact_summary_reset(saip_batch*);
/* ---- contact patches: multi-point contact with a wrench sensor.  A patch is n_points (1..SAIP_CONTACT_PATCH_MAX_POINTS) offsets r_i in
 * the control frame of a motion-force task (`points`, [n][3]), carried by that task's body, against the patch's own planes (format, checks
 * and layouts of saip_batch_contact_attach).  Up to SAIP_CONTACT_PATCH_MAX patches per batch, on different tasks (the two arms of a tree),
 * never together with the single-point attachment above: SAIP_ERR_ORDER from whichever _attach comes second, from a second patch on a
 * task and from a third patch.  Per point p_i = x_c + R_c r_i and f_i as above; an instance has eight slots, the unused ones hold exact
 * zeros, and every sum over the slots has the shape v[i] += v[i + off], off = 4, 2, 1 (csrc/saip_contact_patch.h; tests/contact_patch_ref.py
 * restates it bit for bit):  F = sum f_i,  M = sum (p_i - x_c) x f_i,  n_touch = points with an active plane.
 *   per SUBSTEP of saip_batch_rollout_async / saip_batch_integrate one launch for all patches (in place of the single-point launch) writes
 *        tau_sim[j] = ((tau[j] is NaN ? 0 : tau[j]) + ext_0[j]) + ext_1[j], ext_k[j] = sum_i (J_v(p_i)^T f_i)[j] of patch k (in attach
 *        order), added only for ancestor joints of the patch's body and only when a point of it touches.  One point gives the numbers of
 *        the single-point attachment.  The fused forms of a rollout period are not used while a patch is attached.
 *   sensor != 0: as above, with world F_w = -F, m_w = -M in place of the single point's wrench.  A rollout period enqueues the sensing
 *        launch only if some patch has the sensor, and it evaluates those patches only; saip_batch_contact_patch_sense enqueues the same
 *        launch, so { _contact_patch_sense, saip_batch_step_async, saip_batch_integrate } leaves the bits of a rollout period.  The
 *        schedule-versus-sensor rule on rows 30..35 holds per task.
 *   readout [20][ld] per patch, of the LAST launch that evaluated it: F 3, M 3 (about x_c, world), the smallest d over the points, n_touch,
 *        the lowest point index that attains it, x_c 3, then the normal-force sum of each of the eight slots.
 *   summaries [6][ld] per patch, advanced by every substep: sum dt sum f_n, max |F|, max penetration, substeps with n_touch > 0, max |M|,
 *        substeps in full contact (n_touch == n_points).  They are not part of a state snapshot: a restore pairs with _summary_reset.
 * `task` selects the patch; -1 is every patch for _detach and _summary_reset and the first attached one elsewhere.  Errors as for
 * saip_batch_contact_attach, plus SAIP_ERR_INVALID_ARGUMENT for n_points outside 1..8, NULL points and a point that is not finite, and
 * SAIP_ERR_ORDER for a task without a patch and for _sense when no patch has the sensor. */
#define SAIP_CONTACT_PATCH_MAX_POINTS 8
#define SAIP_CONTACT_PATCH_MAX 2
#define SAIP_CONTACT_PATCH_READOUT_ROWS 20
#define SAIP_CONTACT_PATCH_SUMMARY_ROWS 6
saip_status saip_batch_contact_patch_attach(saip_batch*, int task, int n_points, const double* points /* [n][3] */, int n_planes, const double* planes, int per_instance, int sensor);
saip_status saip_batch_contact_patch_detach(saip_batch*, int task /* -1 = all */);
saip_status saip_batch_contact_patch_info(saip_batch*, int task, int* n_patches, int* n_points, int* n_planes, int* per_instance, int* sensor, double* points /* [8][3] */);  /* any NULL */
saip_status saip_batch_contact_patch_set_planes_host(saip_batch*, int task, const double* planes);
double* saip_batch_contact_patch_planes_device(saip_batch*, int task);   /* NULL when the task has no patch */
saip_status saip_batch_contact_patch_sense(saip_batch*);
saip_status saip_batch_contact_patch_readout_host(saip_batch*, int task, double* out /* [20][B] */);  /* synchronous */
double* saip_batch_contact_patch_readout_device(saip_batch*, int task);  /* [20][ld] */
saip_status saip_batch_contact_patch_summary_host(saip_batch*, int task, double* out /* [6][B] */);  /* synchronous */
double* saip_batch_contact_patch_summary_device(saip_batch*, int task);  /* [6][ld] */
saip_status saip_batch_contact_patch_summary_reset(saip_batch*, int task /* -1 = all */);
double* saip_batch_contact_patch_torques_device(saip_batch*);  /* [dof][ld] tau_sim of the last integrated substep; NULL without a patch */
/* ---- clearance monitor: link spheres against world-fixed obstacles and against each other, evaluated inside rollouts, so that a
 * sampler can score colliding as well as reaching with no host in the loop.  One attachment per batch.
 *   spheres   n_spheres (1..SAIP_CLEARANCE_MAX_SPHERES), batch-uniform: links[s] a saip_model_link_index value, centres[3 s ..] the centre
 *             in that link's frame, radii[s] >= 0.  A link welded to a movable body is composed with its fixed transform here; a link
 *             welded to the fixed base gives a constant centre.  Centres are in the frame of the robot's base, as a task's pose is.
 *   obstacles n_obstacles (0..SAIP_CLEARANCE_MAX_OBSTACLES), each eight doubles { kind, a[3], b[3], r }: kind 0 a capsule (the segment
 *             a-b with radius r >= 0; a == b is a sphere), kind 1 a half-space (a the unit normal, b[0] the offset; the rest is ignored).
 *             `obstacles` is [O][8] (batch-uniform) or [O][8][B] (per_instance).
 *   pairs     n_pairs (0..SAIP_CLEARANCE_MAX_PAIRS) pairs (s1, s2) of sphere indices, s1 != s2: pairs[2 p], pairs[2 p + 1].
 *   margin    >= 0: distances below it are penalised.
 * Items are numbered k = s O + o for sphere x obstacle, then S O + p for pair p; each has a signed distance (negative: penetration):
 *   capsule     e = b - a, w = c - a, t = e.e > 0 ? clamp((w.e) / (e.e), 0, 1) : 0, |w - t e| - (r_s + r_o)
 *   half-space  (n.c - o) - r_s                pair  |c_s1 - c_s2| - (r_s1 + r_s2)
 * every product and sum rounded once, in that order, and summed over the items in a fixed eight-lane split (csrc/saip_clearance.h;
 * tests/clearance_ref.py restates it in NumPy bit for bit).
 *   readout [8][ld], of the LAST launch: the smallest distance dmin; its item k (as a double); the penalty sum_k max(0, margin - dist_k)^2;
 *        the number of items under the margin; rows 4..6 the centre of the (first) sphere of item k; row 7 the smallest self-pair
 *        distance (+inf without pairs).  An instance with a sphere centre that is not finite is invalid: rows 0, 2, 4..7 NaN, k = -1, count 0.
 *   summaries [4][ld], advanced once per rollout period: min over the periods of dmin (NaN is sticky); sum dt penalty (dt = sim_dt x
 *        substeps); periods with dmin < 0; the index, counted from the last reset, of the first such period, else -1.
 *   while attached, every period of saip_batch_rollout_async gains exactly one launch, behind the period's integration (whichever fused
 *        or un-fused form ran) and in front of the recorder.  saip_batch_clearance_evaluate enqueues the same launch at the resident
 *        state and writes the readout (and the kept centres) only.  _summary_reset sets the summaries to +inf, 0, 0, -1 and the period
 *        counter to 0 on the stream; pair it with a snapshot restore, since the attachment's arrays are configuration, scratch and
 *        readout and not part of a state snapshot.  _set_obstacles_host replaces the table (same shape) and waits; _obstacles_device is
 *        the resident table ([O][8] or [O][8][ld]; NULL without obstacles) for domain randomisation on the device -- what is written
 *        there is not checked.  _centres_device is [3 S][ld] (row 3 s + e), NULL unless keep_centres.
 *   saip_batch_clearance_add_cost: cost[i] = cost[i] + (w_penalty S1[i] + (S0[i] < d_safe ? w_collision : 0)) on the sampler's cost
 *        array (S0, S1: summary rows 0 and 1); a NaN S0 gives a NaN cost.  A cost that is not finite is an invalid sample to
 *        saip_batch_sampler_update, so w_collision = +inf is a hard constraint.
 * Without an attachment every entry point enqueues exactly what it did before.  SAIP_ERR_INVALID_ARGUMENT (the message names the
 * entry): a value that is not finite, a radius below 0, a half-space normal off unit length by more than 1e-6, an unknown kind, a link
 * or sphere index out of range, a pair of a sphere with itself, 0 spheres, 0 obstacles together with 0 pairs, counts above the maxima,
 * a negative margin, a NaN weight.  SAIP_ERR_ORDER: before finalize, a model-only batch, a second _attach, any other entry without an
 * attachment, _set_obstacles_host on an attachment without obstacles, _add_cost without a sampler.  Argument and order errors are
 * reported before the device is needed. */
#define SAIP_CLEARANCE_MAX_SPHERES 32
#define SAIP_CLEARANCE_MAX_OBSTACLES 16
#define SAIP_CLEARANCE_MAX_PAIRS 64
#define SAIP_CLEARANCE_OBSTACLE_WORDS 8
#define SAIP_CLEARANCE_READOUT_ROWS 8
#define SAIP_CLEARANCE_SUMMARY_ROWS 4
#define SAIP_CLEARANCE_CAPSULE 0
#define SAIP_CLEARANCE_HALF_SPACE 1
saip_status saip_batch_clearance_attach(saip_batch*, int n_spheres, const int* links, const double* centres /* [S][3] */, const double* radii,
                                        int n_obstacles, const double* obstacles, int per_instance, int n_pairs, const int* pairs /* [P][2] */,
                                        double margin, int keep_centres);
saip_status saip_batch_clearance_detach(saip_batch*);
saip_status saip_batch_clearance_info(saip_batch*, int* n_spheres, int* n_obstacles, int* per_instance, int* n_pairs, double* margin,
                                      int* keep_centres, long long* period /* monitored since the last reset */);  /* any NULL */
saip_status saip_batch_clearance_set_obstacles_host(saip_batch*, const double* obstacles);
double* saip_batch_clearance_obstacles_device(saip_batch*);  /* NULL when detached or without obstacles */
saip_status saip_batch_clearance_evaluate(saip_batch*);
saip_status saip_batch_clearance_readout_host(saip_batch*, double* out /* [8][B] */);  /* synchronous */
double* saip_batch_clearance_readout_device(saip_batch*);    /* [8][ld]; NULL when detached */
saip_status saip_batch_clearance_summary_host(saip_batch*, double* out /* [4][B] */);  /* synchronous */
double* saip_batch_clearance_summary_device(saip_batch*);    /* [4][ld]; NULL when detached */
saip_status saip_batch_clearance_summary_reset(saip_batch*);
double* saip_batch_clearance_centres_device(saip_batch*);    /* [3 S][ld]; NULL unless keep_centres */
saip_status saip_batch_clearance_add_cost(saip_batch*, double w_penalty, double w_collision, double d_safe);
/* ---- link contact: world-fixed obstacles push back on the robot's link spheres, so that an elbow that meets the table stops there in
 * the simulation.  One attachment per batch; it owns its copies of every table (it shares nothing with the clearance monitor).
 *   spheres    n_spheres (1..SAIP_LINK_CONTACT_MAX_SPHERES), as saip_batch_clearance_attach takes them (batch-uniform, sorted by body here).
 *   obstacles  n_obstacles (1..SAIP_LINK_CONTACT_MAX_OBSTACLES) in the clearance monitor's eight words: [O][8] or [O][8][B] (per_instance).
 *   materials  [O][4] = { k, c, mu, v_s } per obstacle, batch-uniform: stiffness, damping, friction, slip-regularisation speed.
 * Item (s, o) has the monitor's signed distance d and a direction n: the half-space normal, or u / |u| of the capsule (u the vector from the
 * closest axis point to the centre; with |u| == 0, the centre exactly on the axis, there is no direction and the item pushes nothing).  It
 * is active iff d < 0; then with v the velocity of the sphere's centre, vn = n.v:
 *   f_n = max(0, (-k d) - c vn)     v_t = v - vn n     f_t = -(mu f_n) v_t / max(|v_t|, v_s) (0 when mu == 0)     f = f_n n + f_t
 * F_s = sum of f over the active obstacles, acting at the sphere's centre, and tau_sim = u0 + sum_s J_v(c_s)^T F_s, u0 the commanded torques
 * (the plant's actuated torques when a plant is attached; NaN -> 0).  Every product and sum is rounded once, in a fixed order and a fixed
 * eight-lane split (csrc/saip_link_contact.h; tests/link_contact_ref.py restates it in NumPy bit for bit).
 *   while attached, every integration substep of saip_batch_integrate and saip_batch_rollout_async is: the plant launch (if attached), the
 *        link-contact launch, the contact-plane or patch launch (if attached; it builds on link contact's tau_sim), the integrate launch
 *        with the last buffer written.  Neither fused form is used.  _evaluate enqueues one launch at the resident state that writes the
 *        readout (and the kept arrays) only.
 *   readout [8][ld], of the LAST launch: rows 0..2 the net force sum_s F_s; 3 the smallest d over all items; 4 its item s O + o (as a
 *        double, s the caller's sphere index; the lowest among equals); 5 active items; 6 sum f_n; 7 the largest single-item |f|.  An instance
 *        with a sphere centre that is not finite is invalid: rows 0..3, 6, 7 NaN, item -1, count 0, tau_sim = u0.
 *   summaries [4][ld], advanced once per substep: sum dt sum f_n (NaN is sticky); the largest single-item |f|; the largest penetration
 *        max(0, -d); substeps with an active item.  _summary_reset zeroes them on the stream; pair it with a snapshot restore: nothing of
 *        the attachment is state.
 *   keep: _keep_device is [9 S][ld]: centres (row 3 s + e), velocities (3 (S + s) + e), F_s (3 (2 S + s) + e) of the last launch; else NULL.
 *   saip_batch_link_contact_add_cost: cost[i] = cost[i] + (w_impulse S0[i] + w_peak S1[i]) on the sampler's cost; a NaN S0 gives a NaN cost.
 * Limits: an explicit penalty is stable only roughly while k dt^2 / m_eff <~ 1; the force acts at the centre, not at the surface point.
 * Without an attachment every entry point enqueues exactly what it did before.  SAIP_ERR_INVALID_ARGUMENT (the message names the sphere,
 * the obstacle or material, and the word): a NaN anywhere, a value that is not finite, a radius below 0, a half-space normal off unit
 * length by more than 1e-6, an unknown kind, a link index out of range, k, c or mu negative or not finite, mu > 0 with v_s <= 0, 0 spheres
 * or obstacles or counts above the maxima, a NaN weight.  SAIP_ERR_ORDER: before finalize, a model-only batch, a second _attach, any other
 * entry without an attachment, _add_cost without a sampler.  Argument and order errors are reported before the device is needed, and
 * nothing is written on refusal. */
#define SAIP_LINK_CONTACT_MAX_SPHERES 32
#define SAIP_LINK_CONTACT_MAX_OBSTACLES 16
#define SAIP_LINK_CONTACT_OBSTACLE_WORDS 8
#define SAIP_LINK_CONTACT_MATERIAL_WORDS 4
#define SAIP_LINK_CONTACT_READOUT_ROWS 8
#define SAIP_LINK_CONTACT_SUMMARY_ROWS 4
saip_status saip_batch_link_contact_attach(saip_batch*, int n_spheres, const int* links, const double* centres /* [S][3] */, const double* radii,
                                           int n_obstacles, const double* obstacles, const double* materials /* [O][4] */, int per_instance, int keep);
saip_status saip_batch_link_contact_detach(saip_batch*);
saip_status saip_batch_link_contact_info(saip_batch*, int* n_spheres, int* n_obstacles, int* per_instance, int* keep);  /* any NULL */
saip_status saip_batch_link_contact_set_obstacles_host(saip_batch*, const double* obstacles);
saip_status saip_batch_link_contact_set_materials_host(saip_batch*, const double* materials);
double* saip_batch_link_contact_obstacles_device(saip_batch*);  /* [O][8] or [O][8][ld]; NULL when detached */
saip_status saip_batch_link_contact_evaluate(saip_batch*);
saip_status saip_batch_link_contact_readout_host(saip_batch*, double* out /* [8][B] */);  /* synchronous */
double* saip_batch_link_contact_readout_device(saip_batch*);    /* [8][ld]; NULL when detached */
saip_status saip_batch_link_contact_summary_host(saip_batch*, double* out /* [4][B] */);  /* synchronous */
double* saip_batch_link_contact_summary_device(saip_batch*);    /* [4][ld]; NULL when detached */
saip_status saip_batch_link_contact_summary_reset(saip_batch*);
saip_status saip_batch_link_contact_add_cost(saip_batch*, double w_impulse, double w_peak);
double* saip_batch_link_contact_torques_device(saip_batch*);    /* [dof][ld] tau_sim of the last APPLY launch; NULL when detached */
double* saip_batch_link_contact_keep_device(saip_batch*);       /* [9 S][ld]; NULL unless keep */
/* ---- link object: a free rigid body that the robot's link spheres push, the optional second stage of link contact ("push the part to the
 * target" inside a rollout).  At most one per batch; it needs link contact and is detached with it.  The launch with the object replaces
 * the link-contact launch: the launch count of a substep does not change.
 *   state     [13][ld] per instance: p[3] of the body origin (world = the robot's base frame), unit quaternion (w, x, y, z) body to world,
 *             v[3], omega[3] (world frame).  State in the sense of the snapshots: segment link_object.state while attached.  _attach leaves
 *             the body frame on the world frame, at rest; _set_state_host takes [13] (per_instance 0: every instance) or [13][B] and
 *             normalises the quaternion.
 *   inertial  { m, Ix, Iy, Iz } (principal moments in body axes), [4] or [4][B] (per_instance), all > 0 and finite.
 *   shape     n_spheres (1..SAIP_LINK_OBJECT_MAX_SPHERES) of { centre[3] in the body frame, radius >= 0 }, batch-uniform; material[4] =
 *             { k, c, mu, v_s } of robot-object contact, under the rules of a link-contact material row.
 * Every APPLY substep (saip_batch_integrate, every rollout substep), at the state of that substep: object sphere p has c_p = p + R r_p,
 * v_p = v + omega x (c_p - p).  Robot sphere s against object sphere p is the link-contact item against the sphere obstacle (c_p, radius_p)
 * with the object's material and the velocity v_s - v_p: f acts on the robot sphere (F_s sums the world obstacles first, then p = 0..P-1),
 * -f on the object at c_p.  Object sphere p meets every link-contact obstacle with that obstacle's material.  The body integrates
 * m g + the world items + the reactions with semi-implicit Euler (csrc/saip_link_object.h has the order of every operation;
 * tests/link_object_ref.py restates it in NumPy bit for bit).  The link-contact readout and summaries keep speaking of the world obstacles
 * alone; the robot's torque loop runs when a world item or an object item is active.  _evaluate never advances the object.
 *   readout [12][ld] of the LAST launch: 0..2 net force of the robot on the object; 3..5 its moment about p; 6..8 net force of the world on
 *        the object; 9 the smallest robot-object distance; 10 its item s P + p (s the caller's robot sphere; lowest among equals); 11 active
 *        robot-object items.  An instance with a robot sphere centre or an object state word that is not finite is invalid: every row NaN,
 *        tau_sim = u0, the state is not written.
 *   summaries [4][ld], advanced once per substep: sum dt sum f_n over the robot-object items (NaN is sticky); the largest robot-object
 *        penetration; the largest object-world penetration; substeps with an active robot-object item.
 *   saip_batch_link_object_add_cost: cost[i] += w_pos |p - target_p|^2 + w_ori (1 - (q . q_t)^2) (the second term only with a target
 *        quaternion, normalised here); a state that is not finite costs +inf.
 * SAIP_ERR_INVALID_ARGUMENT (the message names the sphere, the word and the instance): a centre or radius that is not finite, a radius below
 * 0, a material word against the rules, an inertial word that is not > 0 and finite, a zero or non-finite quaternion, 0 spheres or more than
 * the maximum, a null table, a NaN weight, a target that is not finite.  SAIP_ERR_ORDER: before finalize, a model-only batch, _attach without
 * link contact or twice, any other entry without an attachment, _add_cost without a sampler.  Argument and order errors are reported before
 * the device is needed, and nothing is written on refusal. */
#define SAIP_LINK_OBJECT_MAX_SPHERES 8
#define SAIP_LINK_OBJECT_STATE_ROWS 13
#define SAIP_LINK_OBJECT_INERTIAL_WORDS 4
#define SAIP_LINK_OBJECT_READOUT_ROWS 12
#define SAIP_LINK_OBJECT_SUMMARY_ROWS 4
saip_status saip_batch_link_object_attach(saip_batch*, int n_spheres, const double* centres /* [P][3] */, const double* radii, const double* material /* [4] */,
                                          const double* inertial /* [4] or [4][B] */, int per_instance);
saip_status saip_batch_link_object_detach(saip_batch*);
saip_status saip_batch_link_object_info(saip_batch*, int* n_spheres, int* per_instance);  /* any NULL */
saip_status saip_batch_link_object_set_state_host(saip_batch*, const double* state /* [13] or [13][B] */, int per_instance);
saip_status saip_batch_link_object_state_host(saip_batch*, double* out /* [13][B] */);  /* synchronous */
double* saip_batch_link_object_state_device(saip_batch*);      /* [13][ld]; NULL when detached */
saip_status saip_batch_link_object_set_inertial_host(saip_batch*, const double* inertial);
saip_status saip_batch_link_object_readout_host(saip_batch*, double* out /* [12][B] */);  /* synchronous */
double* saip_batch_link_object_readout_device(saip_batch*);    /* [12][ld]; NULL when detached */
saip_status saip_batch_link_object_summary_host(saip_batch*, double* out /* [4][B] */);  /* synchronous */
double* saip_batch_link_object_summary_device(saip_batch*);    /* [4][ld]; NULL when detached */
saip_status saip_batch_link_object_summary_reset(saip_batch*);
saip_status saip_batch_link_object_add_cost(saip_batch*, const double* target_p /* [3] */, double w_pos, const double* target_quat /* [4] or NULL */, double w_ori);
/* ---- environment schedules: moving obstacles and contact surfaces inside rollouts.  What goal schedules are to the goals: the obstacle
 * table of the clearance monitor, the single-point contact planes and the planes of a contact patch become functions of the rollout
 * period, written from keyframes resident on the device by ONE launch at the head of every period of saip_batch_rollout_async.  At most
 * SAIP_ENV_MAX_SCHEDULES per batch, one per table.
 *   target    SAIP_ENV_TARGET_OBSTACLES, _PLANES, or _PATCH (the planes of the patch on `task`; -1: the first patch; ignored otherwise).
 *   items     the schedule covers items [first, first + n_items) of the table; the others are never written.
 *   keyframes [K][n_items][W], or [K][n_items][W][B] when the target table is per instance (the layout of the target's own _set_*_host call
 *             with a leading keyframe index).  W = 8 for an obstacle; W = SAIP_ENV_PLANE_WORDS for a plane: the eight plane words, a
 *             surface velocity u[3] in the base frame, and one reserved word that must be 0.  Plane normals are normalised as the plane
 *             table's are.
 *   timing    the schedule has its own period counter c (0 after _attach; _rewind sets it to any period, so that a receding-horizon
 *             round starts its prediction at the current time).  A schedule that sees the period index x reads i = x / stride and
 *             s = (x % stride) / stride, the last keyframe held.  Contact targets see x = c: the planes are held through the period's
 *             substeps, as a goal is.  The clearance target sees x = c + 1: the monitor runs behind the period's integration and
 *             looks at the obstacle at the time of the state it looks at.
 *   modes     SAIP_ENV_HOLD writes keyframe i.  SAIP_ENV_LINEAR writes a + s (b - a) per word, the difference, product and sum each
 *             rounded once; at s == 0 the row is a exactly; an obstacle's kind is a's; a unit normal (half-space, plane) is interpolated
 *             the same way and divided by its length.  csrc/saip_env_schedule.h; tests/env_schedule_ref.py restates it bit for bit.
 *   velocity  for every scheduled plane the launch also writes { v_p[3], w_n } to the velocity table [P][4] / [P][4][ld]:
 *             v_p = u + w_n n, w_n = (o_b - o_a) / (stride T) in LINEAR between two keyframes (T = sim_dt x substeps), 0 in HOLD and
 *             past the last keyframe.  The rotation of a normal contributes no velocity.  While the planes of a contact attachment have
 *             a schedule, its SENSE and APPLY launches (rollouts, saip_batch_integrate, _sense) take v - v_p in place of the point's
 *             velocity in damping and friction; with v_p = 0 they give the bits of the static planes.
 * saip_batch_step_async, saip_batch_integrate and saip_batch_clearance_evaluate apply no schedule: they read tables and velocities as last
 * written.  Without a schedule every entry point enqueues exactly what it did before.  A state snapshot is unchanged: tables are
 * configuration; pair a restore with _rewind(period).  Detaching the contact planes, a patch or the clearance monitor releases the schedule
 * on its table first; _set_planes_host / _set_obstacles_host on a scheduled table return SAIP_ERR_ORDER.
 * SAIP_ERR_ORDER: the target is not attached, a second schedule on a table, any other entry without that schedule.
 * SAIP_ERR_INVALID_ARGUMENT (the message says what): unknown target or mode, n_keyframes < 1, stride < 1, null keyframes, an item range
 * outside the table, a word that is not finite, a reserved word that is not 0, a plane the plane table would refuse, a half-space
 * normal off unit length by more than 1e-6, an obstacle whose kind differs between keyframes, in LINEAR two consecutive normals with
 * n_a . n_b < 0, a negative period.  Argument and order errors are reported before the device is needed. */
#define SAIP_ENV_MAX_SCHEDULES 4
#define SAIP_ENV_PLANE_WORDS 12
#define SAIP_ENV_TARGET_OBSTACLES 0
#define SAIP_ENV_TARGET_PLANES 1
#define SAIP_ENV_TARGET_PATCH 2
#define SAIP_ENV_HOLD 0
#define SAIP_ENV_LINEAR 1
saip_status saip_batch_env_schedule_attach(saip_batch*, int target, int task, int first, int n_items, const double* keyframes, int n_keyframes,
                                           int stride, int mode);
saip_status saip_batch_env_schedule_detach(saip_batch*, int target /* -1: every schedule */, int task);
saip_status saip_batch_env_schedule_rewind(saip_batch*, long long period);
saip_status saip_batch_env_schedule_info(saip_batch*, int target, int task, int* first, int* n_items, int* n_keyframes, int* stride, int* mode,
                                         int* per_instance, long long* period);  /* any NULL */
double* saip_batch_env_schedule_keyframes_device(saip_batch*, int target, int task);  /* NULL without that schedule */
double* saip_batch_env_schedule_velocity_device(saip_batch*, int target, int task);   /* [P][4] or [P][4][ld]; NULL for obstacles */
/* ---- plant model: what stands between the commanded torques and the integrator when the robot is not the controller's model --
 * actuator gain, offset and saturation, viscous and Coulomb friction, penalty joint stops and external wrenches on links.  One attachment
 * per batch.  Nothing in it is state: it is configuration plus a host-side period counter, not part of a state snapshot.
 *   joints    SAIP_PLANT_JOINT_WORDS doubles per joint { gain, bias, tau_max, fv, fc, v_s, q_lo, q_hi, k_stop, c_stop }: `joint_table` is
 *             [dof][10] (batch-uniform) or [dof][10][B] (per_instance_joints); NULL: neutral rows { 1, 0, +inf, 0, 0, 0, q_lo, q_hi, 0, 0 }
 *             with q_lo, q_hi the model's joint limits.  With t the commanded torque of the joint:
 *               u0 = t == t ? t : 0        u1 = gain u0 + bias        u2 = min(max(u1, -tau_max), tau_max)
 *               fr = fv dq + (fc > 0 ? (fc dq) / max(|dq|, v_s) : 0)
 *               st = q < q_lo ? max(0, k_stop (q_lo - q) - c_stop dq) : q > q_hi ? -max(0, k_stop (q - q_hi) + c_stop dq) : 0
 *               tau_act = (u2 - fr) + st
 *   wrenches  n_wrenches (0..SAIP_PLANT_MAX_WRENCHES), each with a batch-uniform site: links[k] a saip_model_link_index value, points[3 k ..]
 *             a point in that link's frame, frames[k] SAIP_PLANT_FRAME_WORLD or _LINK, the frame F and M are given in (world: the frame
 *             of the robot's base, as a task's pose is).  `wrench_table` is SAIP_PLANT_WRENCH_WORDS doubles per wrench { F[3], M[3],
 *             p_start, p_end }, [W][8] or [W][8][B] (per_instance_wrenches).  A wrench acts in period p when p_start <= p < p_end (p_end =
 *             +inf: for ever); it adds aw . ((p - o_j) x F + M) (revolute) or aw . F (prismatic) to tau_act of every ancestor joint j of
 *             the link, the wrenches in table order.  F = (0, 0, -m g) for ever is the weight of a carried payload.
 *   summaries [4][ld]: sum dt sum_j |fr_j dq_j|; the largest |u1 - u2| so far; substeps in which a joint clipped or a stop acted;
 *             sum dt sum x dq_j over what the wrenches added (x) to the joints.
 * Every product and sum is rounded once, in the order written; max and min return their first argument on a tie (csrc/saip_plant.h;
 * tests/plant_ref.py restates it in NumPy bit for bit).
 *   while attached, every integration substep of saip_batch_integrate and saip_batch_rollout_async is { plant launch, the contact or patch
 *        APPLY launch if one is attached (reading tau_act in place of the commanded torques), integrate launch with one substep reading
 *        the last buffer written }, and a rollout uses neither fused form.  The period counter starts at 0, advances once per
 *        saip_batch_integrate call and once per rollout period, and is set by _set_period (pair it with a snapshot restore).  The
 *        recorder keeps logging the commanded torques.
 *   saip_batch_plant_randomize fills the per-instance tables on the device: word w (10 j + k of a joint, 8 k + e of a wrench) of instance
 *        i is lo[w] + u (hi[w] - lo[w]), u = the first uniform of Philox4x32-10 at counter (i, w, table, round) (table 0 joints, 1
 *        wrenches) under the key `seed`; lo == hi gives lo exactly; p_start and p_end are floored.  lo / hi are host tables [dof][10] and
 *        [W][8]; a NULL pair leaves that table alone.  Both bounds must be valid tables, and so must what can be drawn between them.
 *   _set_joints_host / _set_wrenches_host replace a table (same shape) and wait; _joints_device / _wrenches_device are the resident
 *        tables ([dof][10] or [dof][10][ld], [W][8] or [W][8][ld]; what is written there is not checked); _torques_device is tau_act
 *        [dof][ld] of the last substep.
 * Without an attachment every entry point enqueues exactly what it did before.  SAIP_ERR_INVALID_ARGUMENT (the message names the entry,
 * the joint or wrench and the word): a NaN anywhere; gain, bias, fv, fc, k_stop, c_stop, F or M not finite; tau_max, fv, fc, k_stop or
 * c_stop below 0; fc > 0 with v_s <= 0; q_lo > q_hi; a link index out of range, a point that is not finite, an unknown frame, a count
 * above the maximum; _randomize of a batch-uniform table.  SAIP_ERR_ORDER: before finalize, a model-only batch, a second _attach, any
 * other entry without an attachment.  Argument and order errors are reported before the device is needed. */
#define SAIP_PLANT_JOINT_WORDS 10
#define SAIP_PLANT_WRENCH_WORDS 8
#define SAIP_PLANT_MAX_WRENCHES 4
#define SAIP_PLANT_SUMMARY_ROWS 4
#define SAIP_PLANT_FRAME_WORLD 0
#define SAIP_PLANT_FRAME_LINK 1
saip_status saip_batch_plant_attach(saip_batch*, const double* joint_table /* NULL = neutral */, int per_instance_joints, int n_wrenches,
                                    const int* links, const double* points /* [W][3] */, const int* frames, const double* wrench_table,
                                    int per_instance_wrenches);
saip_status saip_batch_plant_detach(saip_batch*);
saip_status saip_batch_plant_info(saip_batch*, int* per_instance_joints, int* n_wrenches, int* per_instance_wrenches, long long* period);  /* any NULL */
saip_status saip_batch_plant_set_joints_host(saip_batch*, const double* joint_table);
saip_status saip_batch_plant_set_wrenches_host(saip_batch*, const double* wrench_table);
saip_status saip_batch_plant_randomize(saip_batch*, unsigned long long seed, long long round, const double* joint_lo, const double* joint_hi,
                                       const double* wrench_lo, const double* wrench_hi);
saip_status saip_batch_plant_set_period(saip_batch*, long long period);
saip_status saip_batch_plant_summary_host(saip_batch*, double* out /* [4][B] */);  /* synchronous */
saip_status saip_batch_plant_summary_reset(saip_batch*);
double* saip_batch_plant_joints_device(saip_batch*);    /* NULL when detached */
double* saip_batch_plant_wrenches_device(saip_batch*);  /* NULL when detached or without wrenches */
double* saip_batch_plant_torques_device(saip_batch*);   /* [dof][ld]; NULL when detached */
double* saip_batch_plant_summary_device(saip_batch*);   /* [4][ld]; NULL when detached */
/* ---- actuation chain: the optional second stage of the plant model, the command-side twin of the sensing chain below.  Per joint it
 * stands between the commanded torque and the plant's joint arithmetic: a delay line of up to SAIP_PLANT_CHAIN_MAX_DEPTH control periods,
 * then a slew-rate limit, then a first-order lag.  Everything behind it (gain, bias, tau_max, friction, stops, wrenches, the summaries, the
 * contact launch, the integrator) keeps its arithmetic and sees the chain's output in place of the commanded torque.  Attached only while a
 * plant model is attached (an all-neutral plant table is a valid carrier); saip_batch_plant_detach detaches the chain first.  Its STATE is
 * part of a state snapshot.
 *   table     SAIP_PLANT_CHAIN_WORDS doubles per joint { delay, rate_max, tau_lag }: [dof][3] (batch-uniform) or [dof][3][B] (per_instance);
 *             NULL: neutral rows { 0, +inf, 0 }, which hand the plant the command bit for bit (a NaN command as 0, as the plant reads it).
 *             delay is integer-valued in 0..depth (control periods), rate_max > 0 in torque units per second (+inf: no limit), tau_lag
 *             >= 0 and finite, the time constant in seconds (0: no lag).
 *   substep   one per (joint, instance) per integration substep of length dt; advance = the first substep of a period:
 *             x0 = t == t ? t : 0;   d = (int)delay
 *             if (advance) { unless primed: every tap = x0, x_held = y_rate = y_lag = x0, primed = 1;
 *                            x_held = d ? tap[d-1] : x0;   taps 1..d-1 shift by one, tap 0 takes x0 }
 *             step = rate_max dt;   y_rate = rate_max < +inf ? y_rate + min(max(x_held - y_rate, -step), step) : x_held
 *             y_lag = tau_lag > 0 ? y_lag + (dt / (tau_lag + dt)) (y_rate - y_lag) : y_rate;   the plant's joint gets y_lag
 *             every product, sum and quotient rounded once, in the order written (csrc/saip_plant_chain.h; tests/plant_chain_ref.py).
 *             The delay counts control periods (one saip_batch_integrate call or one rollout period is one period); the rate limit and
 *             the lag run every substep.  No extra launch: while attached, saip_plant_apply<*, true> is enqueued where saip_plant_apply is.
 *   state     per (joint, instance): taps [dof][depth][ld] (absent at depth 0), filt [dof][3][ld] { x_held, y_rate, y_lag }, primed
 *             [dof][ld] (int32); zeroed at attach, freed at detach, listed by a snapshot as plant.chain.taps / .filt / .primed while
 *             attached.  A snapshot of another chain layout is refused with ORDER, the segment named.  A restore does not re-prime: primed
 *             travels with the column.  _chain_reset clears primed on the stream.  A new table keeps the state.
 *   _chain_randomize fills the per-instance table: word w = 3 j + k of instance i is lo[w] + u (hi[w] - lo[w]) as in
 *             saip_batch_plant_randomize, table id 9; lo == hi gives lo exactly (+inf stays +inf); delay is then rounded, floor(x + 0.5),
 *             and clamped to 0..depth.
 *   _chain_state_host: taps [dof][depth][B], filt [dof][3][B], primed [dof][B] (any may be NULL), synchronous: for tests and debugging.
 * The recorder keeps logging commanded torques; saip_batch_plant_torques_device shows the actuated ones.
 * Errors: INVALID_ARGUMENT for a depth outside 0..8, a bad table word (the message names the joint, the word and, per instance, the
 * instance); ORDER before saip_batch_finalize, on a model-only batch, without a plant model, on a second attach and from every other _chain
 * entry without a chain (_chain_info needs the plant model only).  Argument and order errors are reported before the device is needed;
 * nothing is written on a refusal. */
#define SAIP_PLANT_CHAIN_WORDS 3
#define SAIP_PLANT_CHAIN_MAX_DEPTH 8
#define SAIP_PLANT_TABLE_CHAIN 9
saip_status saip_batch_plant_chain_attach(saip_batch*, const double* table /* NULL = neutral */, int per_instance, int depth);
saip_status saip_batch_plant_chain_detach(saip_batch*);
saip_status saip_batch_plant_chain_info(saip_batch*, int* attached, int* per_instance, int* depth, size_t* state_bytes);  /* any NULL */
saip_status saip_batch_plant_chain_set_table_host(saip_batch*, const double* table);
saip_status saip_batch_plant_chain_randomize(saip_batch*, unsigned long long seed, long long round, const double* lo, const double* hi);  /* per-instance table only */
saip_status saip_batch_plant_chain_reset(saip_batch*);
double* saip_batch_plant_chain_table_device(saip_batch*);  /* NULL when detached */
saip_status saip_batch_plant_chain_state_host(saip_batch*, double* taps, double* filt, int* primed);  /* synchronous */
saip_status saip_batch_plant_chain_state_device(saip_batch*, double** taps, double** filt, int** primed);  /* the arrays, [rows][ld]; taps NULL at depth 0 */
/* ---- plant inertia: the inertial parameters of the SIMULATED robot, per instance.  While attached, the resident integrator (and nothing
 * else: the cycle kernels, the model queries and everything the controller computes keep the batch-uniform model) reads mass, centre of
 * mass and inertia of every movable body from a resident table.  One attachment per batch; configuration only, not part of a state
 * snapshot, so every instance keeps its robot across a restore.
 *   rows      SAIP_INERTIA_ROW_WORDS doubles per movable body, in the model's body order { m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz }:
 *             the centre of mass in the body frame, the inertia about it in body axes.  [dof][10] (batch-uniform) or [dof][10][B]
 *             (per_instance); NULL: the model's own rows.
 *   parts     _set_parts_host composes the rows on the device from scaled links plus payloads.  A body's part is SAIP_INERTIA_BODY_WORDS
 *             doubles { s, dx, dy, dz }: m' = s m, I' = s I, c' = c + d (m, c, I the model's); `bodies` is [dof][4] or [dof][4][B]
 *             (per_instance_bodies), NULL: { 1, 0, 0, 0 }.  A payload is SAIP_INERTIA_PAYLOAD_WORDS doubles { m_p, c_p[3], hx, hy, hz }, a
 *             uniform box of half-extents h aligned with the frame of its site link and centred at c_p in it, I_p = m_p / 3 diag(hy^2 +
 *             hz^2, hx^2 + hz^2, hx^2 + hy^2); `payloads` is [P][7] or [P][7][B] (per_instance_payloads), NULL: no mass.  The sites are
 *             fixed by _attach: payload_links[p] a saip_model_link_index value (batch-uniform); a link welded to a movable body is
 *             composed with its fixed transform (p_f, R_f) into that body's frame.  With PA(d) = (d.d) 1 - d d^T, over the payloads
 *             with m_p > 0 on the body in table order:
 *               m = m' + sum m_p     c = (m' c' + sum m_p (p_f + R_f c_p)) / m
 *               I = I' + m' PA(c' - c) + sum (R_f I_p R_f^T + m_p PA(p_f + R_f c_p - c))
 *             A body without such a payload takes m', c', I' as they are.  Every product, sum and quotient is rounded once, in the order
 *             written (csrc/saip_inertia.h; tests/inertia_ref.py restates it in NumPy bit for bit).
 *   saip_batch_inertia_randomize draws the parts on the device and composes them: word w (4 j + k of a body, 7 p + e of a payload) of
 *             instance i is lo[w] + u (hi[w] - lo[w]) clamped to the interval, u = the first uniform of Philox4x32-10 at counter (i, w,
 *             table, round) (table 2 bodies, 3 payloads) under the key `seed`; lo == hi gives lo exactly.  lo / hi are host tables
 *             [dof][4] and [P][7]; a NULL pair stands for the neutral words.  Per-instance tables only.
 *   while attached, saip_batch_integrate and every rollout period pass the table to the integrate launch (on the per-substep sequence
 *             behind a plant or contact attachment too), and a rollout uses neither fused form.  A payload in the table carries its own
 *             weight: no plant wrench is needed for it.
 *   _set_rows_host replaces the table (same shape) and waits; _rows_host reads it back ([dof][10] or [dof][10][B], synchronous);
 *             _rows_device is the resident table ([dof][10] or [dof][10][ld]; what is written there is not checked).
 * Without an attachment every entry point enqueues exactly what it did before.  SAIP_ERR_INVALID_ARGUMENT (the message names the entry,
 * the body or payload, the word and the instance; nothing is written): a value that is not finite; m < 0; an inertia whose smallest
 * eigenvalue is below -1e-12 max(1, trace) (the triangle inequality is not enforced); s <= 0, m_p < 0 or a half-extent < 0, in a table or
 * in a bound; a body whose mass can come out as 0 where the model's is positive; more than SAIP_INERTIA_MAX_PAYLOADS payloads, a link index
 * out of range or a link welded to the fixed base; per-instance parts or a draw onto a batch-uniform table.  SAIP_ERR_ORDER: before
 * finalize, a model-only batch, a second _attach, any other entry without an attachment.  Argument and order errors are reported before
 * the device is needed. */
#define SAIP_INERTIA_ROW_WORDS 10
#define SAIP_INERTIA_BODY_WORDS 4
#define SAIP_INERTIA_PAYLOAD_WORDS 7
#define SAIP_INERTIA_MAX_PAYLOADS 2
saip_status saip_batch_inertia_attach(saip_batch*, const double* rows /* NULL = the model's */, int per_instance, int n_payloads, const int* payload_links);
saip_status saip_batch_inertia_detach(saip_batch*);
saip_status saip_batch_inertia_info(saip_batch*, int* per_instance, int* n_payloads, int* payload_bodies /* [P] movable body of each site */,
                                    double* payload_frames /* [P][12]: p_f (3), R_f (9, row-major) of each site link in that body */);  /* any NULL */
saip_status saip_batch_inertia_set_rows_host(saip_batch*, const double* rows);
saip_status saip_batch_inertia_set_parts_host(saip_batch*, const double* bodies, int per_instance_bodies, const double* payloads, int per_instance_payloads);
saip_status saip_batch_inertia_randomize(saip_batch*, unsigned long long seed, long long round, const double* body_lo, const double* body_hi,
                                         const double* payload_lo, const double* payload_hi);
saip_status saip_batch_inertia_rows_host(saip_batch*, double* out /* [dof][10] or [dof][10][B] */);  /* synchronous */
double* saip_batch_inertia_rows_device(saip_batch*);     /* NULL when detached */
/* ---- sensing model: what stands between the simulated robot and what the controller reads of it -- a constant offset, Gaussian noise and
 * quantisation on every joint position and velocity and on the sensed wrench of up to SAIP_SENSE_MAX_WRENCH_TASKS motion-force tasks.  One
 * attachment per batch.  Nothing in it is state: it is configuration plus a host-side period counter, not part of a state snapshot.
 *   measured  m = x + off;  if (sigma > 0) m = m + sigma z;  if (res > 0) m = res rint(m / res)   (round half to even)
 *             every product and sum rounded once, in the order written (csrc/saip_sense.h; tests/sensing_ref.py restates it in NumPy).  A
 *             non-finite x goes through the same arithmetic: a NaN state stays NaN and the cycle flags the instance as it does unattached.
 *   joints    SAIP_SENSE_JOINT_WORDS doubles per joint { q_off, q_res, q_sigma, dq_off, dq_res, dq_sigma }: `joint_table` is [dof][6]
 *             (batch-uniform) or [dof][6][B] (per_instance_joints); NULL: neutral rows, all zeros
 *   wrenches  n_wrench_tasks (0..2) motion-force tasks `tasks`, each with SAIP_SENSE_WRENCH_WORDS doubles: 6 axes (F then M, the frame the
 *             simulated sensor writes in) x { off, res, sigma }; `wrench_tables` is [S][6][3] or [S][6][3][B] (per_instance_wrenches).  They
 *             act on goal rows 30..35 of the task, directly behind every launch of a simulated sensor that writes them (contact planes,
 *             contact patches; in a rollout period and in the standalone _sense entries).  The sensor rewrites the rows it perturbs, so a
 *             repeated _sense does not stack the perturbation; a table for a task whose sensor is never simulated is inert.
 *   noise     z: the standard normals of Philox4x32-10 (the rollout sampler's generator) at counter (instance, row, table << 16, period)
 *             under `seed`: table 6, row j gives (z of q_j, z of dq_j); table 7, row 3 slot + a / 2 gives the z of wrench axes a (even) and
 *             a + 1 of the task in slot `slot`.  period: the counter of _info, advanced by every rollout period and every
 *             saip_batch_integrate, set by _set_period (pair it with saip_batch_restore_state: it is not part of a snapshot).
 *   while attached, every non-diagnostic cycle launch (the whole-controller cycle, its slow-path launches, the per-task entries,
 *             re-initialisation, the pose and task-diagnostics queries) and the internal OTGs read q_meas, dq_meas in place of the resident
 *             state; diagnostic launches, the recorder, the model queries, contact, clearance, plant and the integrator keep reading the true
 *             state.  The measurement is taken in front of the first such launch after the state, the tables, the seed or the period
 *             changed: once per rollout period (there in one launch with the wrench part), and two cycles at one state see one
 *             measurement.  A rollout uses neither fused form.  The true state is never written.
 *   saip_batch_sensing_randomize fills the per-instance tables on the device: word w (6 j + k of a joint, 18 s + 3 a + e of a wrench) of
 *             instance i is lo[w] + u (hi[w] - lo[w]) clamped to the interval, u the first uniform of Philox4x32-10 at counter (i, w,
 *             table, round) (table 4 joints, 5 wrenches); lo == hi gives lo exactly.
 *   _measure  enqueues the measurement of q, dq now: for host-driven loops and after writes through the _device pointers, which are
 *             neither checked nor noticed.  _measured_host: the measured copy, [dof][B] each (either may be NULL), synchronous.
 * Errors: ORDER before saip_batch_finalize, on a model-only batch, on a second attach and from every other entry without an attachment;
 * INVALID_ARGUMENT for a NaN or non-finite word, a negative res or sigma (the message names the joint or the task and axis, the word and,
 * for per-instance tables, the instance), a task that is not a motion-force task or is named twice, a period outside 0 .. 2^32 - 1.
 * Argument and order errors are reported before the device is needed; nothing is written on a refusal. */
#define SAIP_SENSE_JOINT_WORDS 6
#define SAIP_SENSE_AXIS_WORDS 3
#define SAIP_SENSE_WRENCH_WORDS 18
#define SAIP_SENSE_MAX_WRENCH_TASKS 2
#define SAIP_SENSE_TABLE_JOINTS 4
#define SAIP_SENSE_TABLE_WRENCHES 5
#define SAIP_SENSE_TABLE_JOINT_NOISE 6
#define SAIP_SENSE_TABLE_WRENCH_NOISE 7
saip_status saip_batch_sensing_attach(saip_batch*, const double* joint_table /* NULL = neutral */, int per_instance_joints, int n_wrench_tasks,
                                      const int* tasks, const double* wrench_tables, int per_instance_wrenches, unsigned long long seed);
saip_status saip_batch_sensing_detach(saip_batch*);
saip_status saip_batch_sensing_info(saip_batch*, int* per_instance_joints, int* n_wrench_tasks, int* per_instance_wrenches, long long* period);  /* any NULL */
saip_status saip_batch_sensing_set_joints_host(saip_batch*, const double* joint_table);
saip_status saip_batch_sensing_set_wrenches_host(saip_batch*, const double* wrench_tables);
saip_status saip_batch_sensing_seed(saip_batch*, unsigned long long seed);
saip_status saip_batch_sensing_set_period(saip_batch*, long long period);  /* 0 <= period < 2^32 */
saip_status saip_batch_sensing_randomize(saip_batch*, unsigned long long seed, long long round, const double* joint_lo, const double* joint_hi,
                                         const double* wrench_lo, const double* wrench_hi);  /* per-instance tables only */
saip_status saip_batch_sensing_measure(saip_batch*);
saip_status saip_batch_sensing_measured_host(saip_batch*, double* q /* [dof][B] */, double* dq);  /* synchronous */
double* saip_batch_sensing_joints_device(saip_batch*);       /* NULL when detached */
double* saip_batch_sensing_wrenches_device(saip_batch*);     /* NULL when detached or without wrench tasks */
double* saip_batch_sensing_measured_q_device(saip_batch*);   /* [dof][ld]; NULL when detached */
double* saip_batch_sensing_measured_dq_device(saip_batch*);  /* [dof][ld]; NULL when detached */
/* ---- sensing chain: the optional second stage of the sensing model, per joint: a delay line of up to SAIP_SENSE_CHAIN_MAX_DEPTH samples, an
 * optional finite-difference velocity and a first-order low-pass between the measured sample (q_m, dq_m) above and what the controller
 * reads.  Attached only while a sensing model is attached (an all-zero sensing table is a valid carrier); saip_batch_sensing_detach detaches
 * the chain first.  It is the one attachment with STATE, and that state is part of a state snapshot.
 *   table     SAIP_SENSE_CHAIN_WORDS doubles per joint { delay, vel_mode, a_q, a_dq }: [dof][4] (batch-uniform) or [dof][4][B] (per_instance);
 *             NULL: neutral rows, all zeros (no delay, measured dq, no filter), which return the sensing model's output bit for bit.
 *             delay is integer-valued in 0..depth, vel_mode 0 (measured dq) or 1 (finite difference), a_q and a_dq in [0, 1] (0: no filter).
 *             For a cutoff f_c in Hz the facades offer a = 1 - exp(-2 pi f_c sample_time); the kernel never sees a frequency.
 *   sample    d = (int)delay;  unless primed: every tap = (q_m, dq_m), q_prev = y_q = q_m, y_dq = dq_m, primed = 1
 *             x = d ? tap_q[d-1] : q_m;  v = d ? tap_dq[d-1] : dq_m;   taps 1..d-1 shift by one, tap 0 takes (q_m, dq_m)
 *             if (vel_mode == 1) { v = (x - q_prev) / sample_time;  q_prev = x }        (the first sample gives 0)
 *             y_q = a_q > 0 ? y_q + a_q (x - y_q) : x;   y_dq = a_dq > 0 ? y_dq + a_dq (v - y_dq) : v;   the controller reads (y_q, y_dq)
 *             every product, sum and quotient rounded once, in the order written (csrc/saip_sense_chain.h; tests/sensing_chain_ref.py).
 *   every JOINTS launch of the sensing model is one sample: one per state change in front of the first launch that reads the controller's
 *             state, one per rollout period, and one per saip_batch_sensing_measure (two calls at one state are two samples).  While
 *             attached, saip_sense_chain_apply is enqueued wherever saip_sense_apply would be; a rollout period keeps one measurement launch.
 *   state     per (joint, instance): taps [dof][2][depth][ld] (absent at depth 0), filt [dof][3][ld] { q_prev, y_q, y_dq }, primed [dof][ld]
 *             (int32); zeroed at attach, freed at detach, listed by a snapshot as sense.chain.taps / .filt / .primed while attached.  A
 *             snapshot of another chain layout (not attached, another depth, another attachment) is refused with ORDER, the segment named.
 *             A restore does not re-prime: primed travels with the column.  _chain_reset clears primed on the stream.
 *   _chain_randomize fills the per-instance table: word w = 4 j + k of instance i is lo[w] + u (hi[w] - lo[w]) as in
 *             saip_batch_sensing_randomize, table id 8; delay and vel_mode are then rounded, floor(x + 0.5), and clamped to their range.
 *   _chain_state_host: taps [dof][2][depth][B], filt [dof][3][B], primed [dof][B] (any may be NULL), synchronous: for tests and debugging.
 * Errors: INVALID_ARGUMENT for a depth outside 0..8, a sample time that is not finite and positive, a bad table word (the message names the
 * joint, the word and, per instance, the instance); ORDER before saip_batch_finalize, on a model-only batch, without a sensing model, on a
 * second attach and from every other _chain entry without a chain (_chain_info needs the sensing model only).  Argument and order errors
 * are reported before the device is needed; nothing is written on a refusal. */
#define SAIP_SENSE_CHAIN_WORDS 4
#define SAIP_SENSE_CHAIN_MAX_DEPTH 8
#define SAIP_SENSE_TABLE_CHAIN 8
saip_status saip_batch_sensing_chain_attach(saip_batch*, const double* table /* NULL = neutral */, int per_instance, int depth, double sample_time);
saip_status saip_batch_sensing_chain_detach(saip_batch*);
saip_status saip_batch_sensing_chain_info(saip_batch*, int* attached, int* per_instance, int* depth, double* sample_time, size_t* state_bytes);  /* any NULL */
saip_status saip_batch_sensing_chain_set_table_host(saip_batch*, const double* table);
saip_status saip_batch_sensing_chain_randomize(saip_batch*, unsigned long long seed, long long round, const double* lo, const double* hi);  /* per-instance table only */
saip_status saip_batch_sensing_chain_reset(saip_batch*);
double* saip_batch_sensing_chain_table_device(saip_batch*);  /* NULL when detached */
saip_status saip_batch_sensing_chain_state_host(saip_batch*, double* taps, double* filt, int* primed);  /* synchronous */
saip_status saip_batch_sensing_chain_state_device(saip_batch*, double** taps, double** filt, int** primed);  /* the arrays, [rows][ld]; taps NULL at depth 0 */
/* ---- resident guards: event-triggered phases and goal switching inside rollouts.  The policy of a rollout stops being open loop in time:
 * every instance carries a phase 0 .. P-1, a table of guards (transitions) moves it on what the instance itself senses, and a table of
 * phases says what a phase does to the goal of ONE motion-force task ("descend until touch, then stop, then retract 5 cm").  One
 * attachment per batch.  Task parametrisation stays batch-uniform: a guard switches the goal, not the control law.
 *   guards   n_guards (1..SAIP_GUARD_MAX_GUARDS) rows of SAIP_GUARD_WORDS doubles { from, to, signal, axis, cmp, threshold, hold, blank }:
 *            [G][8], or [G][8][B] with per_instance.  All words but threshold are integer-valued.
 *            signal  SAIP_GUARD_PERIODS     periods the instance has spent in its phase (`since` below)
 *                    SAIP_GUARD_FORCE       goal rows 30..32 (sensed force, sensor frame) as the control law reads them: axis 0..2 a
 *                                           component, axis 3 sqrt((f0 f0 + f1 f1) + f2 f2), every product and sum rounded on its own
 *                    SAIP_GUARD_MOMENT      the same on rows 33..35
 *                    SAIP_GUARD_POSITION    world position of the task's control point, axis 0..2
 *                    SAIP_GUARD_POS_ERROR   norm of the selection-projected position error against the task's goal rows as they stand
 *                    SAIP_GUARD_ORI_ERROR   ... of the orientation error (both: the bits of rows 0..5 of the task diagnostics, squared,
 *                                           summed and rooted as the recorder's summaries are).  "As they stand" is before
 *                                           this evaluation writes: in a HOLD or OFFSET phase rows 0..11 are what the previous
 *                                           evaluation wrote, unless something in front of the guard wrote them since -- a goal
 *                                           schedule on the position rows does so in every period, and the error is then against
 *                                           the schedule's goal of the period, not against the held pose the task tracks.  A guard
 *                                           meant as "settled at the held pose" belongs on a task without such a schedule.
 *                    SAIP_GUARD_JOINT_SPEED max_j |dq_j|
 *            cmp     SAIP_GUARD_GE (signal >= threshold) or SAIP_GUARD_LE; a NaN signal satisfies neither.
 *            hold    >= 1, a debounce: the condition must be true in `hold` consecutive evaluations.
 *            blank   >= 0, a blanking time: the guard is evaluated only once since >= blank (a contact transient is not an event).
 *   phases   n_phases (1..SAIP_GUARD_MAX_PHASES) rows of SAIP_GUARD_PHASE_WORDS doubles { mode, dx, dy, dz }, batch-uniform.
 *            SAIP_GUARD_FREE    the evaluation writes no goal row: whatever a schedule or the host wrote stands.  Phase 0 must be FREE.
 *            SAIP_GUARD_HOLD    in every period goal rows 0..11 take the pose latched at the transition into the phase, rows 12..23 take 0.
 *            SAIP_GUARD_OFFSET  HOLD with the latched position plus (dx, dy, dz) in the world frame, each sum rounded once.
 *   one evaluation of one instance (csrc/saip_guard.h; tests/guard_ref.py restates it in NumPy bit for bit):
 *            p = phase; fired = -1
 *            for g = 0 .. G-1:  if from[g] != p or since < blank[g]: run[g] = 0
 *                               else: run[g] = cond(g) ? run[g] + 1 : 0;  if fired < 0 and run[g] >= hold[g]: fired = g
 *            if fired >= 0:     fires[fired] += 1; phase = to[fired]; since = 0; every run[g] = 0
 *                               if entry[phase] < 0: entry[phase] = clock;  latch[0..11] = the pose this evaluation computed
 *            else:              since += 1
 *            the mode of the (new) phase is applied to the goal rows; clock += 1
 *            At most one transition per period.  _attach and _reset leave phase = since = clock = run = fires = 0, entry[0] = 0,
 *            entry[p > 0] = -1, latch = 0.  There is no host-side counter: clock is a per-instance device word.
 *   reads    what the controller reads: the measured q, dq while a sensing model is attached (behind its chain), else the resident state;
 *            goal rows 30..35 as the simulated sensor and the sensing model left them.  The pose is computed only when a guard
 *            (POSITION, *_ERROR) or a phase (HOLD, OFFSET) needs it; a launch that computes none leaves the latch as it is.
 *   where    in a period of saip_batch_rollout_async: behind the goal schedules, the environment schedules, the simulated-sensor launches
 *            and the sensing launch, in front of the period's OTG step and cycle -- an internal OTG sees a guard's goal change as it sees
 *            a host setGoal and replans, which makes HOLD a smooth stop.  One extra launch per period; while attached the integration is
 *            not fused with the next period's OTG step (as with goal schedules).  saip_batch_guard_evaluate enqueues the same launch on
 *            its own: { saip_batch_contact_sense, saip_batch_guard_evaluate, saip_batch_step_async, saip_batch_integrate } leaves the bits
 *            of a rollout period.  Without the attachment every entry point enqueues exactly what it did before.
 *   readout  [SAIP_GUARD_READOUT_ROWS][ld] of the last launch: force norm, moment norm, position error norm, orientation error norm,
 *            joint speed, position 3.  A row the launch did not need holds NaN.
 *   state    phase, since, clock [B]; run, fires [G][B]; entry [P][B] (the clock at the first entry into a phase, -1: never); latch [12][B]
 *            (position 3, rotation 9 row-major).  While attached a state snapshot carries it as segments guard.phase, guard.since,
 *            guard.clock, guard.run, guard.entry, guard.fires, guard.latch; a snapshot of another guard layout is refused (SAIP_ERR_ORDER,
 *            the segment named).
 *   saip_batch_guard_set_guards_host replaces the table and keeps the state.  A writer through saip_batch_guard_guards_device keeps to
 *   the signals of the table last uploaded from the host: the launch gathers only what that table needs.
 *   saip_batch_guard_add_cost: cost[i] = cost[i] + (entry[phase][i] >= 0 ? w_time (double)entry[phase][i] : w_miss) on the sampler's
 *   per-instance cost; w_miss = +inf makes "never got there" an invalid sample.
 * Only columns 0 .. B-1 of any array are written.
 * SAIP_ERR_ORDER: before finalize, on a model-only batch, a second attach, any other entry without the attachment, _add_cost without a
 * sampler.  SAIP_ERR_INVALID_ARGUMENT (the message names the guard or phase, the word and, for a per-instance table, the instance): a task
 * that is not a motion-force task, n_guards or n_phases outside 1..8, from / to outside the phases, an unknown signal, axis, cmp or mode,
 * a threshold or offset that is not finite, hold < 1, blank < 0, an integer word that is not an integer, phase 0 not FREE, null tables,
 * a phase outside the table or a NaN weight in _add_cost.  Argument and order errors are reported before the device is needed and write
 * nothing. */
#define SAIP_GUARD_MAX_PHASES 8
#define SAIP_GUARD_MAX_GUARDS 8
#define SAIP_GUARD_WORDS 8
#define SAIP_GUARD_PHASE_WORDS 4
#define SAIP_GUARD_READOUT_ROWS 8
#define SAIP_GUARD_PERIODS 0
#define SAIP_GUARD_FORCE 1
#define SAIP_GUARD_MOMENT 2
#define SAIP_GUARD_POSITION 3
#define SAIP_GUARD_POS_ERROR 4
#define SAIP_GUARD_ORI_ERROR 5
#define SAIP_GUARD_JOINT_SPEED 6
#define SAIP_GUARD_GE 0
#define SAIP_GUARD_LE 1
#define SAIP_GUARD_FREE 0
#define SAIP_GUARD_HOLD 1
#define SAIP_GUARD_OFFSET 2
saip_status saip_batch_guard_attach(saip_batch*, int task, int n_guards, const double* guards, int per_instance, int n_phases, const double* phases);
saip_status saip_batch_guard_detach(saip_batch*);
saip_status saip_batch_guard_info(saip_batch*, int* task, int* n_guards, int* per_instance, int* n_phases, int* needs_pose);  /* any NULL */
saip_status saip_batch_guard_set_guards_host(saip_batch*, const double* guards);
double* saip_batch_guard_guards_device(saip_batch*);  /* [G][8] or [G][8][ld]; NULL when detached */
saip_status saip_batch_guard_reset(saip_batch*);      /* on the stream */
saip_status saip_batch_guard_evaluate(saip_batch*);
saip_status saip_batch_guard_state_host(saip_batch*, int* phase, int* since, int* clock, int* run, int* entry, int* fires, double* latch);  /* any NULL; synchronous */
saip_status saip_batch_guard_state_device(saip_batch*, int** phase, int** since, int** clock, int** run, int** entry, int** fires, double** latch);  /* the arrays, [rows][ld] */
saip_status saip_batch_guard_readout_host(saip_batch*, double* out /* [8][B] */);  /* synchronous */
double* saip_batch_guard_readout_device(saip_batch*);  /* [8][ld]; NULL when detached */
saip_status saip_batch_guard_add_cost(saip_batch*, int phase, double w_time, double w_miss);
/* ---- rollout recorder: a per-period trajectory log and running summaries of saip_batch_rollout_async, kept on the device (the
 * reference's example loops print or log the same quantities every period: state, torques, position / orientation error).  A recorder
 * is attached to a finalized batch and stays attached across rollout calls until detached.  It observes rollout periods only
 * (saip_batch_step_async, saip_batch_integrate and saip_batch_compute_control_torques called directly are not recorded), each one AFTER
 * its integration: the torques that were applied during the period (the array saip_batch_integrate reads), the status byte of the
 * period's cycle, q and dq as the integration left them, and the task quantities of one motion-force task at that state against its
 * user goal as it stands.  A period counter p starts at 1 with the first recorded period and continues across rollout calls.
 *   log: every stride-th period (p % stride == 0) goes to slot (p / stride - 1) % capacity of a ring that keeps the last `capacity`
 *        samples: log[slot][row][ld] doubles and status[slot][ld] bytes (ld = saip_batch_ld; columns B..ld-1 are never written).  The
 *        rows of a sample are the channels selected by `channels`, in this order:
 *          SAIP_RECORD_Q     q    [dof]
 *          SAIP_RECORD_DQ    dq   [dof]
 *          SAIP_RECORD_TAU   tau  [dof], NaN kept as NaN
 *          SAIP_RECORD_POSE  position [3], rotation [9] row-major of the task's control frame (as saip_batch_get_current_pose_host)
 *          SAIP_RECORD_ERROR rows 0..5 of saip_batch_get_task_diagnostics_host: selection-projected position and orientation error
 *        With an empty mask nothing is sampled.
 *   summaries (summaries != 0), advanced on EVERY period whatever the stride; [8][ld], T = sim_dt * substeps of the rollout call:
 *          0 sum T tau.tau (NaN entries count as 0, the way the integrator coasts)    1 sum T |e_pos|^2    2 sum T |e_ori|^2
 *          3 max |e_pos|    4 max |e_ori|    5 max_j |tau_j|    6 max_j |dq_j|    7 number of periods with status != 0
 *        e_pos, e_ori are the error rows above; rows 1..4 stay 0 without a task.  The maxima skip NaN entries.
 *   task: one motion-force task, or -1 (then the pose and error channels are SAIP_ERR_INVALID_ARGUMENT).
 * The log is allocated and zeroed by _attach, never inside a rollout; _detach waits for the stream and frees it; _reset (on the stream)
 * sets p back to 0, empties the log and zeroes the summaries.  Without a recorder a rollout enqueues exactly what it did before; with
 * one, one small launch per observed period (per sampled period when summaries are off).  SAIP_ERR_ORDER: before saip_batch_finalize,
 * on a model-only batch, a second _attach without _detach, and every other entry without a recorder. */
enum { SAIP_RECORD_Q = 1, SAIP_RECORD_DQ = 2, SAIP_RECORD_TAU = 4, SAIP_RECORD_POSE = 8, SAIP_RECORD_ERROR = 16 };
#define SAIP_RECORD_SUMMARY_ROWS 8
saip_status saip_batch_rollout_recorder_attach(saip_batch*, int capacity, int stride, unsigned channels, int task, int summaries);
saip_status saip_batch_rollout_recorder_detach(saip_batch*);
saip_status saip_batch_rollout_recorder_reset(saip_batch*);
/* samples in the log, rows per sample, period number of the oldest sample (0 when empty), stride; any pointer may be NULL */
saip_status saip_batch_rollout_log_info(saip_batch*, int* n_samples, int* rows, int* first_period, int* stride);
/* the log in chronological order: out [n_samples][rows][B], status [n_samples][B] (either may be NULL); synchronous */
saip_status saip_batch_rollout_log_host(saip_batch*, double* out, uint8_t* status);
/* the summaries: out [8][B]; synchronous.  SAIP_ERR_ORDER when the recorder was attached without summaries */
saip_status saip_batch_rollout_summary_host(saip_batch*, double* out);
double* saip_batch_rollout_log_device(saip_batch*);      /* [capacity][rows][ld], ring order; NULL when detached or nothing is sampled */
double* saip_batch_rollout_summary_device(saip_batch*);  /* [8][ld]; NULL when detached or without summaries */
/* overwrite the resident torque array ([dof][B]) that saip_batch_integrate applies -- sim->setJointTorques(name, control_torques +
 * ui_torques) in the examples (05-...cpp:226-228) when the applied torque is not just the last cycle's output */
saip_status saip_batch_set_torques_host(saip_batch*, const double* tau);
/* read the resident state back: q, dq [dof][B] (either may be NULL) */
saip_status saip_batch_get_state_host(saip_batch*, double* q, double* dq);
/* ---- robot-model queries: batched SaiModel accessors at the resident state (q, dq as they stand on the device, whoever wrote them:
 * saip_batch_set_state_host / _device, saip_batch_integrate, saip_batch_rollout_async).  They write their outputs and nothing else: no
 * task, torque, status, integrator, OTG or singularity-handler state changes.  sai-model is not part of the reference tree; its
 * semantics below are [RECALLED] unless a reference line is cited.  Call sites: examples/05-using_robot_controller/
 * 05-using_robot_controller.cpp:69,120-122 (setTRobotBase, positionInWorld, rotationInWorld), examples/03-...cpp:133-134 (position,
 * rotation), examples/15-...cpp:225-230 (linearVelocityInWorld, angularVelocityInWorld, transformInWorld).
 * Errors: SAIP_ERR_ORDER before finalize, SAIP_ERR_NO_DEVICE on a configuration-only batch, SAIP_ERR_INVALID_ARGUMENT for a link index
 * out of range, n_frames outside 1..SAIP_MAX_QUERY_FRAMES, unknown flag bits, a NULL out or links, or dynamics with every output NULL. */
#define SAIP_MAX_QUERY_FRAMES 8
enum { SAIP_QUERY_JACOBIAN = 1, SAIP_QUERY_WORLD = 2 };
/* SaiModel::setTRobotBase / TRobotBase [RECALLED]: T_world_robot of every instance of the batch, R row-major + translation p; identity
 * by default.  Used ONLY by queries with SAIP_QUERY_WORLD: gravity, g(q), the torques and the integrator stay in the robot base frame
 * with the model's gravity.  Whether sai-model also rotates gravity by the base cannot be seen in the reference tree; the engine does
 * not. */
saip_status saip_batch_set_robot_base(saip_batch*, const double R[9], const double p[3]);
saip_status saip_batch_get_robot_base(const saip_batch*, double R[9], double p[3]);
/* rows written per frame by saip_batch_model_frames_*: 18, or 18 + 6 * dof with SAIP_QUERY_JACOBIAN (0 for a NULL batch or bad flags) */
int saip_batch_model_frame_rows(const saip_batch*, int flags);
/* Kinematics of n_frames frames (link, point fixed in the link) at the resident state, in the robot base frame:
 *   rows  0..2   SaiModel::position(link, pos_in_link)           3..11  rotation(link), row-major
 *   rows 12..14  linearVelocity(link, pos_in_link)               15..17 angularVelocity(link)
 *   rows 18..    J(link, pos_in_link) = [Jv; Jw], 6 x dof row-major (SAIP_QUERY_JACOBIAN; the [Jv; Jw] order of MotionForceTask.cpp:293-298)
 * SAIP_QUERY_WORLD maps every row through T_world_robot: the *InWorld accessors (positionInWorld, rotationInWorld, linearVelocityInWorld,
 * angularVelocityInWorld, JWorldFrame [RECALLED]): positions -> R_wb x + p_wb, rotations -> R_wb R, every other 3-vector -> R_wb v.
 * links: saip_model_link_index values; links welded to a movable body compose their fixed transform as tasks on them do; a link welded
 * to the fixed base has a constant pose, zero twist and an all-zero Jacobian.  pos_in_link: [n_frames][3], NULL = all zero.  A frame
 * equal to a task's control frame (identity compliant rotation) gives rows 0..11 bit-identical to saip_batch_get_current_pose_host.
 * _host: out = [n_frames][rows][B], synchronous.  _device: out_dev = [n_frames][rows][ld] device memory, asynchronous on the batch stream. */
saip_status saip_batch_model_frames_host(saip_batch*, int n_frames, const int* links, const double* pos_in_link, int flags, double* out);
saip_status saip_batch_model_frames_device(saip_batch*, int n_frames, const int* links, const double* pos_in_link, int flags, double* out_dev);
/* Joint-space dynamics at the resident state; any output may be NULL (that quantity is skipped, not computed):
 *   M     = SaiModel::M()                [dof*dof] row-major per instance (composite rigid bodies)
 *   M_inv = SaiModel::MInv()             [dof*dof] (from the Cholesky factor of M)
 *   g     = SaiModel::jointGravityVector(): what gravity compensation adds to the torques (RobotController.cpp:114-115), model gravity
 *           in the robot base frame   [dof]
 *   b     = SaiModel::coriolisForce(): C(q, dq) dq, so that M qdd + b + g = tau (the convention of saip_batch_integrate)   [dof]
 * _host: [..][B], synchronous.  _device: [..][ld] device pointers, asynchronous on the batch stream. */
saip_status saip_batch_model_dynamics_host(saip_batch*, double* M, double* M_inv, double* g, double* b);
saip_status saip_batch_model_dynamics_device(saip_batch*, double* M_dev, double* M_inv_dev, double* g_dev, double* b_dev);
/* finalize a batch with NO tasks that only mirrors a robot's state for the model queries (SaiModel::updateModel).  Allowed afterwards:
 * the state setters and getters, saip_batch_synchronize / _wait_for, the robot base, the model queries, saip_batch_ld / _size / _dof /
 * _stream and saip_batch_device_q / _dq.  Every entry that needs a task or a controller returns SAIP_ERR_ORDER: cycle, step, per-task,
 * rollout, integrate, timing, gather.  saip_batch_finalize itself still refuses a batch with no tasks. */
saip_status saip_batch_finalize_model_only(saip_batch*);
/* getDesiredPosition/Velocity/Acceleration (JointTask.h:185-200; MotionForceTask desired* likewise): [goal_components][B] in the
 * goal layout -- the internal OTG's output of the last cycle when it is enabled, otherwise the goal itself. */
saip_status saip_batch_get_desired_host(saip_batch*, int task, double* desired);
/* per-instance OTG state of a task after the last cycle: flags (bit 0 goal reached = OTG_joints::isGoalReached, bit 3 an
 * error occurred since the last re-initialisation, bit 4 a trajectory finished with non-zero velocity) and the ruckig::Result of
 * the last cycle (0 Working, 1 Finished, < 0 error codes of ruckig/result.hpp).  Motion-force tasks additionally: bit 6 = the
 * goal orientation of the last cycle was not a rotation matrix (the reference throws, OTG_6dof_cartesian.cpp:158-162; the goal
 * is ignored).  Either pointer may be NULL. */
saip_status saip_batch_get_otg_status_host(saip_batch*, int task, int* flags, int* result);
/* velocity saturation: MotionForceTask::enableVelocitySaturation(linear, angular) / disableVelocitySaturation
 * (MotionForceTask.cpp:771-792, law :416-430, :449-462); JointTask::enableVelocitySaturation(value | vector) (JointTask.cpp:410-436,
 * law :327-341).  n_values: motion-force task 2 = {linear, angular}; joint task 1 or task dof; 0 keeps the stored/default limits
 * (MotionForceTask.h:63-64: 0.3, pi/3; JointTask.h:44: pi/3). */
saip_status saip_batch_set_velocity_saturation(saip_batch*, int task, int enabled);
saip_status saip_batch_set_saturation_velocities(saip_batch*, int task, const double* values, int n_values);
/* MotionForceTask::parametrizeForceMotionSpaces / parametrizeMomentRotMotionSpaces (MotionForceTask.cpp:828-890): dimension 0..3,
 * axis used for dimensions 1 and 2.  *changed (optional) = the reference's return value; when the parametrisation changed and the
 * device holds a state, the linear (angular) goal is reset to the current pose and the integrators to zero like the reference does. */
saip_status saip_batch_parametrize_force_motion_spaces(saip_batch*, int task, int force_space_dimension, const double axis[3], int* changed);
saip_status saip_batch_parametrize_moment_rot_motion_spaces(saip_batch*, int task, int moment_space_dimension, const double axis[3], int* changed);
/* constructor argument is_force_motion_parametrization_in_compliant_frame (MotionForceTask.h:96-110): axes and goal force/moment
 * are expressed in the compliant frame instead of the world frame */
saip_status saip_batch_set_parametrization_in_compliant_frame(saip_batch*, int task, int enabled);
/* MotionForceTask::setForceControlGains / setMomentControlGains: open-loop force control uses kv only (MotionForceTask.cpp:350-354, :379-383) */
saip_status saip_batch_set_force_control_gains(saip_batch*, int task, double kp, double kv, double ki);
saip_status saip_batch_set_moment_control_gains(saip_batch*, int task, double kp, double kv, double ki);
/* setClosedLoopForceControl / setClosedLoopMomentControl (MotionForceTask.cpp:973-986; law :327-349, :357-378, :484-487): PI feedback
 * on the sensed force / moment inside the force / moment space, saturated at the maximum feedback output, goal force feed-forward
 * scaled by kff.  The sensed force and moment of the current cycle are rows 30..32 / 33..35 of the task's goal block, in the SENSOR
 * frame (updateSensedForceAndMoment, :805-828: the engine applies _T_control_to_sensor and the control frame's world rotation of the
 * current state).  A change of either flag resets the linear / angular integrators like the reference.
 * saip_batch_set_passivity = enablePassivity / disablePassivity (.h:630-631): the windowed passivity observer + passivity controller
 * of POPCExplicitForceControl.cpp:29-96 around the force loop (off by default like in the reference; disabling re-initialises it).
 * The reference's energy window is an unbounded std::queue; the device keeps 1024 samples per instance and sets status bit 2 (value
 * 4) on an instance whose window would have grown beyond that (more than ~0.77 s of uninterrupted activity at 1 kHz). */
saip_status saip_batch_set_closed_loop_force_control(saip_batch*, int task, int enabled);
saip_status saip_batch_set_closed_loop_moment_control(saip_batch*, int task, int enabled);
saip_status saip_batch_set_passivity(saip_batch*, int task, int enabled);
/* setFeedforwardForceGain / setFeedforwardMomentGain / setMaxForceControlFeedbackOutput / setMaxMomentControlFeedbackOutput
 * (MotionForceTask.h:330-355); defaults 0.95, 0.95, 20 N, 10 Nm (.h:56-59) */
saip_status saip_batch_set_force_control_parameters(saip_batch*, int task, double kff_force, double kff_moment, double max_force_feedback, double max_moment_feedback);
/* setForceSensorFrame (MotionForceTask.cpp:794-803) given as _T_control_to_sensor = compliant_frame^-1 * T_link_sensor:
 * rotation 3x3 row-major and translation; default identity (:94) */
saip_status saip_batch_set_control_to_sensor_transform(saip_batch*, int task, const double* R_row_major, const double* translation);
/* RobotController::enable{GravityCompensation,JointLimitAvoidance,TorqueSaturation}, RobotController.h:64-75 */
saip_status saip_batch_enable_gravity_compensation(saip_batch*, int enabled);
saip_status saip_batch_enable_joint_limit_avoidance(saip_batch*, int enabled); /* JLA wrap, RobotController.cpp:96-112 */
saip_status saip_batch_enable_torque_saturation(saip_batch*, int enabled);
/* torques of an instance that ends a cycle flagged (status 1): 0 (default) = not written, i.e. the last valid torques of that instance are
 * held (zero before the first valid cycle); 1 = NaN.  The reference has no such state: it never refuses an instance. */
saip_status saip_batch_set_flagged_torque_policy(saip_batch*, int nan);
/* where the eight-lane kernels recompute the instances they cannot finish themselves (a task outside SingularityHandler's non-singular branch,
 * SingularityHandler.cpp:100-121, 146-158, 310-367): 0 (default) = in the kernel, by the wavefront that met them, right behind its epilogue -- no
 * second launch; costs nothing when there are none and ~70 us per instance and wavefront when there are, one after the other; 1 = on a device-side
 * list that a second launch behind every cycle spreads over the chip (+4.5 us per cycle, always) -- faster when MANY instances of one group of
 * eight are singular at once (measured, config 3's stack, 4096 instances: 1/8 of the batch packed into whole groups: 96 against 271 us per cycle;
 * spread evenly: 89 against 86).  Same results either way. */
saip_status saip_batch_set_flagged_recompute(saip_batch*, int on_list);
/* integrator state policy: 0 = advance the integral terms only while the task's ki != 0 (default; elides the
 * state traffic), 1 = advance every cycle like the reference does (MotionForceTask.cpp:411-413,446; JointTask.cpp:323) */
saip_status saip_batch_set_integrator_tracking(saip_batch*, int always);

/* ---- per-instance inputs (host staging: H2D copies on the engine stream) */
saip_status saip_batch_set_state_host(saip_batch*, const double* q /*[dof][B]*/, const double* dq /*[dof][B]*/); /* setQ/setDq */
/* whole goal block of a task, [goal_components][B]: setGoalPosition/Orientation/LinearVelocity/AngularVelocity/
 * LinearAcceleration/AngularAcceleration (MotionForceTask.h:211-247) or setGoalPosition/Velocity/Acceleration (JointTask.h:140-175) */
saip_status saip_batch_set_goal_host(saip_batch*, int task, const double* goal);
/* one goal field: component offset/count inside the goal block (e.g. position: 0,3; orientation: 3,9) */
saip_status saip_batch_set_goal_field_host(saip_batch*, int task, int first_component, int n_components, const double* values);
saip_status saip_batch_get_goal_host(saip_batch*, int task, double* goal);
/* TemplateTask::reInitializeTask / RobotController::reinitializeTasks: goal := current pose of every instance,
 * velocities/accelerations := 0, integrators := 0 (MotionForceTask.cpp:204-245, JointTask.cpp:91-107). GPU kernel. */
saip_status saip_batch_reinitialize_tasks(saip_batch*);
/* MotionForceTask::getCurrentPosition / getCurrentOrientation (MotionForceTask.h:121-138) at the state last set: pos [3][B], rot [9][B]
 * (row-major per instance); either pointer may be NULL */
saip_status saip_batch_get_current_pose_host(saip_batch*, int task, double* pos, double* rot);
/* Task-space diagnostics of one motion-force task at the state last set (q, dq) -- 24 rows per instance:
 *    0..2   getPositionError()     sigmaPosition (x_goal - x)                        (MotionForceTask.cpp:540-542)
 *    3..5   getOrientationError()  sigmaOrientation orientationError(R_goal, R)      (:544-546, :291)
 *    6..8   getCurrentLinearVelocity()   rows 0-2 of (P J_world) dq, P = partial-task projection (:293-298)
 *    9..11  getCurrentAngularVelocity()  rows 3-5 of (P J_world) dq
 *   12..14  getSensedForceControlWorldFrame()   from goal entries 30..32 (sensor frame; zero unless closed-loop force or moment
 *   15..17  getSensedMomentControlWorldFrame()  control gives the goal block those entries) through the control-to-sensor transform (:805-828)
 *   18..23  getUnitMassForce()     the control law's position / orientation term (MotionForceTask.h:266, .cpp:478), here DEFINED as the law
 *           evaluated at the state last set, with the desired state of the last cycle (the OTG output, or the goal when the OTG is off) and
 *           the integrators as they stand, advanced by one step on a copy.  With zero integral gains and no closed-loop force / moment
 *           control this is what the last cycle used at that state.
 * Nothing of the task's state is written (integrators, OTG, passivity observer, goal, status).  Motion-force tasks only.
 * _host: out [24][B], synchronous.  _device: out_dev [24][ld] (device memory), asynchronous on the batch stream. */
saip_status saip_batch_get_task_diagnostics_host(saip_batch*, int task, double* out);
saip_status saip_batch_task_diagnostics_device(saip_batch*, int task, double* out_dev);
/* TemplateTask::reInitializeTask of ONE task (MotionForceTask.cpp:204-245, JointTask.cpp:95-106) */
saip_status saip_batch_reinitialize_task(saip_batch*, int task);
/* MotionForceTask::resetIntegrators / resetIntegratorsLinear / resetIntegratorsAngular (MotionForceTask.cpp:988-1002; the linear part
 * also clears the force integrator, the angular part the moment integrator), JointTask::resetIntegrators.  parts: 1 linear (or the
 * joint task's), 2 angular, 3 both. */
saip_status saip_batch_reset_integrators(saip_batch*, int task, int parts);

/* ---- zero-copy access for resident pipelines (simulator / rollout on the same GPU) */
double* saip_batch_device_q(saip_batch*);
double* saip_batch_device_dq(saip_batch*);
double* saip_batch_device_goal(saip_batch*, int task);
double* saip_batch_device_tau(saip_batch*);          /* [dof][ld] */
uint8_t* saip_batch_device_status(saip_batch*);      /* [ld] */
/* write torques to a caller-owned device buffer (e.g. a torch tensor used for the RCCL gather); NULL restores the internal one */
saip_status saip_batch_bind_tau_device(saip_batch*, double* tau_dev /*[dof][ld]*/);
void* saip_batch_stream(saip_batch*);                /* hipStream_t */

/* ---- the control cycle */
/* robot->updateModel() + RobotController::updateControllerTaskModels() (RobotController.cpp:68-77) */
saip_status saip_batch_update_task_models(saip_batch*);
/* RobotController::computeControlTorques() (RobotController.cpp:79-118); requires update_task_models since the last
 * state change.  tau_host may be NULL (results stay on the device); status_host may be NULL. */
saip_status saip_batch_compute_control_torques(saip_batch*, double* tau_host /*[dof][B]*/, uint8_t* status_host /*[B]*/);
/* both of the above as ONE asynchronous launch on the engine stream; no host synchronisation */
saip_status saip_batch_step_async(saip_batch*);
saip_status saip_batch_synchronize(saip_batch*);
saip_status saip_batch_get_torques_host(saip_batch*, double* tau_host, uint8_t* status_host);
/* per-task diagnostics of the hierarchy, for parity tests of the task models: TemplateTask::getTaskNullspace()
 * ([dof*dof][B] row-major per instance).  Re-evaluates the task models with the general kernel (no control law; torques, status,
 * integrators, OTG and handler state of the last cycle stay untouched). */
saip_status saip_batch_get_task_nullspace_host(saip_batch*, int task, double* N /*[dof*dof][B]*/);

/* ---- the reference's per-task plug-in interface, TemplateTask.h:43-60 (pure virtuals of every task):
 *        virtual void updateTaskModel(const Eigen::MatrixXd& N_prec);
 *        virtual Eigen::VectorXd computeTorques();
 *        virtual Eigen::VectorXd computeTorques(const Eigen::VectorXd& tau_prec);
 *        getTaskNullspace() / getPreviousTasksNullspace() / getTaskAndPreviousNullspace()   (:71-89)
 * A caller that builds its own hierarchy drives the tasks by hand (examples/04-task_and_redundancy/04-task_and_redundancy.cpp:141-206):
 *        N_prec = I;  mf->updateTaskModel(N_prec);  N_prec = mf->getTaskAndPreviousNullspace();  jt->updateTaskModel(N_prec);
 *        tau = mf->computeTorques() + jt->computeTorques();
 * Nullspace matrices are [dof*dof][B] (host) / [dof*dof][ld] (device), row-major per instance.  The task keeps its own copy of N_prec
 * (MotionForceTask.cpp:259-267 / JointTask.cpp:230).  One launch of the general kernel per call, restricted to the task:
 * update_model evaluates the model for the current state (nullspaces out; SingularityHandler's classification state advances here like in
 * SingularityHandler::updateTaskModel, .cpp:227), compute_torques evaluates the control law (integrators, internal OTG, the type-2
 * direction memory advance here like in the reference's computeTorques) and returns THIS task's torques, without any of
 * RobotController's post-processing.  tau_prec = NULL is computeTorques(); otherwise the joint task subtracts its disturbance
 * compensation (JointTask.cpp:285-292) and the motion-force task adds nothing (its _Lambda is never written, MotionForceTask.cpp:140,273).
 * compute_torques after a state change without a new update_model is SAIP_ERR_ORDER (the reference would mix a fresh Jacobian with
 * stale Lambda / N_prec, MotionForceTask.cpp:280-283).  status: per-instance codes as for the whole cycle; where it is 1 the task's
 * torques follow saip_batch_set_flagged_torque_policy like the controller's (default: left as they were -- zero before the first valid
 * call --, 1: NaN): check the status, not isnan. */
saip_status saip_batch_task_update_model(saip_batch*, int task, const double* N_prec_host /* NULL = identity */);
saip_status saip_batch_task_update_model_device(saip_batch*, int task, const double* N_prec_dev /* NULL = identity; asynchronous */);
saip_status saip_batch_task_compute_torques(saip_batch*, int task, const double* tau_prec_host /*[dof][B] or NULL*/, double* tau_host /*[dof][B]*/, uint8_t* status_host /*[B] or NULL*/);
/* asynchronous flavour on the engine stream: tau_prec_dev [dof][ld] or NULL, tau_dev [dof][ld] or NULL (= the task's own buffer, saip_batch_task_device_torques) */
saip_status saip_batch_task_compute_torques_device(saip_batch*, int task, const double* tau_prec_dev, double* tau_dev);
/* getTaskNullspace (N), getPreviousTasksNullspace (N_prec), getTaskAndPreviousNullspace (N N_prec) of the last update_model; any pointer may be NULL */
saip_status saip_batch_task_get_nullspaces_host(saip_batch*, int task, double* N, double* N_prec, double* N_total);
/* the same on the device: which = 0 N, 1 N_prec (NULL when the identity was used), 2 N N_prec; NULL before the first update_model */
const double* saip_batch_task_device_nullspace(saip_batch*, int task, int which);
double* saip_batch_task_device_torques(saip_batch*, int task);
/* robot->setQ/setDq from arrays already on the device ([dof][ld], e.g. the state of another batch of the same robots): asynchronous D2D copy */
saip_status saip_batch_set_state_device(saip_batch*, const double* q_dev, const double* dq_dev);
/* device-side ordering between two batches' streams (no host synchronisation): everything enqueued so far on `producer` happens before
 * what is enqueued on `waiter` from now on.  Needed when one batch consumes device arrays another batch has just written (tasks driven
 * by hand that live in batches of their own). */
saip_status saip_batch_wait_for(saip_batch* waiter, saip_batch* producer);

/* kernel selection: 0 = auto, 1 = general workgroup-per-instance kernel, 2 = lane-per-instance register kernel (dof <= 8),
 * 3 = eight-lanes-per-instance kernel (7-dof chain, full MotionForceTask + full JointTask; the auto choice for batches <= 24576 of that stack, and at every batch size for its partial-task /
 *     reduced-task / joint-first / 6- and 8-dof instantiations),
 * 4 = wavefront-per-instance kernel on the FP64 matrix cores (chains of 9..32 dof; the auto choice there) */
saip_status saip_batch_set_kernel(saip_batch*, int which);
const char* saip_batch_kernel_name(saip_batch*);
/* HIP-event timing of `steps` back-to-back cycles on the engine stream (after `warmup` untimed ones):
 * total elapsed ms over the timed region.  Used by bench.py for the live roofline figure. */
saip_status saip_batch_time_steps(saip_batch*, int steps, int warmup, double* elapsed_ms);
/* the same without a wait inside: _begin records the first event, enqueues `steps` cycles, records the second event and returns; the caller waits
 * for the device in whatever way it waits anyway (bench.py: the torch.cuda.synchronize() its timing contract prescribes) and then asks _end for the
 * event time.  One wait instead of two: every runtime wait is its own marker round trip (4 - 15 us), which a 20-step timed region notices. */
saip_status saip_batch_time_steps_begin(saip_batch*, int steps);
saip_status saip_batch_time_steps_end(saip_batch*, double* elapsed_ms);

/* ---- multi-GPU (the reference is single-robot / single-thread, /root/reference/src/RobotController.cpp:68-118 has nothing to
 * shard): instances shard embarrassingly across the GPUs of a node, one batch per device, NO data-path collective; the only exchange is the
 * final gather of the [dof][ld] torque slabs, one ncclAllGather over xGMI.  C++ on RCCL, loaded on first use -- no PyTorch.
 * (a) one process per GPU: rank 0 draws a unique id, the 128 bytes reach the other ranks by the launcher's rendezvous, every rank creates its
 *     communicator; saip_batch_all_gather_torques enqueues the all-gather on the batch's stream: gathered_dev = [world][dof][ld]. */
#define SAIP_COMM_ID_BYTES 128
typedef struct saip_comm saip_comm;
/* can this process join a communicator on `device` (librccl loads, the device can be selected)?  Ask on EVERY rank and reduce the answers
 * before any rank calls saip_comm_create: a rank that fails locally would leave the others blocked inside ncclCommInitRank. */
saip_status saip_comm_probe(int device);
saip_status saip_comm_unique_id(void* id128);
saip_status saip_comm_create(int device, int world, int rank, const void* id128, saip_comm** out);
void saip_comm_destroy(saip_comm* comm);
int saip_comm_world(const saip_comm* comm); /* the number of ranks RCCL counts in the communicator (ncclCommCount) */
int saip_comm_rank(const saip_comm* comm);
/* every rank's batch must have the same dof and leading dimension (saip_batch_set_leading_dimension for uneven shards) */
saip_status saip_batch_all_gather_torques(saip_batch* batch, saip_comm* comm, double* gathered_dev);
/* HIP-event timing of `steps` cycles WITH the torque gather in the timed region: gather_mode 0 = one all-gather behind the last cycle (north_star:
 * "RCCL ... only for the final torque gather"), 1 = one behind EVERY cycle (what a consumer that takes the torques each control period sees,
 * /root/reference/examples/05-using_robot_controller/05-using_robot_controller.cpp:193-196, 225-231).  elapsed_ms = events around the whole region,
 * gather_ms = the sum over the gathers of the event time of each (so gather_ms / number of gathers is the cost of one).  comm == NULL (one
 * rank): no collective is issued and gather_ms = 0. */
saip_status saip_batch_time_steps_gather(saip_batch* batch, saip_comm* comm, double* gathered_dev, int steps, int gather_mode, double* elapsed_ms, double* gather_ms);
/* (b) one process, n devices: one batch + stream + communicator per device.  saip_multi_create makes the (unfinalized) batches -- add the same
 *     tasks to every saip_multi_batch(m, i) -- saip_multi_finalize finalizes them, runs ncclCommInitAll and allocates the gather buffers;
 *     saip_multi_step_async = saip_batch_step_async on every device, saip_multi_all_gather_torques = one grouped ncclAllGather, after which
 *     every device holds [n_devices][dof][ld] at saip_multi_gathered_device(m, i). */
typedef struct saip_multi saip_multi;
saip_status saip_multi_create(const saip_model* model, int batch_per_device, const int* devices, int n_devices, saip_multi** out);
int saip_multi_size(const saip_multi* m);
saip_batch* saip_multi_batch(saip_multi* m, int i);
saip_status saip_multi_finalize(saip_multi* m);
saip_status saip_multi_step_async(saip_multi* m);
saip_status saip_multi_all_gather_torques(saip_multi* m);
saip_status saip_multi_synchronize(saip_multi* m);
/* the same timing for the one-process form: every device runs `steps` cycles (+ the grouped all-gather, gather_mode as above); elapsed_ms / gather_ms =
 * the maximum over the devices of each device's event times */
saip_status saip_multi_time_steps(saip_multi* m, int steps, int gather_mode, double* elapsed_ms, double* gather_ms);
double* saip_multi_gathered_device(saip_multi* m, int i);
saip_status saip_multi_get_gathered_host(saip_multi* m, int i, double* out /*[n_devices][dof][B]*/);
void saip_multi_destroy(saip_multi* m);

const char* saip_last_error(void);
const char* saip_version(void);
int saip_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* SAIP_H_ */
