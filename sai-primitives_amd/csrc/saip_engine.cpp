// Host side of the engine behind include/saip.h: robot constants, task stacks, device arena, launches.
// C++ (the reference is a C++ library), HIP runtime only -- no PyTorch, no Eigen.
#include "saip_engine_internal.h"

static thread_local std::string g_err;
namespace saip {
saip_status fail_external(saip_status st, const char* fmt, ...) {  // `fail` of the engine's units, and what saip_comm.cpp calls by this name
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
	return st;
}
}  // namespace saip

// ------------------------------------------------------------------ batch
// finalized on a device; model-only batches included (state entries and model queries)
saip_status saip::eng::need_state(saip_batch* b, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (!has_device(b)) return fail(SAIP_ERR_NO_DEVICE, "%s: configuration-only batch (no HIP device): the engine has no CPU path", fn);
	if (hipSetDevice(b->device) != hipSuccess) return fail(SAIP_ERR_DEVICE, "hipSetDevice(%d) failed", b->device);
	return SAIP_OK;
}
// ... with a controller: every entry that needs a task
saip_status saip::eng::need_ready(saip_batch* b, const char* fn) {
	if (b && b->finalized && b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	return need_state(b, fn);
}
// host [comps][B] <-> device [comps][ld]
saip_status saip::eng::copy_h2d(saip_batch* b, double* dev, const double* host, int comps) {
	HIP_TRY(hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), comps,
							 hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the host buffer may be reused by the caller right away
	return SAIP_OK;
}
saip_status saip::eng::copy_d2h(saip_batch* b, double* host, const double* dev, int comps) {
	HIP_TRY(hipMemcpy2DAsync(host, (size_t)b->B * sizeof(double), dev, (size_t)b->ld * sizeof(double), (size_t)b->B * sizeof(double), comps,
							 hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
// finalized as a controller (no device needed yet: argument errors come first, as in the model queries)
saip_status saip::eng::need_controller(const saip_batch* b, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	return SAIP_OK;
}
// ---- what every resident attachment does with arrays of its own
// (alloc_zero, a template, is in the header; *p stays null when either of its calls fails)
// host [rows] or [rows][B] -> device [rows] or [rows][ld]; `what` names the table in the message ("plane", "obstacle", "table")
saip_status saip::eng::upload_table(saip_batch* b, double* dev, const double* host, size_t rows, int per_instance, const char* what, const char* fn) {
	hipError_t e;
	if (per_instance)
		e = hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), rows, hipMemcpyHostToDevice,
							 b->stream);
	else e = hipMemcpyAsync(dev, host, rows * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffer may be reused by the caller right away
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: %s upload failed: %s", fn, what, hipGetErrorString(e));
	return SAIP_OK;
}
saip_status saip::eng::check_bound_infinities(const char* fn, const char* what, size_t unit, const double* lo, const double* hi, int words, const char* const* names) {
	for (int k = 0; k < words; k++)
		if (lo[k] != hi[k] && !(std::isfinite(lo[k]) && std::isfinite(hi[k])))
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s %zu: word %s has an infinite bound on one side only", fn, what, unit, names[k]);
	return SAIP_OK;
}
saip_status saip::eng::upload_bound_pair(saip_batch* b, double* dst, const double* lo, const double* hi, size_t rows, const char* fn) {
	saip_status st = upload_table(b, dst, lo, rows, 0, "table", fn);
	return st ? st : upload_table(b, dst + rows, hi, rows, 0, "table", fn);
}
// the body of the _readout_host and _summary_host entries behind their own need-check, whose result is `st`: device [rows][ld] -> host [rows][B]
saip_status saip::eng::rows_to_host(saip_batch* b, saip_status st, double* out, const double* dev, int rows, const char* fn) {
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, dev, rows);
}
// ... and of the _summary_reset entries whose rows reset to zero, on the stream
saip_status saip::eng::zero_rows(saip_batch* b, double* dev, int rows) {
	HIP_TRY(hipMemsetAsync(dev, 0, (size_t)rows * b->ld * sizeof(double), b->stream));
	return SAIP_OK;
}

extern "C" int saip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" saip_status saip_batch_create(const saip_model* model, int batch_size, int device, saip_batch** out) {
	if (!model || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_create: null argument");
	if (batch_size <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_create: batch size must be positive");
	if (device >= 0) {
		int cnt = saip_device_count();
		if (cnt <= 0) return fail(SAIP_ERR_NO_DEVICE, "no HIP device available: the engine has no CPU path");
		if (device >= cnt) return fail(SAIP_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, cnt);
	}
	auto* b = new saip_batch();
	b->model = model;
	b->B = batch_size;
	b->ld = (batch_size + 31) / 32 * 32;
	b->device = device;  // < 0: configuration-only batch (host logic can be exercised; every compute call fails)
	*out = b;
	return SAIP_OK;
}
// leading dimension of the device arrays (default: B rounded up to 32).  Shards of a sharded run that differ by an instance all take the
// ld of the largest one, so that the final all-gather moves slabs of one shape (sharding.shard_ld)
extern "C" saip_status saip_batch_set_leading_dimension(saip_batch* b, int ld) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "the leading dimension is fixed by saip_batch_finalize");
	if (ld < b->B || ld % 32 != 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "leading dimension %d: must be a multiple of 32 and at least the batch size %d", ld, b->B);
	b->ld = ld;
	return SAIP_OK;
}
extern "C" void saip_batch_destroy(saip_batch* b) {
	if (!b) return;
	if (has_device(b)) {
		(void)hipSetDevice(b->device);
		if (b->stream) (void)hipStreamSynchronize(b->stream);  // nothing of this batch may still be in flight
		if (b->sync_event) (void)hipEventDestroy(b->sync_event);
		for (hipEvent_t e : b->time_ev)
			if (e) (void)hipEventDestroy(e);
		for (void* p : b->allocs) (void)hipFree(p);
		// the attachments free their own arrays (none of them needs the stream, which is idle and still alive here)
		record_free(b);
		for (int t = 0; t < (int)b->sched.size(); t++)
			if (b->sched[t].attached) schedule_release(b, t);  // (with the sampler on it)
		for (saip_snapshot* s : b->snapshots) snapshot_release_device(s);  // the handles stay valid for saip_snapshot_destroy
		contact_free(b);
		while (b->n_patch > 0) patch_free(b, b->n_patch - 1);
		clearance_free(b);
		link_contact_free(b);
		plant_free(b);
		inertia_free(b);
		sensing_free(b);
		guard_free(b);
		if (b->stream) (void)hipStreamDestroy(b->stream);
	}
	delete b;
}
extern "C" int saip_batch_size(const saip_batch* b) { return b ? b->B : 0; }
extern "C" int saip_batch_ld(const saip_batch* b) { return b ? b->ld : 0; }
extern "C" int saip_batch_dof(const saip_batch* b) { return (b && b->model) ? b->model->n : 0; }

saip_status saip::eng::check_batch(const saip_batch* b, int task, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	if (task >= (int)b->tasks.size() || task < -1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	return SAIP_OK;
}
static void refresh_has_ki(TaskDev& d) {
	// derived fields: pseudo-inverse of the diagonal kv gains (SaiModel::computePseudoInverse), control-law variant
	for (int c = 0; c < 3; c++) {
		d.kvinv_pos[c] = fabs(d.kv_pos[c]) > 1e-6 ? 1.0 / d.kv_pos[c] : 0.0;
		d.kvinv_ori[c] = fabs(d.kv_ori[c]) > 1e-6 ? 1.0 / d.kv_ori[c] : 0.0;
	}
	for (int c = 0; c < d.m; c++) d.kvinv[c] = fabs(d.kv[c]) > 1e-6 ? 1.0 / d.kv[c] : 0.0;
	d.general_law = (d.vel_sat || d.force_dim || d.moment_dim || d.cl_force || d.cl_moment) ? 1 : 0;
	d.has_ki = 0;
	if (d.type == saip::TASK_MOTION_FORCE) {
		for (int c = 0; c < 3; c++)
			if (d.ki_pos[c] != 0 || d.ki_ori[c] != 0) d.has_ki = 1;
	} else {
		for (int c = 0; c < d.m; c++)
			if (d.ki[c] != 0) d.has_ki = 1;
	}
}
static void task_defaults(TaskDev& d, double dt) {
	memset(&d, 0, sizeof(TaskDev));
	d.dt = dt;
	d.decoupling = SAIP_BOUNDED_INERTIA_ESTIMATES;  // MotionForceTask.h:41-43, JointTask.h:35-37
	d.bie_threshold = 0.1;
}

extern "C" saip_status saip_batch_add_motion_force_task(saip_batch* b, const char* task_name, const char* link_name,
														const double pos_in_link[3], const double rot_in_link[9],
														const double* dirs_trans, int n_trans, const double* dirs_rot, int n_rot,
														double loop_timestep, int* task_id) {
	if (!b || !task_name || !link_name || !pos_in_link) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_add_motion_force_task: null argument");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "tasks cannot be added after saip_batch_finalize");
	if ((int)b->tasks.size() >= SAIP_MAX_TASKS) return fail(SAIP_ERR_UNSUPPORTED, "more than %d tasks", SAIP_MAX_TASKS);
	int li = saip_model_link_index(b->model, link_name);
	if (li < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "link %s does not exist in the robot model", link_name);
	const LinkInfo& L = b->model->links[li];
	if (L.body < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "link %s is welded to the base: no controllable degree of freedom", link_name);
	TaskHost T;
	T.name = task_name;
	task_defaults(T.dev, loop_timestep);
	T.dev.type = saip::TASK_MOTION_FORCE;
	T.dev.body = L.body;
	double I3[9];
	m3_eye(I3);
	const double* Rin = rot_in_link ? rot_in_link : I3;
	double t[3];
	m3_vec(L.R, pos_in_link, t);
	for (int i = 0; i < 3; i++) T.dev.pos[i] = L.p[i] + t[i];
	m3_mul(L.R, Rin, T.dev.rot);
	double bt[9], br[9];
	int pr, orr;
	if (n_trans < 0 && n_rot < 0) {  // full task, MotionForceTask.cpp:28
		m3_eye(bt);
		m3_eye(br);
		pr = orr = 3;
	} else {
		if (n_trans <= 0 && n_rot <= 0)  // MotionForceTask.cpp:47-53
			return fail(SAIP_ERR_INVALID_ARGUMENT, "controlled_directions_translation and controlled_directions_rotation cannot both be empty in MotionForceTask::MotionForceTask");
		if ((n_trans > 0 && !dirs_trans) || (n_rot > 0 && !dirs_rot)) return fail(SAIP_ERR_INVALID_ARGUMENT, "null direction array");
		pr = range_basis_3(dirs_trans, n_trans > 0 ? n_trans : 0, bt);   // :55-87
		orr = range_basis_3(dirs_rot, n_rot > 0 ? n_rot : 0, br);
	}
	if (pr + orr == 0)  // :154-160
		return fail(SAIP_ERR_INVALID_ARGUMENT, "controlled_directions_translation and controlled_directions_rotation cannot both be empty in MotionForceTask::MotionForceTask");
	if (pr + orr == 1)
		return fail(SAIP_ERR_UNSUPPORTED, "rank-1 MotionForceTask: the reference's SingularityHandler never initialises its model for task_rank == 1 (SingularityHandler.cpp:100), refusing");
	memset(T.P, 0, sizeof(T.P));
	memset(T.dev.Bm, 0, sizeof(T.dev.Bm));
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) {
			double sp = 0, so = 0;
			for (int c = 0; c < pr; c++) sp += bt[3 * i + c] * bt[3 * j + c];
			for (int c = 0; c < orr; c++) so += br[3 * i + c] * br[3 * j + c];
			T.P[6 * i + j] = sp;
			T.P[6 * (3 + i) + 3 + j] = so;
			T.dev.Ppos[3 * i + j] = sp;
			T.dev.Pori[3 * i + j] = so;
		}
	for (int i = 0; i < 3; i++) {
		for (int c = 0; c < pr; c++) T.dev.Bm[6 * i + c] = bt[3 * i + c];
		for (int c = 0; c < orr; c++) T.dev.Bm[6 * (3 + i) + pr + c] = br[3 * i + c];
	}
	// sigmaPosition = Ppos (I - sigmaForce) Ppos^T with force space dimension 0 (MotionForceTask.cpp:927-930), same for orientation
	double PT[9];
	m3_T(T.dev.Ppos, PT);
	m3_mul(T.dev.Ppos, PT, T.dev.sig_p);
	m3_T(T.dev.Pori, PT);
	m3_mul(T.dev.Pori, PT, T.dev.sig_o);
	T.dev.k = pr + orr;
	T.dev.goal_comps = 36;  // x3 R9 v3 w3 a3 alpha3 + goal force 3 + goal moment 3 + sensed force 3 + sensed moment 3 (sensor frame)
	T.dev.kv_force = 10.0;   // MotionForceTask.h:51,54
	T.dev.kv_moment = 10.0;
	T.dev.lin_sat = 0.3;     // :63-64
	T.dev.ang_sat = M_PI / 3;
	T.dev.force_axis[2] = T.dev.moment_axis[2] = 1.0;
	T.dev.bm_identity = (pr == 3 && orr == 3) ? 1 : 0;
	T.dev.cert_kroot = pow((double)T.dev.k, -1.0 / 8.0);
	for (int i = 0; i < 3; i++) {  // MotionForceTask.h:44-49
		T.dev.kp_pos[i] = 100.0; T.dev.kv_pos[i] = 20.0; T.dev.ki_pos[i] = 0.0;
		T.dev.kp_ori[i] = 200.0; T.dev.kv_ori[i] = 28.3; T.dev.ki_ori[i] = 0.0;
	}
	T.dev.s_min = 6e-3;   // MotionForceTask.cpp:197
	T.dev.s_max = 6e-2;
	T.dev.s_abs_tol = 1e-3;  // SingularityHandler.cpp:11
	T.dev.sing_handling = 1; // _enforce_handling_strategy = true, SingularityHandler.cpp:61
	T.dev.sing_strategies = 1;  // the reference always runs its blended type-1 / type-2 strategies while the handling is enforced (:100-121, 146-158, 310-367)
	T.dev.sh_kp1 = 50.0;     // KP_TYPE_1, KV_TYPE_1, KV_TYPE_2, SingularityHandler.cpp:17-19
	T.dev.sh_kv1 = 14.0;
	T.dev.sh_kv2 = 5.0;
	T.integ_rows = 12;  // position 3, orientation 3, force 3, moment 3
	T.dev.kp_force = T.dev.kp_moment = 0.7;  // MotionForceTask.h:50-59
	T.dev.ki_force = T.dev.ki_moment = 1.3;
	T.dev.kff_force = T.dev.kff_moment = 0.95;
	T.dev.max_force_fb = 20.0;
	T.dev.max_moment_fb = 10.0;
	T.dev.Rcs[0] = T.dev.Rcs[4] = T.dev.Rcs[8] = 1.0;  // _T_control_to_sensor = identity, MotionForceTask.cpp:94
	refresh_has_ki(T.dev);
	memset(&T.otg, 0, sizeof(T.otg));
	T.otg.m = 6;
	T.otg.gs = 8;
	for (int i = 0; i < SAIP_MAXN; i++) T.otg_limits[i] = T.otg_limits[SAIP_MAXN + i] = T.otg_limits[2 * SAIP_MAXN + i] = 1.0;
	for (int i = 0; i < 3; i++) {  // MotionForceTask.h:68-71
		T.otg_limits[i] = 0.3;
		T.otg_limits[SAIP_MAXN + i] = 2.0;
		T.otg_limits[3 + i] = M_PI / 3.0;
		T.otg_limits[SAIP_MAXN + 3 + i] = 2.0 * M_PI;
	}
	b->tasks.push_back(T);
	b->config_dirty = true;
	if (task_id) *task_id = (int)b->tasks.size() - 1;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_add_joint_task(saip_batch* b, const char* task_name, const double* S, int rows, double loop_timestep, int* task_id) {
	if (!b || !task_name) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_add_joint_task: null argument");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "tasks cannot be added after saip_batch_finalize");
	if ((int)b->tasks.size() >= SAIP_MAX_TASKS) return fail(SAIP_ERR_UNSUPPORTED, "more than %d tasks", SAIP_MAX_TASKS);
	const int n = b->model->n;
	TaskHost T;
	T.name = task_name;
	task_defaults(T.dev, loop_timestep);
	T.dev.type = saip::TASK_JOINT;
	if (rows <= 0 || !S) {  // JointTask.cpp:18-19
		T.dev.m = n;
		T.dev.s_identity = 1;
		for (int i = 0; i < n; i++) T.dev.S[i * n + i] = 1.0;
		T.full_joint = true;
	} else {
		if (rows > n)  // a rows x n matrix with rows > n cannot have full row rank (JointTask.cpp:34-39)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "joint selection matrix is not full rank in JointTask constructor");
		// full row rank check (the reference uses FullPivLU, JointTask.cpp:34-39): Gaussian elimination with full pivoting
		std::vector<double> A(S, S + (size_t)rows * n);
		double amax = 0;
		for (double v : A) amax = fmax(amax, fabs(v));
		int rank = 0;
		std::vector<char> rused(rows, 0), cused(n, 0);
		for (int step = 0; step < rows; step++) {
			int pi = -1, pj = -1;
			double best = 0;
			for (int i = 0; i < rows; i++)
				if (!rused[i])
					for (int j = 0; j < n; j++)
						if (!cused[j] && fabs(A[(size_t)i * n + j]) > best) {
							best = fabs(A[(size_t)i * n + j]);
							pi = i;
							pj = j;
						}
			if (pi < 0 || best <= amax * 1e-12 * (rows > n ? rows : n)) break;
			rank++;
			rused[pi] = cused[pj] = 1;
			for (int i = 0; i < rows; i++)
				if (!rused[i]) {
					double f = A[(size_t)i * n + pj] / A[(size_t)pi * n + pj];
					for (int j = 0; j < n; j++) A[(size_t)i * n + j] -= f * A[(size_t)pi * n + j];
				}
		}
		if (rank != rows) return fail(SAIP_ERR_INVALID_ARGUMENT, "joint selection matrix is not full rank in JointTask constructor");
		T.dev.m = rows;
		memcpy(T.dev.S, S, sizeof(double) * rows * n);
		bool ident = (rows == n);
		for (int i = 0; i < rows && ident; i++)
			for (int j = 0; j < n; j++)
				if (S[i * n + j] != (i == j ? 1.0 : 0.0)) ident = false;
		T.dev.s_identity = ident;
		T.full_joint = (rows == n);  // JointTask::isFullJointTask(): task dof == robot dof
	}
	for (int i = 0; i < T.dev.m; i++) {  // JointTask.h:32-34
		T.dev.kp[i] = 50.0;
		T.dev.kv[i] = 14.0;
		T.dev.ki[i] = 0.0;
		T.dev.sat[i] = M_PI / 3.0;  // JointTask.h:44
	}
	T.dev.goal_comps = 3 * T.dev.m;
	T.integ_rows = T.dev.m;
	refresh_has_ki(T.dev);
	memset(&T.otg, 0, sizeof(T.otg));
	T.otg.m = T.dev.m;
	T.otg.gs = T.dev.m <= 8 ? 8 : 32;
	for (int i = 0; i < SAIP_MAXN; i++) {
		T.otg_limits[i] = M_PI / 3.0;              // DefaultParameters::otg_max_velocity, JointTask.h:40
		T.otg_limits[SAIP_MAXN + i] = 2.0 * M_PI;  // DefaultParameters::otg_max_acceleration, JointTask.h:41
		T.otg_limits[2 * SAIP_MAXN + i] = 10.0 * M_PI;  // DefaultParameters::otg_max_jerk, JointTask.h:42 (used in jerk-limited mode only)
	}
	b->tasks.push_back(T);
	b->config_dirty = true;
	if (task_id) *task_id = (int)b->tasks.size() - 1;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_finalize(saip_batch* b) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return SAIP_OK;
	// RobotController constructor checks, RobotController.cpp:8-66
	if (b->tasks.empty()) return fail(SAIP_ERR_INVALID_ARGUMENT, "RobotController must have at least one task");
	bool closed = false;
	for (size_t i = 0; i < b->tasks.size(); i++) {
		if (b->tasks[i].dev.dt != b->tasks[0].dev.dt) return fail(SAIP_ERR_INVALID_ARGUMENT, "All tasks must have the same loop timestep in RobotController");
		for (size_t j = 0; j < i; j++)
			if (b->tasks[j].name == b->tasks[i].name) return fail(SAIP_ERR_INVALID_ARGUMENT, "Tasks in RobotController must have unique names");
		if (closed)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "task [%s] cannot be added to the controller because it is in the nullspace of a full joint task", b->tasks[i].name.c_str());
		if (b->tasks[i].dev.type == saip::TASK_JOINT && b->tasks[i].full_joint) closed = true;
		// k > n: the reference's thin SVD of the k x n task Jacobian has min(k, n) singular values and SingularityHandler.cpp:78-118
		// reads k of them (undefined behaviour); the per-task interface goes through this batch too, so it is refused with it
		if (b->tasks[i].dev.type == saip::TASK_MOTION_FORCE && b->tasks[i].dev.k > b->model->n)
			return fail(SAIP_ERR_UNSUPPORTED,
						"MotionForceTask [%s] controls %d directions but the robot has only %d dof: the reference's singularity handler is undefined "
						"for a task with more directions than joints; use a partial task (controlled_directions_translation / _rotation) of at most %d directions",
						b->tasks[i].name.c_str(), b->tasks[i].dev.k, b->model->n, b->model->n);
	}
	if (has_device(b)) {
		HIP_TRY(hipSetDevice(b->device));
		HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
		const size_t n = b->model->n, ld = b->ld;
		saip_status st;
		if ((st = dev_alloc(b, &b->q, n * ld)) || (st = dev_alloc(b, &b->dq, n * ld)) || (st = dev_alloc(b, &b->tau, n * ld)) ||
			(st = dev_alloc(b, &b->status, ld)) || (st = dev_alloc(b, &b->model_dev, 1)) || (st = dev_alloc(b, &b->tasks_dev, b->tasks.size())) ||
			(st = dev_alloc(b, &b->flags.buf, 2 * (ld + 32))))
			return st;
		for (auto& T : b->tasks) {
			if ((st = dev_alloc(b, &T.goal_dev, (size_t)T.dev.goal_comps * ld)) || (st = dev_alloc(b, &T.integ_dev, (size_t)T.integ_rows * ld)) ||
				(st = dev_alloc(b, &T.integ_new_dev, (size_t)T.integ_rows * ld)))
				return st;
			T.dev.goal = T.goal_dev;
			T.dev.integ = T.integ_dev;
			T.dev.integ_new = T.integ_new_dev;
		}
		HIP_TRY(hipMemcpy(b->model_dev, &b->model->dev, sizeof(ModelDev), hipMemcpyHostToDevice));
	}
	b->finalized = true;
	b->config_dirty = true;
	return SAIP_OK;
}

extern "C" int saip_batch_task_count(const saip_batch* b) { return b ? (int)b->tasks.size() : 0; }
extern "C" int saip_batch_task_type(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return SAIP_TASK_UNDEFINED;
	return b->tasks[t].dev.type;
}
extern "C" const char* saip_batch_task_name(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return nullptr;
	return b->tasks[t].name.c_str();
}
extern "C" int saip_batch_task_by_name(const saip_batch* b, const char* name) {
	if (!b || !name) return -1;
	for (size_t i = 0; i < b->tasks.size(); i++)
		if (b->tasks[i].name == name) return (int)i;
	return -1;
}
extern "C" int saip_batch_task_dof(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return 0;
	return b->tasks[t].dev.type == saip::TASK_JOINT ? b->tasks[t].dev.m : b->tasks[t].dev.k;
}
extern "C" int saip_batch_goal_components(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return 0;
	return b->tasks[t].dev.goal_comps;
}
// projection of a motion-force task (parity tests): P 6x6 row-major, basis 6x6 row-major (first *rank columns valid)
extern "C" saip_status saip_batch_get_task_projection(const saip_batch* b, int t, double* P36, double* basis36, int* rank) {
	saip_status st = check_batch(b, t, "saip_batch_get_task_projection");
	if (st) return st;
	if (t < 0 || b->tasks[t].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "task %d is not a MotionForceTask", t);
	if (P36) memcpy(P36, b->tasks[t].P, sizeof(double) * 36);
	if (basis36) memcpy(basis36, b->tasks[t].dev.Bm, sizeof(double) * 36);
	if (rank) *rank = b->tasks[t].dev.k;
	return SAIP_OK;
}

static saip_status set_gain3(double* kp, double* kv, double* ki, const double* p, const double* v, const double* i, int n_gains, const char* who) {
	if (!p || !v || !i) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null gain pointer", who);
	if (n_gains != 1 && n_gains != 3) return fail(SAIP_ERR_INVALID_ARGUMENT, "kp, kv and ki should be of size 1 or 3 in %s", who);
	for (int c = 0; c < n_gains; c++)
		if (p[c] < 0 || v[c] < 0 || i[c] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "all gains should be positive or zero in %s", who);
	for (int c = 0; c < 3; c++) {
		kp[c] = p[n_gains == 1 ? 0 : c];
		kv[c] = v[n_gains == 1 ? 0 : c];
		ki[c] = i[n_gains == 1 ? 0 : c];
	}
	return SAIP_OK;
}
static saip_status need_type(saip_batch* b, int t, int type, const char* fn) {
	saip_status st = check_batch(b, t, fn);
	if (st) return st;
	if (t < 0 || b->tasks[t].dev.type != type) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d has the wrong type", fn, t);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_pos_control_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_pos_control_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	st = set_gain3(d.kp_pos, d.kv_pos, d.ki_pos, kp, kv, ki, ng, "MotionForceTask::setPosControlGains");
	refresh_has_ki(d);
	b->config_dirty = true;
	return st;
}
extern "C" saip_status saip_batch_set_ori_control_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_ori_control_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	st = set_gain3(d.kp_ori, d.kv_ori, d.ki_ori, kp, kv, ki, ng, "MotionForceTask::setOriControlGains");
	refresh_has_ki(d);
	b->config_dirty = true;
	return st;
}
extern "C" saip_status saip_batch_set_joint_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_JOINT, "saip_batch_set_joint_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	if (!kp || !kv || !ki) return fail(SAIP_ERR_INVALID_ARGUMENT, "JointTask::setGains: null gain pointer");
	if (ng != 1 && ng != d.m) return fail(SAIP_ERR_INVALID_ARGUMENT, "size of gain vectors inconsistent with number of task dofs in JointTask::setGains");
	for (int c = 0; c < ng; c++)
		if (kp[c] < 0 || kv[c] < 0 || ki[c] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "gains must be positive or zero in JointTask::setGains");
	for (int c = 0; c < d.m; c++) {
		d.kp[c] = kp[ng == 1 ? 0 : c];
		d.kv[c] = kv[ng == 1 ? 0 : c];
		d.ki[c] = ki[ng == 1 ? 0 : c];
	}
	refresh_has_ki(d);
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_dynamic_decoupling_type(saip_batch* b, int t, int type) {
	saip_status st = check_batch(b, t, "saip_batch_set_dynamic_decoupling_type");
	if (st) return st;
	if (t < 0 || type < 0 || type > 2) return fail(SAIP_ERR_INVALID_ARGUMENT, "Dynamic decoupling type not recognized");
	b->tasks[t].dev.decoupling = type;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_bie_threshold(saip_batch* b, int t, double thr) {
	saip_status st = check_batch(b, t, "saip_batch_set_bie_threshold");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	// JointTask clamps negative thresholds to 0 (JointTask.h:372-378); SingularityHandler stores them as-is (SingularityHandler.h:81-86)
	if (thr < 0 && b->tasks[t].dev.type == saip::TASK_JOINT) thr = 0;
	b->tasks[t].dev.bie_threshold = thr;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_bounds(saip_batch* b, int t, double s_min, double s_max) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_bounds");
	if (st) return st;
	if (s_min < 0 || s_max < s_min) return fail(SAIP_ERR_INVALID_ARGUMENT, "singularity bounds must satisfy 0 <= s_min <= s_max");
	b->tasks[t].dev.s_min = s_min;
	b->tasks[t].dev.s_max = s_max;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_handling(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_handling");
	if (st) return st;
	b->tasks[t].dev.sing_handling = enabled ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
// SingularityHandler state of every instance back to "never singular" (SingularityHandler.cpp:55-63); allocates on first use
static saip_status sh_reinit(saip_batch* b, TaskHost& T) {
	if (!T.dev.sh) {
		saip_status st = dev_alloc(b, &T.dev.sh, (size_t)b->ld);
		if (st) return st;
	}
	HIP_TRY(hipMemsetAsync(T.dev.sh, 0, (size_t)b->ld * sizeof(saip::ShState), b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_strategies(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_strategies");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.dev.sing_strategies = enabled ? 1 : 0;
	b->config_dirty = true;
	if (enabled && b->finalized && has_device(b)) {
		if ((st = need_ready(b, "saip_batch_set_singularity_strategies"))) return st;
		return sh_reinit(b, T);
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_gains(saip_batch* b, int t, double kp_type_1, double kv_type_1, double kv_type_2) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_gains");
	if (st) return st;
	b->tasks[t].dev.sh_kp1 = kp_type_1;
	b->tasks[t].dev.sh_kv1 = kv_type_1;
	b->tasks[t].dev.sh_kv2 = kv_type_2;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_all_singularities_type1(saip_batch* b, int t, int flag) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_all_singularities_type1");
	if (st) return st;
	b->tasks[t].dev.sh_force_type1 = flag ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_type1_posture(saip_batch* b, int t, const double* q_des, int per_instance) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_type1_posture");
	if (st) return st;
	if (!q_des) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_type1_posture: null posture");
	TaskHost& T = b->tasks[t];
	// _q_prior is overwritten with the current posture whenever an instance enters a singular region (SingularityHandler.cpp:232-235):
	// the call only matters for instances that are inside one, which needs the device state
	if (!T.dev.sing_strategies || !T.dev.sh || !b->finalized || !has_device(b)) return SAIP_OK;
	if ((st = need_ready(b, "saip_batch_set_type1_posture"))) return st;
	const int n = b->model->n;
	std::vector<double> host((size_t)b->B * n);
	for (int i = 0; i < b->B; i++)
		for (int j = 0; j < n; j++) host[(size_t)i * n + j] = per_instance ? q_des[(size_t)i * n + j] : q_des[j];
	HIP_TRY(hipMemcpy2DAsync(T.dev.sh, sizeof(saip::ShState), host.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)b->B,
							 hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_internal_otg(saip_batch* b, int t, int enabled) {
	saip_status st = check_batch(b, t, "saip_batch_set_internal_otg");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (enabled && !T.otg_enabled) T.otg_inited = false;  // enableInternalOtg* re-initialises a disabled OTG (JointTask.cpp:374-376)
	T.otg_enabled = enabled != 0;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_otg_acceleration_limited(saip_batch* b, int t, const double* max_velocity, const double* max_acceleration, int count) {
	saip_status st = check_batch(b, t, "saip_batch_set_otg_acceleration_limited");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (T.dev.type == saip::TASK_MOTION_FORCE) {
		// MotionForceTask::enableInternalOtgAccelerationLimited(max_lin_vel, max_lin_acc, max_ang_vel, max_ang_acc), MotionForceTask.cpp:510-523
		if (!max_velocity || !max_acceleration || count != 2)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "motion-force task: pass {linear, angular} max velocities and max accelerations (count = 2)");
		for (int i = 0; i < 2; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sVelocity", i ? "Angular" : "Linear");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sAcceleration", i ? "Angular" : "Linear");
		}
		for (int i = 0; i < 6; i++) {
			T.otg_limits[i] = max_velocity[i / 3];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[i / 3];
		}
		T.otg_limits_dirty = true;
		T.otg.epoch++;
		if (!T.otg_enabled || T.otg.jerk) T.otg_inited = false;  // MotionForceTask.cpp:513-515: re-initialised when the OTG was off or jerk-limited
		T.otg.jerk = 0;
		T.otg_enabled = true;
		b->config_dirty = true;
		return SAIP_OK;
	}
	const int m = T.dev.m;
	if (!max_velocity || !max_acceleration || (count != 1 && count != m))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity or max acceleration vector size not consistent with task dof in JointTask::enableInternalOtgAccelerationLimited");
	for (int i = 0; i < count; i++) {
		if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity");
		if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration");
	}
	for (int i = 0; i < m; i++) {
		T.otg_limits[i] = max_velocity[count == 1 ? 0 : i];
		T.otg_limits[SAIP_MAXN + i] = max_acceleration[count == 1 ? 0 : i];
	}
	T.otg_limits_dirty = true;
	T.otg.epoch++;
	if (!T.otg_enabled || T.otg.jerk) T.otg_inited = false;  // JointTask.cpp:374-376
	T.otg.jerk = 0;
	T.otg_enabled = true;
	b->config_dirty = true;
	return SAIP_OK;
}
// JointTask::enableInternalOtgJerkLimited (JointTask.cpp:383-410; OTG_joints::setMaxVelocity / setMaxAcceleration / setMaxJerk, OTG_joints.cpp:44-86) and
// MotionForceTask::enableInternalOtgJerkLimited (MotionForceTask.cpp:525-545; OTG_6dof_cartesian::setMaxJerk, OTG_6dof_cartesian.cpp:126-136):
// third-order Ruckig profiles on the device (csrc/saip_otg3.h).  The OTG is re-initialised at the current task position when it was off or
// acceleration-limited (:400-402 / :530-532).
extern "C" saip_status saip_batch_set_otg_jerk_limited(saip_batch* b, int t, const double* max_velocity, const double* max_acceleration, const double* max_jerk, int count) {
	saip_status st = check_batch(b, t, "saip_batch_set_otg_jerk_limited");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (T.dev.type == saip::TASK_MOTION_FORCE) {
		if (!max_velocity || !max_acceleration || !max_jerk || count != 2)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "motion-force task: pass {linear, angular} max velocities, max accelerations and max jerks (count = 2)");
		for (int i = 0; i < 2; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sVelocity", i ? "Angular" : "Linear");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sAcceleration", i ? "Angular" : "Linear");
			if (!(max_jerk[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max jerk set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxJerk");
		}
		for (int i = 0; i < 6; i++) {
			T.otg_limits[i] = max_velocity[i / 3];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[i / 3];
			T.otg_limits[2 * SAIP_MAXN + i] = max_jerk[i / 3];
		}
	} else {
		const int m = T.dev.m;
		if (!max_velocity || !max_acceleration || !max_jerk || (count != 1 && count != m))
			return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity, max acceleration or max jerk vector size not consistent with task dof in JointTask::enableInternalOtgJerkLimited");
		for (int i = 0; i < count; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration");
			if (!(max_jerk[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max jerk cannot be 0 or negative in any directions in OTG_joints::setMaxJerk");
		}
		for (int i = 0; i < m; i++) {
			T.otg_limits[i] = max_velocity[count == 1 ? 0 : i];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[count == 1 ? 0 : i];
			T.otg_limits[2 * SAIP_MAXN + i] = max_jerk[count == 1 ? 0 : i];
		}
	}
	T.otg_limits_dirty = true;
	T.otg.epoch++;
	if (!T.otg_enabled || !T.otg.jerk) T.otg_inited = false;
	T.otg.jerk = 1;
	T.otg_enabled = true;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_velocity_saturation(saip_batch* b, int t, int enabled) {
	saip_status st = check_batch(b, t, "saip_batch_set_velocity_saturation");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	b->tasks[t].dev.vel_sat = enabled ? 1 : 0;
	refresh_has_ki(b->tasks[t].dev);
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_saturation_velocities(saip_batch* b, int t, const double* v, int nv) {
	saip_status st = check_batch(b, t, "saip_batch_set_saturation_velocities");
	if (st) return st;
	if (t < 0 || (nv > 0 && !v)) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task or null values");
	TaskDev& d = b->tasks[t].dev;
	if (d.type == saip::TASK_MOTION_FORCE) {
		if (nv != 2) return fail(SAIP_ERR_INVALID_ARGUMENT, "MotionForceTask::enableVelocitySaturation takes a linear and an angular saturation velocity");
		if (v[0] <= 0 || v[1] <= 0)  // MotionForceTask.cpp:773-777
			return fail(SAIP_ERR_INVALID_ARGUMENT, "Velocity saturation values should be strictly positive or zero in MotionForceTask::enableVelocitySaturation");
		d.lin_sat = v[0];
		d.ang_sat = v[1];
	} else {
		if (nv != 1 && nv != d.m)  // JointTask.cpp:423-427
			return fail(SAIP_ERR_INVALID_ARGUMENT, "saturation velocity vector size not consistent with task dof in JointTask::enableVelocitySaturation");
		for (int i = 0; i < nv; i++)
			if (v[i] <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saturation velocity must be positive in JointTask::enableVelocitySaturation");
		for (int i = 0; i < d.m; i++) d.sat[i] = v[nv == 1 ? 0 : i];
	}
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_parametrization_in_compliant_frame(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_parametrization_in_compliant_frame");
	if (st) return st;
	b->tasks[t].dev.param_in_compliant_frame = enabled ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
static saip_status set_fm_gains(saip_batch* b, int t, double kp, double kv, double ki, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	if (kp < 0 || kv < 0 || ki < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "all gains should be positive or zero in %s", who);
	TaskDev& d = b->tasks[t].dev;
	(moment ? d.kv_moment : d.kv_force) = kv;
	(moment ? d.kp_moment : d.kp_force) = kp;  // kp, ki only act in closed-loop control
	(moment ? d.ki_moment : d.ki_force) = ki;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_force_control_gains(saip_batch* b, int t, double kp, double kv, double ki) {
	return set_fm_gains(b, t, kp, kv, ki, false, "MotionForceTask::setForceControlGains");
}
extern "C" saip_status saip_batch_set_moment_control_gains(saip_batch* b, int t, double kp, double kv, double ki) {
	return set_fm_gains(b, t, kp, kv, ki, true, "MotionForceTask::setMomentControlGains");
}
// setClosedLoopForceControl / setClosedLoopMomentControl (MotionForceTask.cpp:973-986): a change resets the linear / angular integrators
static saip_status set_closed_loop(saip_batch* b, int t, int enabled, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	int& flag = moment ? d.cl_moment : d.cl_force;
	const bool changed = (flag != 0) != (enabled != 0);
	flag = enabled ? 1 : 0;
	refresh_has_ki(d);
	b->config_dirty = true;
	if (changed && b->finalized && has_device(b)) {
		// resetIntegratorsLinear / Angular: position + force (orientation + moment) integrators := 0
		const int rows[2] = {moment ? 3 : 0, moment ? 9 : 6};
		for (int r : rows) HIP_TRY(hipMemsetAsync(b->tasks[t].integ_dev + (size_t)r * b->ld, 0, (size_t)3 * b->ld * sizeof(double), b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_closed_loop_force_control(saip_batch* b, int t, int enabled) {
	return set_closed_loop(b, t, enabled, false, "saip_batch_set_closed_loop_force_control");
}
extern "C" saip_status saip_batch_set_closed_loop_moment_control(saip_batch* b, int t, int enabled) {
	return set_closed_loop(b, t, enabled, true, "saip_batch_set_closed_loop_moment_control");
}
// POPCExplicitForceControl::reInitialize (POPCExplicitForceControl.cpp:10-22) for every instance; allocates the state on first use
static saip_status popc_reinit(saip_batch* b, TaskHost& T) {
	const int cap = T.dev.popc_cap;
	const size_t rows = 7 + (size_t)cap, ld = b->ld;
	if (!T.dev.popc) {
		saip_status st = dev_alloc(b, &T.dev.popc, rows * ld);
		if (st) return st;
	}
	HIP_TRY(hipMemsetAsync(T.dev.popc, 0, rows * ld * sizeof(double), b->stream));
	std::vector<double> one(ld, 1.0), fifty(ld, 50.0);  // _Rc = 1, _PO_counter = _PO_max_counter
	HIP_TRY(hipMemcpyAsync(T.dev.popc + 2 * ld, one.data(), ld * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipMemcpyAsync(T.dev.popc + 4 * ld, fifty.data(), ld * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
// enablePassivity / disablePassivity (MotionForceTask.h:630-631 -> POPCExplicitForceControl::enable / disable, .cpp:24-29)
extern "C" saip_status saip_batch_set_passivity(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_passivity");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.dev.popc_enabled = enabled ? 1 : 0;
	if (T.dev.popc_cap == 0) T.dev.popc_cap = 1024;
	b->config_dirty = true;
	if (b->finalized && has_device(b)) {
		if ((st = need_ready(b, "saip_batch_set_passivity"))) return st;
		if (!enabled || !T.dev.popc) return popc_reinit(b, T);  // disable() re-initialises; the first enable() creates the state
	}
	return SAIP_OK;
}
// setFeedforwardForceGain / MomentGain, setMaxForceControlFeedbackOutput / Moment (MotionForceTask.h:330-355)
extern "C" saip_status saip_batch_set_force_control_parameters(saip_batch* b, int t, double kff_force, double kff_moment, double max_force_feedback, double max_moment_feedback) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_force_control_parameters");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	d.kff_force = kff_force;
	d.kff_moment = kff_moment;
	d.max_force_fb = max_force_feedback;
	d.max_moment_fb = max_moment_feedback;
	b->config_dirty = true;
	return SAIP_OK;
}
// setForceSensorFrame (MotionForceTask.cpp:794-803), given directly as _T_control_to_sensor = compliant_frame^-1 * T_link_sensor
extern "C" saip_status saip_batch_set_control_to_sensor_transform(saip_batch* b, int t, const double* R_row_major, const double* translation) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_control_to_sensor_transform");
	if (st) return st;
	if (!R_row_major || !translation) return fail(SAIP_ERR_INVALID_ARGUMENT, "null transform");
	TaskDev& d = b->tasks[t].dev;
	for (int i = 0; i < 9; i++) d.Rcs[i] = R_row_major[i];
	for (int i = 0; i < 3; i++) d.tcs[i] = translation[i];
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_gravity_compensation(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->gravity_comp = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_joint_limit_avoidance(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->jla = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_torque_saturation(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->torque_sat = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_flagged_torque_policy(saip_batch* b, int nan) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->flag_nan = nan != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_flagged_recompute(saip_batch* b, int on_list) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->flagged_on_list = on_list != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_integrator_tracking(saip_batch* b, int always) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->integ_always = always != 0;
	return SAIP_OK;
}


extern "C" saip_status saip_batch_set_state_host(saip_batch* b, const double* q, const double* dq) {
	saip_status st = need_state(b, "saip_batch_set_state_host");
	if (st) return st;
	if (!q || !dq) return fail(SAIP_ERR_INVALID_ARGUMENT, "null state pointer");
	b->models_valid = false;
	b->state_epoch++;
	if ((st = copy_h2d(b, b->q, q, b->model->n))) return st;
	b->state_pushed = true;
	return copy_h2d(b, b->dq, dq, b->model->n);
}
extern "C" saip_status saip_batch_set_goal_host(saip_batch* b, int t, const double* goal) {
	saip_status st = need_ready(b, "saip_batch_set_goal_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !goal) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null goal");
	return copy_h2d(b, b->tasks[t].goal_dev, goal, b->tasks[t].dev.goal_comps);
}
extern "C" saip_status saip_batch_set_goal_field_host(saip_batch* b, int t, int first, int count, const double* values) {
	saip_status st = need_ready(b, "saip_batch_set_goal_field_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !values) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null values");
	if (first < 0 || count <= 0 || first + count > b->tasks[t].dev.goal_comps)  // e.g. JointTask.cpp:110-114
		return fail(SAIP_ERR_INVALID_ARGUMENT, "goal vector size not consistent with task dof");
	return copy_h2d(b, b->tasks[t].goal_dev + (size_t)first * b->ld, values, count);
}
extern "C" saip_status saip_batch_get_goal_host(saip_batch* b, int t, double* goal) {
	saip_status st = need_ready(b, "saip_batch_get_goal_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !goal) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null goal");
	return copy_d2h(b, goal, b->tasks[t].goal_dev, b->tasks[t].dev.goal_comps);
}

extern "C" double* saip_batch_device_q(saip_batch* b) { return b ? b->q : nullptr; }
extern "C" double* saip_batch_device_dq(saip_batch* b) { return b ? b->dq : nullptr; }
extern "C" double* saip_batch_device_goal(saip_batch* b, int t) { return (b && t >= 0 && t < (int)b->tasks.size()) ? b->tasks[t].goal_dev : nullptr; }
extern "C" double* saip_batch_device_tau(saip_batch* b) { return b ? commanded_tau(b) : nullptr; }
extern "C" uint8_t* saip_batch_device_status(saip_batch* b) { return b ? b->status : nullptr; }
extern "C" saip_status saip_batch_bind_tau_device(saip_batch* b, double* tau_dev) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->tau_bound = tau_dev;
	return SAIP_OK;
}
extern "C" void* saip_batch_stream(saip_batch* b) { return b ? (void*)b->stream : nullptr; }

// lazily allocate the OTG state of a joint task: [fields][B*gs] lane-major doubles + per-instance scalars
static saip_status ensure_otg(saip_batch* b, TaskHost& T) {
	if (T.otg_alloc) return SAIP_OK;
	saip_status st;
	OtgDev& O = T.otg;
	O.lanes = (long long)b->B * O.gs;
	O.dt = T.dev.dt;
	O.n = b->model->n;
	if ((st = dev_alloc(b, &O.state, (size_t)saip::otg_state_fields() * (size_t)O.lanes)) || (st = dev_alloc(b, &O.time, (size_t)b->ld)) ||
		(st = dev_alloc(b, &O.duration, (size_t)b->ld)) || (st = dev_alloc(b, &O.flags, (size_t)b->ld)) || (st = dev_alloc(b, &O.seen_epoch, (size_t)b->ld)) ||
		(st = dev_alloc(b, &O.result, (size_t)b->ld)) || (st = dev_alloc(b, &T.desired_dev, (size_t)T.dev.goal_comps * b->ld)) ||
		(st = dev_alloc(b, &T.otg_limits_dev, (size_t)3 * SAIP_MAXN)))
		return st;
	if (T.dev.type == saip::TASK_MOTION_FORCE && (st = dev_alloc(b, &O.frame, (size_t)21 * b->ld))) return st;
	O.model = b->model_dev;
	O.goal_comps = T.dev.goal_comps;
	O.limits = T.otg_limits_dev;
	T.otg_limits_dirty = true;
	O.desired = T.desired_dev;
	O.goal = T.goal_dev;
	O.q = b->q;
	T.otg_alloc = true;
	T.otg_inited = false;
	return SAIP_OK;
}
// mode 1: OTG_joints::reInitialize(S q) for every instance; mode 0: one cycle of setGoal + update
static saip_status run_otg(saip_batch* b, int t, int mode, int mask = 3) {
	TaskHost& T = b->tasks[t];
	T.otg.goal_comps = T.dev.goal_comps;
	T.otg.task = b->tasks_dev + t;
	T.otg.dt = T.dev.dt;
	T.otg.q = controller_q(b);  // (the measured copy while a sensing model is attached)
	if (T.otg_limits_dirty) {
		HIP_TRY(hipMemcpyAsync(T.otg_limits_dev, T.otg_limits, sizeof(T.otg_limits), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));  // limits change rarely; keeps the host array free to change again
		T.otg_limits_dirty = false;
	}
	hipError_t e = T.dev.type == saip::TASK_JOINT ? saip::launch_otg_joints(T.otg, b->B, b->ld, mode, b->stream)
												  : saip::launch_otg_cartesian(T.otg, b->B, b->ld, mode | (mask << 4), b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "OTG kernel launch failed: %s", hipGetErrorString(e));
	if (mode == 1 && mask == 3) T.otg_inited = true;
	return SAIP_OK;
}

static bool m3_is_eye(const double* A) {
	for (int i = 0; i < 9; i++)
		if (A[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
	return true;
}
// a motion-force task that controls all of its space in motion: identity projections and, where the short control law is used, identity
// sigma matrices as well
static bool mf_full_identity(const TaskDev& d, bool with_sigma) {
	return m3_is_eye(d.Ppos) && m3_is_eye(d.Pori) && (!with_sigma || (m3_is_eye(d.sig_p) && m3_is_eye(d.sig_o)));
}

// the lazily allocated state arrays every enabled feature needs: what the first cycle would allocate (state snapshots call it too, so
// that a snapshot created before the first cycle has the layout the cycles will use)
saip_status saip::eng::ensure_lazy_state(saip_batch* b) {
	for (auto& T : b->tasks) {
		if (T.otg_enabled) {
			saip_status st = ensure_otg(b, T);
			if (st) return st;
		}
		if (T.dev.type == saip::TASK_MOTION_FORCE && T.dev.sing_strategies && !T.dev.sh) {  // enabled before finalize
			saip_status st = sh_reinit(b, T);
			if (st) return st;
			b->config_dirty = true;
		}
		if (T.dev.type == saip::TASK_MOTION_FORCE && T.dev.popc_enabled && !T.dev.popc) {  // enabled before finalize
			saip_status st = popc_reinit(b, T);
			if (st) return st;
			b->config_dirty = true;
		}
	}
	return SAIP_OK;
}
// The launch words of the eight-lane kernels (CycleParams::lw): what they read of the model block, of the stack's first motion-force
// task and of its first joint task, derived from the host copies the blocks were uploaded from.  The one place that does so: a word and
// its field cannot disagree.
static CycleParams::LaunchWords launch_words(const ModelDev& md, const TaskDev* mf, const TaskDev* jt) {
	CycleParams::LaunchWords w = {};
	w.all_axis_z = md.all_axis_z;
	if (jt) {
		w.jt_dec = jt->decoupling;
		w.jt_has_ki = jt->has_ki;
		w.jt_vel_sat = jt->vel_sat;
		w.jt_dt = jt->dt;
	}
	if (!mf) return w;
	w.body = mf->body;
	w.sing_handling = mf->sing_handling;
	w.strategies_on = (mf->sing_handling && mf->sing_strategies && mf->sh != nullptr) ? 1 : 0;
	w.mf_dec = mf->decoupling;
	w.mf_has_ki = mf->has_ki;
	w.dt = mf->dt;
	w.s_max = mf->s_max;
	w.s_abs_tol = mf->s_abs_tol;
	w.cert_kroot = mf->cert_kroot;
	for (int e = 0; e < 3; e++) w.pos[e] = mf->pos[e];
	for (int e = 0; e < 9; e++) w.rot[e] = mf->rot[e];
	const double* const gains[6] = {mf->kp_pos, mf->kv_pos, mf->ki_pos, mf->kp_ori, mf->kv_ori, mf->ki_ori};
	for (int k = 0; k < 6; k++)
		for (int e = 0; e < 3; e++) w.gain[3 * k + e] = gains[k][e];
	return w;
}
// reads_state: a launch that reads the controller's state follows (with a sensing model attached, the measurement is made current first)
static saip_status make_params(saip_batch* b, CycleParams& P, bool diag, bool reads_state = true) {
	{
		saip_status st = ensure_lazy_state(b);
		if (st) return st;
		// (in front of a diagnostic launch too: it reads the true state itself, but may have to initialise an internal OTG first)
		if (reads_state && (st = sensing_refresh(b))) return st;
	}
	if (b->config_dirty || diag) {
		std::vector<TaskDev> tmp;
		for (auto& T : b->tasks) {
			TaskDev d = T.dev;
			d.diag_N = diag ? T.diag_dev : nullptr;
			if (T.otg_enabled) d.goal = T.desired_dev;  // the law tracks the OTG output (JointTask.cpp:317-319, MotionForceTask.cpp:394-406)
			d.law_identity = 0;
			if (d.type == saip::TASK_MOTION_FORCE && d.k == 6 && !d.general_law) {
				bool id = mf_full_identity(d, true);
				for (int i = 0; i < 36 && id; i++) id = d.Bm[i] == ((i % 7 == 0) ? 1.0 : 0.0);
				d.law_identity = id ? 1 : 0;
			}
			tmp.push_back(d);
		}
		HIP_TRY(hipMemcpyAsync(b->tasks_dev, tmp.data(), tmp.size() * sizeof(TaskDev), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));  // tmp is a stack object
		b->config_dirty = diag;  // a diagnostic upload must be replaced before the next normal launch
	}
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.nt = (int)b->tasks.size();
	P.sim_substeps = 0;
	P.sim_dt = P.sim_damping = 0.0;
	P.sim_gravity[0] = P.sim_gravity[1] = P.sim_gravity[2] = 0.0;
	P.gravity_comp = b->gravity_comp;
	P.torque_sat = b->torque_sat;
	P.integ_always = b->integ_always;
	P.jla = b->jla;
	P.only_flagged = 0;
	P.diag = diag;
	// what the controller reads: the measured copy of a sensing model, except in a diagnostic launch, which reports where the robot is
	P.q = diag ? b->q : controller_q(b);
	P.dq = diag ? b->dq : controller_dq(b);
	P.tau = commanded_tau(b);
	P.status = b->status;
	if (diag) {
		// a diagnostic launch re-evaluates the task models only (phase 1: no control law, no integrator / OTG / handler / passivity state
		// is advanced) and writes its torques and status to scratch: the results of the last cycle stay what integrate() / getTorques() see
		saip_status st;
		if (!b->diag_tau && ((st = dev_alloc(b, &b->diag_tau, (size_t)b->model->n * b->ld)) || (st = dev_alloc(b, &b->diag_status, (size_t)b->ld)))) return st;
		P.tau = b->diag_tau;
		P.status = b->diag_status;
	}
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	for (int t = 0; t < 2; t++) {
		P.goal2[t] = t < (int)b->tasks.size() ? (b->tasks[t].otg_enabled ? b->tasks[t].desired_dev : b->tasks[t].dev.goal) : nullptr;  // (as in the task block uploaded above)
		P.integ2[t] = t < (int)b->tasks.size() ? b->tasks[t].dev.integ : nullptr;
	}
	// lane kernel: motion-force task slots, batch-uniform rank bounds, the shared BIE threshold
	P.mf_task[0] = P.mf_task[1] = -1;
	P.any_bie = 0;
	P.bie_thr = 0.0;
	int nmf = 0, used = 0;
	for (int t = 0; t < SAIP_MAXT; t++) P.rank_bound[t] = P.lane_task_is_joint[t] = 0;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskDev& d = b->tasks[t].dev;
		int own = d.type == saip::TASK_MOTION_FORCE ? d.k : d.m;
		int bound = own < P.n - used ? own : P.n - used;  // rank(J N_prec) <= n - sum of the ranks certified above
		P.rank_bound[t] = bound < 0 ? 0 : bound;
		P.lane_task_is_joint[t] = d.type == saip::TASK_JOINT;
		if (d.type == saip::TASK_MOTION_FORCE) {
			if (nmf < 2) P.mf_task[nmf] = (int)t;
			nmf++;
			used += d.k;  // exact whenever the instance stays in the non-singular branch (otherwise it is flagged anyway)
		}
		if (d.decoupling == SAIP_BOUNDED_INERTIA_ESTIMATES) {
			P.any_bie = 1;
			P.bie_thr = d.bie_threshold;
		}
	}
	{
		const TaskDev* jt = nullptr;
		for (size_t t = 0; t < b->tasks.size() && !jt; t++)
			if (b->tasks[t].dev.type == saip::TASK_JOINT) jt = &b->tasks[t].dev;
		P.lw = launch_words(b->model->dev, P.mf_task[0] >= 0 ? &b->tasks[P.mf_task[0]].dev : nullptr, jt);
	}
	P.reinit_task = -1;
	P.reinit_mask = 7;
	P.single_task = -1;
	P.phase = diag ? 1 : 0;
	P.ext_nprec = nullptr;
	P.ext_tau_prec = nullptr;
	P.out_N = nullptr;
	P.out_Ntot = nullptr;
	for (int t = 0; t < SAIP_MAXT; t++) P.task_cycle[t] = t < (int)b->tasks.size() ? b->tasks[t].sh_cycle : 0;
	P.flag_nan = b->flag_nan ? 1 : 0;
	// neutral: no work list, no slow tail, the lean eight-lane instantiation.  launch_cycle alone overwrites these, from its CyclePlan
	P.flag_count = P.flag_count_next = P.flag_list = nullptr;
	P.slow_tail = P.oct_general_joint = P.oct_partial_mf = P.oct_truncate = 0;
	P.lane_general = 0;
	for (auto& T : b->tasks)
		if (T.dev.general_law) P.lane_general = 1;
	P.wave_general_joint = 0;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskDev& T = b->tasks[t].dev;
		if (T.type == saip::TASK_JOINT && !(T.s_identity && T.m == P.n && t + 1 == b->tasks.size())) P.wave_general_joint = 1;
	}
	P.lane_prefetch_ok = (b->tasks.size() == 2 && b->tasks[0].dev.type == saip::TASK_MOTION_FORCE && b->tasks[1].dev.type == saip::TASK_JOINT &&
						  b->tasks[1].dev.m == P.n && !b->tasks[0].dev.general_law) ? 1 : 0;
	return SAIP_OK;
}
// the task constants on the device made current (uploaded when the configuration changed), for launches that read them without a cycle
saip_status saip::eng::ensure_task_constants(saip_batch* b) {
	CycleParams P;
	return make_params(b, P, false, false);
}
// the lane-per-instance register kernel covers 6..8 dof, at most two motion-force tasks and one shared BIE threshold
static bool lane_eligible(const saip_batch* b) {
	const int n = b->model->n;
	if (n < 6 || n > 8 || b->model->dev.is_tree) return false;  // (chains only: the fast kernels scan along the chain)
	int nmf = 0;
	double thr = -1.0;
	for (auto& T : b->tasks) {
		if (T.dev.type == saip::TASK_MOTION_FORCE) nmf++;
		// closed-loop force / moment control runs in the lane kernel's general-law instantiations; with the passivity controller around
		// the force loop (per-instance energy window in HBM) the stack stays with the general kernel
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.cl_force || T.dev.cl_moment) && T.dev.popc_enabled) return false;
		if (T.dev.decoupling == SAIP_BOUNDED_INERTIA_ESTIMATES) {
			if (thr >= 0.0 && thr != T.dev.bie_threshold) return false;
			thr = T.dev.bie_threshold;
		}
	}
	return nmf <= 2;
}
// wavefront-per-instance kernel (saip_kernel_wave.hip): chains of 9..32 dof, any stack of motion-force tasks (rank >= 2) and joint tasks.
// A passivity controller around a force loop keeps its stack on the general kernel: its observer state in HBM is advanced by the control
// law itself, so an instance this kernel flags late in the hierarchy would advance it twice when the general kernel recomputes it.
static bool wave_eligible(const saip_batch* b) {
	const int n = b->model->n;
	if (n <= 8 || n > 32 || b->model->dev.is_tree) return false;
	for (auto& T : b->tasks) {
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.cl_force || T.dev.cl_moment) && T.dev.popc_enabled) return false;
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.k < 2 || T.dev.k > 6)) return false;
	}
	return true;
}
// eight-lanes-per-instance kernel (saip_kernel_oct.hip): 7-dof chain, { MotionForceTask, JointTask }.  Either the headline stack
// (full 6-dof motion-force task + full joint task: the joint task has rank <= 1) or any motion-force task of rank >= 2 with a joint
// task of at most four rows (general range basis); default or general control laws, no closed-loop force control.
static OctFit oct_eligible(const saip_batch* b) {  // (on top of lane_eligible)
	OctFit fit;
	const int n = b->model->n;
	if (n < 6 || n > 8 || b->tasks.size() != 2 || b->model->dev.is_tree) return fit;
	const TaskDev& mf = b->tasks[0].dev;
	const TaskDev& jt = b->tasks[1].dev;
	if (mf.type != saip::TASK_MOTION_FORCE || jt.type != saip::TASK_JOINT) return fit;
	if (mf.cl_force || mf.cl_moment || mf.k < 2) return fit;
	const bool full_mf = mf.k == 6 && mf.bm_identity;
	const bool full_jt = jt.m == n && jt.s_identity;
	if (!full_mf && mf.general_law) return fit;  // the general laws are wired for the full task only
	// full task: the projections are identities; the short control law also relies on identity sigma matrices
	if (full_mf && !mf_full_identity(mf, !mf.general_law)) return fit;
	if (n != 7) {
		// 6- and 8-dof chains: the general instantiation only -- full joint task behind a motion-force task, Jp = N_1 of rank n - k (<= 5) by the
		// multi-pivot Gram-Schmidt path; singularity handling on (a reduced task would need the 7-dof bookkeeping), no joint limit avoidance
		if (!full_jt || n - mf.k > 5 || n - mf.k < 0 || !mf.sing_handling || b->jla) return fit;
		fit.general_joint = 2;
	} else {
		const bool full_behind_partial = full_jt && !full_mf && mf.k <= 5;  // Jp = N_1 has rank 7 - k: multi-pivot Gram-Schmidt path
		if (!(full_mf && full_jt) && !full_behind_partial && jt.m > 4) return fit;
		fit.general_joint = (full_mf && full_jt) ? 0 : (full_behind_partial ? 2 : 1);
		if (full_mf && full_jt && !mf.sing_handling && !mf.general_law) {  // disableSingularityHandling(): reduced tasks need the multi-pivot joint-task path
			fit.general_joint = 2;
			fit.truncate = 1;
		}
	}
	fit.partial_mf = full_mf ? 0 : 1;
	fit.ok = true;
	return fit;
}
// eight-lanes-per-instance kernel for hierarchies that START with a joint task (saip_kernel_octjf.hip): 7- or 8-dof chain,
// { JointTask of <= 4 rows, each selecting one joint; full 6-dof MotionForceTask in its nullspace } -- the stack of examples/06.
// Default or general (open-loop) control laws, any decoupling type, gravity compensation, torque saturation; joint limit avoidance and
// closed-loop force control keep the stack on the lane kernel.
static bool octjf_eligible(const saip_batch* b) {  // (on top of lane_eligible)
	const int n = b->model->n;
	if ((n != 7 && n != 8) || b->tasks.size() != 2 || b->jla || b->model->dev.is_tree) return false;
	const TaskDev& jt = b->tasks[0].dev;
	const TaskDev& mf = b->tasks[1].dev;
	if (jt.type != saip::TASK_JOINT || mf.type != saip::TASK_MOTION_FORCE) return false;
	if (jt.m < 1 || jt.m > 4 || n - jt.m < 6) return false;  // (fewer than six joints left: the 6-dof task behind is always singular)
	unsigned seen = 0;
	for (int a = 0; a < jt.m; a++) {  // rows of S: distinct unit vectors (S then has full row rank: matrixRangeBasis returns the identity)
		int hit = -1;
		for (int l = 0; l < n; l++) {
			const double v = jt.S[a * n + l];
			if (v == 1.0 && hit < 0) hit = l;
			else if (v != 0.0) return false;
		}
		if (hit < 0 || (seen >> hit & 1u)) return false;
		seen |= 1u << hit;
	}
	if (mf.k != 6 || !mf.bm_identity || mf.cl_force || mf.cl_moment) return false;  // (goal rows 30..35, the sensed force and moment, are only read by the closed-loop laws)
	return mf_full_identity(mf, false);
}
// both OTGs of a { MotionForceTask, JointTask } stack on, initialised and with clean limits: their cycle-mode steps share one launch
bool saip::eng::otg_pair_ready(saip_batch* b) {
	if (!(b->tasks.size() == 2 && b->tasks[0].otg_enabled && b->tasks[1].otg_enabled && b->tasks[0].dev.type == saip::TASK_MOTION_FORCE &&
		  b->tasks[1].dev.type == saip::TASK_JOINT && b->tasks[1].otg.gs == 8 && !b->tasks[0].otg_limits_dirty && !b->tasks[1].otg_limits_dirty &&
		  !b->tasks[0].otg.jerk && !b->tasks[1].otg.jerk))
		return false;
	for (int t = 0; t < 2; t++) {
		TaskHost& T = b->tasks[t];
		if (!T.otg_inited) return false;
		T.otg.goal_comps = T.dev.goal_comps;
		T.otg.task = b->tasks_dev + t;
		T.otg.dt = T.dev.dt;
		T.otg.q = controller_q(b);
	}
	return true;
}

// ---- which cycle kernel a launch takes, who recomputes the instances it flags, and whether it integrates the state as well: decided
// here and nowhere else.  A pure function of the batch and the parameter block; launch_cycle carries the plan out.
static CyclePlan plan_cycle(const saip_batch* b, const CycleParams& P, bool diag, bool wants_sim) {
	CyclePlan plan;
	const KernelChoice choice = b->kernel_choice;
	auto refuse = [&plan](const char* why) {
		plan.refused = SAIP_ERR_UNSUPPORTED;
		plan.why = why;
		return plan;
	};
	if (diag || choice == KernelChoice::Wg) return plan;  // diagnostic launches always take the general kernel
	const bool lane = lane_eligible(b);
	if (lane) plan.oct = oct_eligible(b);
	const bool octjf_ok = lane && !plan.oct.ok && octjf_eligible(b);
	if (choice == KernelChoice::Oct && !plan.oct.ok && !octjf_ok) return refuse(kOctRefusal);
	if (lane) {
		// small batches of the headline stack: eight lanes per instance (the lane kernel would leave most of the chip idle)
		// Up to which batch: 1024 wavefronts (8192 instances) are resident at once, larger launches run in rounds.  Measured against the lane
		// kernel (round 3): the lean instantiation (config 2's stack) stays ahead up to 24 576 instances (26.8 against
		// 31.1 us) and is level at 32 768; every other instantiation -- partial tasks, reduced tasks, joint task first, 6 / 8 dof -- is ahead
		// at every size (config 3: 109 against 195 us at 65 536, 384 against 627 at 262 144; config 6: 102 against 190 at 65 536), and
		// stacks whose instances leave the non-singular branch are not a contest (the lane kernel hands those to the general kernel).
		const bool oct_lean = plan.oct.ok && plan.oct.general_joint == 0 && !(P.jla || P.lane_general || plan.oct.partial_mf);
		const bool oct_size = !oct_lean || b->B <= 24576;
		const bool eight = choice == KernelChoice::Oct || (choice == KernelChoice::Auto && oct_size);
		plan.kernel = (eight && plan.oct.ok) ? CycleKernel::Oct : ((eight && octjf_ok) ? CycleKernel::OctJf : CycleKernel::Lane);
		// slow path: instances the lane / eight-lane kernel flags (outside the fully non-singular branch) are recomputed by the general kernel
		// when a task can handle them there (blended strategies -- the reference default -- or singularity handling disabled: the task is
		// reduced to its non-singular subspace).  Flagged instances are appended to a list on the device; the general kernel launched
		// behind strides over it with a small fixed grid, no host round trip, and leaves at once when the list is empty.
		bool handled = false;
		for (auto& T : b->tasks)
			if (T.dev.type == saip::TASK_MOTION_FORCE && (!T.dev.sing_handling || T.dev.sing_strategies)) handled = true;
		const bool headline = plan.kernel == CycleKernel::Oct && plan.oct.general_joint == 0;
		if (!handled) plan.recompute = Recompute::None;
		// the eight-lane kernel runs the blended singularity strategies of the headline stack itself (and passes a fully singular task
		// through): with the handling enforced nothing is left for a slow path, and what it still refuses the general kernel would too
		else if (headline && b->tasks[0].dev.sing_handling) plan.recompute = Recompute::None;
		// every other eight-lane stack: the wavefront that flags an instance recomputes it itself behind its epilogue (the general kernel's body on
		// its own LDS block) -- no list and no second launch behind the kernel (round 4)
		else if (plan.kernel != CycleKernel::Lane && !headline && !b->flagged_on_list) plan.recompute = Recompute::Tail;
		else plan.recompute = Recompute::List;
		plan.fuse_sim = wants_sim && headline && plan.recompute == Recompute::None;  // nothing recomputes torques behind this launch: it can integrate as well
		return plan;
	}
	if (choice == KernelChoice::Lane) return refuse(kLaneRefusal);
	const bool wave = wave_eligible(b);
	if (choice == KernelChoice::Wave && !wave) return refuse(kWaveRefusal);
	if (wave) {  // (the choice is Auto or Wave here)
		// chains of 9..32 dof: one wavefront per instance, matrices in MFMA operand form (saip_kernel_wave.hip).  What it cannot certify
		// (a task outside the non-singular branch, an ambiguous rank gap, ...) it leaves untouched on the device-side work list; the
		// general kernel behind recomputes those instances -- an empty list costs that launch one scalar load per workgroup
		plan.kernel = CycleKernel::Wave;
		plan.recompute = Recompute::List;
	}
	return plan;
}

// sim: the integration a rollout would like this launch to do as well; *integrated tells whether it did
saip_status saip::eng::launch_cycle(saip_batch* b, bool diag, const SimRequest* sim, bool* integrated) {
	CycleParams P;
	if (!diag)
		for (auto& T : b->tasks) T.sh_cycle++;  // updateControllerTaskModels: every task's model is updated once per cycle
	saip_status st = make_params(b, P, diag);
	if (st) return st;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		TaskHost& T = b->tasks[t];
		if (T.otg_enabled && !T.otg_inited && (st = run_otg(b, (int)t, 1))) return st;
	}
	// { MotionForceTask, JointTask } with both OTGs on: one launch for the two cycle-mode kernels
	bool paired = false;
	if (!diag && otg_pair_ready(b)) {
		if (b->otg_prelaunched) {  // a rollout ran this step together with the previous period's integration
			b->otg_prelaunched = false;
		} else {
			hipError_t e = saip::launch_otg_pair(b->tasks[0].otg, b->tasks[1].otg, b->B, b->ld, b->stream);
			if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "OTG kernel launch failed: %s", hipGetErrorString(e));
		}
		paired = true;
	}
	for (size_t t = 0; t < b->tasks.size() && !paired; t++) {
		TaskHost& T = b->tasks[t];
		if (!T.otg_enabled) continue;
		if (!diag && (st = run_otg(b, (int)t, 0))) return st;  // a diagnostic re-launch must not advance the trajectory
	}
	const CyclePlan plan = plan_cycle(b, P, diag, sim != nullptr);
	if (plan.refused) return fail(plan.refused, "%s", plan.why);
	P.oct_general_joint = plan.oct.general_joint;
	P.oct_partial_mf = plan.oct.partial_mf;
	P.oct_truncate = plan.oct.truncate;
	P.slow_tail = plan.recompute == Recompute::Tail ? 1 : 0;
	if (plan.fuse_sim) {
		P.sim_substeps = sim->substeps;
		P.sim_dt = sim->dt;
		P.sim_damping = sim->damping;
		for (int i = 0; i < 3; i++) P.sim_gravity[i] = sim->gravity[i];
	}
	bool list = plan.recompute == Recompute::List;
	if (list) {
		b->flags.bind(P, b->ld);
		HIP_TRY(b->flags.zero_current(P, b->stream));
	}
	CycleKernel kernel = plan.kernel;
	hipError_t e;
	bool took = true;
	switch (kernel) {
		case CycleKernel::Oct: e = saip::launch_cycle_oct(P, b->stream); break;
		case CycleKernel::OctJf: e = saip::launch_cycle_octjf(P, b->stream); break;
		case CycleKernel::Lane: e = saip::launch_cycle_lane(P, b->stream, &took); break;
		case CycleKernel::Wave: e = saip::launch_cycle_wave(P, b->stream); break;
		default: e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	}
	if (!took) {  // the lane kernel has no instantiation for this stack (there is none such at 6..8 dof): as if the stack were not eligible
		if (b->kernel_choice == KernelChoice::Lane) return fail(SAIP_ERR_UNSUPPORTED, "%s", kLaneRefusal);
		if (b->kernel_choice == KernelChoice::Wave) return fail(SAIP_ERR_UNSUPPORTED, "%s", kWaveRefusal);
		kernel = CycleKernel::Wg;
		list = false;
		e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	}
	if (e != hipSuccess) {
		const char* what = kernel == CycleKernel::Wg ? "kernel" : (kernel == CycleKernel::Wave ? "wavefront-per-instance kernel" : "lane kernel");
		return fail(SAIP_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
	}
	if (list) b->flags.handed_over();
	switch (kernel) {
		case CycleKernel::Oct: b->kernel_name = "saip_cycle_oct"; break;
		case CycleKernel::OctJf: b->kernel_name = "saip_cycle_octjf"; break;
		case CycleKernel::Lane: b->kernel_name = "saip_cycle_lane"; break;
		case CycleKernel::Wave: b->kernel_name = "saip_cycle_wave"; break;
		default:
			if (b->model->dev.is_tree) b->kernel_name = P.n <= 8 ? "saip_cycle_wg_tree<8,64>" : "saip_cycle_wg_tree<32,512>";
			else b->kernel_name = P.n <= 8 ? "saip_cycle_wg<8,64>" : "saip_cycle_wg<32,512>";
	}
	if (list) {
		hipError_t e2 = saip::launch_cycle_wg_list(P, b->stream);
		if (e2 != hipSuccess) return fail(SAIP_ERR_DEVICE, "slow-path kernel launch failed: %s", hipGetErrorString(e2));
	}
	if (integrated) *integrated = plan.fuse_sim;
	return SAIP_OK;
}

static saip_status launch_reinit_masked(saip_batch* b, int task, int mask) {
	std::vector<bool> otg;
	for (auto& T : b->tasks) otg.push_back(T.otg_enabled), T.otg_enabled = false;  // reinit does not depend on the OTG flag
	CycleParams P;
	saip_status st = make_params(b, P, false);
	bool any_otg = false;
	for (size_t i = 0; i < b->tasks.size(); i++) {
		b->tasks[i].otg_enabled = otg[i];
		any_otg = any_otg || otg[i];
	}
	if (any_otg) b->config_dirty = true;  // the upload above pointed the tasks at the raw goal rows: the next cycle must re-point them at the OTG output
	if (st) return st;
	P.reinit_task = task;
	P.reinit_mask = mask;
	hipError_t e = saip::launch_reinit(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "reinit launch failed: %s", hipGetErrorString(e));
	for (size_t t = 0; t < b->tasks.size(); t++) {  // JointTask::reInitializeTask -> _otg->reInitialize (JointTask.cpp:106)
		TaskHost& T = b->tasks[t];
		if ((task >= 0 && (int)t != task) || !T.otg_enabled) continue;
		const int m3 = T.dev.type == saip::TASK_JOINT ? ((mask & 1) ? 3 : 0) : (mask & 3);  // linear / angular parts (reInitializeLinear / Angular)
		if (m3 == 0) continue;
		if ((st = ensure_otg(b, T))) return st;
		if (m3 != 3 && !T.otg_inited && (st = run_otg(b, (int)t, 1, 3))) return st;
		if ((st = run_otg(b, (int)t, 1, m3))) return st;
	}
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_reinitialize_tasks(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_reinitialize_tasks");
	if (st) return st;
	return launch_reinit_masked(b, -1, 7);
}
// parametrizeForceMotionSpaces / parametrizeMomentRotMotionSpaces: a setter like those above, here because a change re-initialises the task
static saip_status parametrize_space(saip_batch* b, int t, int dim, const double* axis, int* changed, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	if (dim < 0 || dim > 3)  // MotionForceTask.cpp:831-835, 864-868
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s space dimension should be between 0 and 3 in %s", moment ? "Moment" : "Force", who);
	TaskDev& d = b->tasks[t].dev;
	int& cur_dim = moment ? d.moment_dim : d.force_dim;
	double* cur_axis = moment ? d.moment_axis : d.force_axis;
	bool reset = dim != cur_dim;
	if (dim == 1 || dim == 2) {
		if (!axis) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null axis", who);
		double nrm = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
		if (nrm < 1e-2)  // :838-842, 871-875
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s axis should be a non singular vector in %s", moment ? "Moment or rot motion" : "Force or motion", who);
		double a[3] = {axis[0] / nrm, axis[1] / nrm, axis[2] / nrm};
		double diff = fabs(a[0] - cur_axis[0]) + fabs(a[1] - cur_axis[1]) + fabs(a[2] - cur_axis[2]);
		reset = reset || diff > 1e-12;
		memcpy(cur_axis, a, sizeof(a));
	}
	cur_dim = dim;
	refresh_has_ki(d);
	b->config_dirty = true;
	if (changed) *changed = reset ? 1 : 0;
	if (reset && b->finalized && b->device >= 0 && b->state_pushed)  // goal := current, integrators := 0 (:846-852, 880-886)
		return launch_reinit_masked(b, t, moment ? 2 : 1);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_parametrize_force_motion_spaces(saip_batch* b, int t, int dim, const double* axis, int* changed) {
	return parametrize_space(b, t, dim, axis, changed, false, "MotionForceTask::parametrizeForceMotionSpaces");
}
extern "C" saip_status saip_batch_parametrize_moment_rot_motion_spaces(saip_batch* b, int t, int dim, const double* axis, int* changed) {
	return parametrize_space(b, t, dim, axis, changed, true, "MotionForceTask::parametrizeMomentRotMotionSpaces");
}

// MotionForceTask::getCurrentPosition / getCurrentOrientation (MotionForceTask.h:121-138) for the state last pushed: pos [3][B], rot [9][B]
extern "C" saip_status saip_batch_get_current_pose_host(saip_batch* b, int task, double* pos, double* rot) {
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, "saip_batch_get_current_pose_host");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_get_current_pose_host"))) return st;
	if (!b->pose_dev && (st = dev_alloc(b, &b->pose_dev, (size_t)12 * b->ld))) return st;
	CycleParams P;
	if ((st = make_params(b, P, false))) return st;
	hipError_t e = saip::launch_pose(P, task, b->pose_dev, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "pose kernel launch failed: %s", hipGetErrorString(e));
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (pos && (st = copy_d2h(b, pos, b->pose_dev, 3))) return st;
	if (rot && (st = copy_d2h(b, rot, b->pose_dev + 3 * (size_t)b->ld, 9))) return st;
	return SAIP_OK;
}
// task diagnostics of one motion-force task (saip_task_diag.hip) for the state last pushed, into out_dev [24][ld] on the batch stream
static saip_status launch_task_diagnostics(saip_batch* b, int task, double* out_dev, const char* fn) {
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (!out_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	CycleParams P;
	if ((st = make_params(b, P, false))) return st;
	TaskHost& T = b->tasks[task];
	const bool otg = T.otg_enabled && T.otg_alloc && T.otg_inited;  // as saip_batch_get_desired_host
	hipError_t e = saip::launch_task_diag(P, task, T.goal_dev, otg ? T.desired_dev : T.goal_dev, T.dev.goal_comps, out_dev, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "task diagnostics kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_task_diagnostics_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_get_task_diagnostics_host";
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if (!b->task_diag_dev && (st = dev_alloc(b, &b->task_diag_dev, (size_t)24 * b->ld))) return st;
	if ((st = launch_task_diagnostics(b, task, b->task_diag_dev, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, out, b->task_diag_dev, 24);
}
extern "C" saip_status saip_batch_task_diagnostics_device(saip_batch* b, int task, double* out_dev) {
	return launch_task_diagnostics(b, task, out_dev, "saip_batch_task_diagnostics_device");
}
extern "C" saip_status saip_batch_reinitialize_task(saip_batch* b, int task) {
	saip_status st = need_ready(b, "saip_batch_reinitialize_task");
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_reinitialize_task: bad task");
	return launch_reinit_masked(b, task, 7);
}
// MotionForceTask::resetIntegrators / Linear / Angular (MotionForceTask.cpp:988-1002), JointTask::resetIntegrators: parts bit 0 = linear
// (or the joint task's), bit 1 = angular
extern "C" saip_status saip_batch_reset_integrators(saip_batch* b, int task, int parts) {
	saip_status st = need_ready(b, "saip_batch_reset_integrators");
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_reset_integrators: bad task");
	TaskHost& T = b->tasks[task];
	if (!T.integ_dev) return SAIP_OK;
	const size_t row = (size_t)b->ld * sizeof(double);
	if (T.dev.type == saip::TASK_JOINT) {
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev, 0, row * T.dev.m, b->stream));
	} else {
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev, 0, row * 3, b->stream));                      // position, then force (rows 6..8)
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev + 6 * (size_t)b->ld, 0, row * 3, b->stream));
		if (parts & 2) HIP_TRY(hipMemsetAsync(T.integ_dev + 3 * (size_t)b->ld, 0, row * 3, b->stream));  // orientation, then moment (rows 9..11)
		if (parts & 2) HIP_TRY(hipMemsetAsync(T.integ_dev + 9 * (size_t)b->ld, 0, row * 3, b->stream));
	}
	return SAIP_OK;
}

extern "C" saip_status saip_batch_update_task_models(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_update_task_models");
	if (st) return st;
	// The task models are a pure function of the state set by saip_batch_set_state_host; the fused cycle kernel
	// evaluates them together with the control law when computeControlTorques is called (goals may still change).
	b->models_valid = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_step_async(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_step_async");
	if (st) return st;
	return launch_cycle(b, false);
}
extern "C" saip_status saip_batch_synchronize(saip_batch* b) {
	saip_status st = need_state(b, "saip_batch_synchronize");
	if (st) return st;
	// A blocking wait.  Polling hipStreamQuery returns ~1 us after the last kernel instead of 4 - 5, but a caller that follows up with ANOTHER
	// runtime wait (hipDeviceSynchronize, torch.cuda.synchronize) then pays for that one's own marker round trip (~19 us instead of ~4 after a
	// blocking wait) -- measured with bench.py at 20 steps: 10.2 us per step polling, 9.7 blocking.
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_torques_host(saip_batch* b, double* tau_host, uint8_t* status_host) {
	saip_status st = need_ready(b, "saip_batch_get_torques_host");
	if (st) return st;
	if (tau_host && (st = copy_d2h(b, tau_host, commanded_tau(b), b->model->n))) return st;
	if (status_host) {
		HIP_TRY(hipMemcpyAsync(status_host, b->status, b->B, hipMemcpyDeviceToHost, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_compute_control_torques(saip_batch* b, double* tau_host, uint8_t* status_host) {
	saip_status st = need_ready(b, "saip_batch_compute_control_torques");
	if (st) return st;
	if (!b->models_valid)
		return fail(SAIP_ERR_ORDER, "computeControlTorques: the robot state changed since the last updateControllerTaskModels (stale task models are not supported)");
	if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return saip_batch_get_torques_host(b, tau_host, status_host);
}
extern "C" saip_status saip_batch_get_task_nullspace_host(saip_batch* b, int t, double* N) {
	saip_status st = need_ready(b, "saip_batch_get_task_nullspace_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !N) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null output");
	const int n = b->model->n;
	TaskHost& T = b->tasks[t];
	if (!T.diag_dev && (st = dev_alloc(b, &T.diag_dev, (size_t)n * n * b->ld))) return st;
	// the diagnostic pass re-evaluates the models only (make_params: phase 1, scratch outputs): no state of the batch is advanced
	st = launch_cycle(b, true);
	b->config_dirty = true;
	if (st) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, N, T.diag_dev, n * n);
}
// ------------------------------------------------------------------ per-task entry points, TemplateTask.h:43-60
// The reference's plug-in interface: a caller that builds its own hierarchy drives each task by hand
// (examples/04-task_and_redundancy/04-task_and_redundancy.cpp:141-206): updateTaskModel(N_prec), N_prec = getTaskAndPreviousNullspace(),
// computeTorques() / computeTorques(tau_prec).  One launch of the general kernel per call, restricted to the task.
static saip_status ensure_task_buffers(saip_batch* b, TaskHost& T) {
	if (T.tstatus_dev) return SAIP_OK;
	const size_t n = b->model->n, ld = b->ld;
	saip_status st;
	if ((st = dev_alloc(b, &T.nprec_dev, n * n * ld)) || (st = dev_alloc(b, &T.ntask_dev, n * n * ld)) || (st = dev_alloc(b, &T.ntot_dev, n * n * ld)) ||
		(st = dev_alloc(b, &T.ttau_dev, n * ld)) || (st = dev_alloc(b, &T.tprec_dev, n * ld)) || (st = dev_alloc(b, &T.tstatus_dev, ld)))
		return st;
	return SAIP_OK;
}
static saip_status launch_task(saip_batch* b, int t, int phase, const double* tau_prec_dev, double* tau_out_dev) {
	CycleParams P;
	saip_status st = make_params(b, P, false);
	if (st) return st;
	TaskHost& T = b->tasks[t];
	if (phase == 1) P.task_cycle[t] = ++T.sh_cycle;
	if (phase == 2 && T.otg_enabled) {
		// computeTorques steps the task's internal OTG (JointTask.cpp:313-319, MotionForceTask.cpp:394-406); updateTaskModel does not
		if (!T.otg_inited && (st = run_otg(b, t, 1))) return st;
		if ((st = run_otg(b, t, 0))) return st;
	}
	P.single_task = t;
	P.phase = phase;
	P.rank_bound[t] = T.dev.type == saip::TASK_JOINT ? T.dev.m : T.dev.k;  // N_prec is the caller's: nothing is known about the ranks above
	P.ext_nprec = T.nprec_identity ? nullptr : T.nprec_dev;
	P.ext_tau_prec = phase == 2 ? tau_prec_dev : nullptr;
	P.out_N = phase == 1 ? T.ntask_dev : nullptr;
	P.out_Ntot = phase == 1 ? T.ntot_dev : nullptr;
	P.tau = tau_out_dev ? tau_out_dev : T.ttau_dev;
	P.status = T.tstatus_dev;
	hipError_t e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "per-task kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
static saip_status task_ready(saip_batch* b, int t, const char* fn) {
	saip_status st = need_ready(b, fn);
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, t);
	if (!b->state_pushed) return fail(SAIP_ERR_ORDER, "%s: no robot state has been set (saip_batch_set_state_host)", fn);
	return ensure_task_buffers(b, b->tasks[t]);
}
static saip_status task_update_model(saip_batch* b, int t) {
	saip_status st = launch_task(b, t, 1, nullptr, nullptr);
	if (st) return st;
	b->tasks[t].model_epoch = b->state_epoch;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_task_update_model(saip_batch* b, int t, const double* N_prec_host) {
	saip_status st = task_ready(b, t, "saip_batch_task_update_model");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.nprec_identity = N_prec_host == nullptr;
	if (N_prec_host && (st = copy_h2d(b, T.nprec_dev, N_prec_host, b->model->n * b->model->n))) return st;
	return task_update_model(b, t);
}
extern "C" saip_status saip_batch_task_update_model_device(saip_batch* b, int t, const double* N_prec_dev) {
	saip_status st = task_ready(b, t, "saip_batch_task_update_model_device");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.nprec_identity = N_prec_dev == nullptr;
	if (N_prec_dev && N_prec_dev != T.nprec_dev)  // the task keeps its own copy like the reference (_N_prec = N_prec)
		HIP_TRY(hipMemcpyAsync(T.nprec_dev, N_prec_dev, (size_t)b->model->n * b->model->n * b->ld * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
	return task_update_model(b, t);
}
static saip_status task_model_fresh(saip_batch* b, int t, const char* fn) {
	if (b->tasks[t].model_epoch != b->state_epoch)
		return fail(SAIP_ERR_ORDER, "%s: task [%s] has no model for the current robot state: call updateTaskModel(N_prec) first (stale task models are not supported)",
					fn, b->tasks[t].name.c_str());
	return SAIP_OK;
}
extern "C" saip_status saip_batch_task_compute_torques_device(saip_batch* b, int t, const double* tau_prec_dev, double* tau_dev) {
	saip_status st = task_ready(b, t, "saip_batch_task_compute_torques_device");
	if (st || (st = task_model_fresh(b, t, "computeTorques"))) return st;
	return launch_task(b, t, 2, tau_prec_dev, tau_dev);
}
extern "C" saip_status saip_batch_task_compute_torques(saip_batch* b, int t, const double* tau_prec_host, double* tau_host, uint8_t* status_host) {
	saip_status st = task_ready(b, t, "saip_batch_task_compute_torques");
	if (st || (st = task_model_fresh(b, t, "computeTorques"))) return st;
	TaskHost& T = b->tasks[t];
	if (tau_prec_host && (st = copy_h2d(b, T.tprec_dev, tau_prec_host, b->model->n))) return st;
	if ((st = launch_task(b, t, 2, tau_prec_host ? T.tprec_dev : nullptr, nullptr))) return st;
	if (tau_host && (st = copy_d2h(b, tau_host, T.ttau_dev, b->model->n))) return st;
	if (status_host) HIP_TRY(hipMemcpyAsync(status_host, T.tstatus_dev, b->B, hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" const double* saip_batch_task_device_nullspace(saip_batch* b, int t, int which) {
	if (!b || t < 0 || t >= (int)b->tasks.size() || b->tasks[t].model_epoch < 0) return nullptr;
	const TaskHost& T = b->tasks[t];
	return which == 0 ? T.ntask_dev : (which == 1 ? (T.nprec_identity ? nullptr : T.nprec_dev) : (which == 2 ? T.ntot_dev : nullptr));
}
extern "C" double* saip_batch_task_device_torques(saip_batch* b, int t) {
	return (b && t >= 0 && t < (int)b->tasks.size()) ? b->tasks[t].ttau_dev : nullptr;
}
extern "C" saip_status saip_batch_task_get_nullspaces_host(saip_batch* b, int t, double* N, double* N_prec, double* N_total) {
	saip_status st = task_ready(b, t, "saip_batch_task_get_nullspaces_host");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	if (T.model_epoch < 0) return fail(SAIP_ERR_ORDER, "task [%s]: updateTaskModel has not been called", T.name.c_str());
	const int n = b->model->n;
	if (N && (st = copy_d2h(b, N, T.ntask_dev, n * n))) return st;
	if (N_total && (st = copy_d2h(b, N_total, T.ntot_dev, n * n))) return st;
	if (N_prec) {
		if (T.nprec_identity) {
			for (int i = 0; i < n; i++)
				for (int j = 0; j < n; j++)
					for (int k = 0; k < b->B; k++) N_prec[((size_t)i * n + j) * b->B + k] = (i == j) ? 1.0 : 0.0;
		} else if ((st = copy_d2h(b, N_prec, T.nprec_dev, n * n))) {
			return st;
		}
	}
	return SAIP_OK;
}
// resident state shared between batches (tasks driven by hand live in batches of their own): device-to-device copy of q, dq [dof][ld]
extern "C" saip_status saip_batch_set_state_device(saip_batch* b, const double* q_dev, const double* dq_dev) {
	saip_status st = need_state(b, "saip_batch_set_state_device");
	if (st) return st;
	if (!q_dev || !dq_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "null state pointer");
	const size_t bytes = (size_t)b->model->n * b->ld * sizeof(double);
	b->models_valid = false;
	b->state_epoch++;
	if (q_dev != b->q) HIP_TRY(hipMemcpyAsync(b->q, q_dev, bytes, hipMemcpyDeviceToDevice, b->stream));
	if (dq_dev != b->dq) HIP_TRY(hipMemcpyAsync(b->dq, dq_dev, bytes, hipMemcpyDeviceToDevice, b->stream));
	b->state_pushed = true;
	return SAIP_OK;
}
// everything enqueued so far on `producer`'s stream happens before what is enqueued on `waiter`'s stream from now on (device-side
// ordering, no host synchronisation): lets one batch consume device arrays another batch has just written
extern "C" saip_status saip_batch_wait_for(saip_batch* waiter, saip_batch* producer) {
	saip_status st = need_state(waiter, "saip_batch_wait_for");
	if (st || (st = need_state(producer, "saip_batch_wait_for"))) return st;
	if (waiter == producer) return SAIP_OK;
	if (waiter->device != producer->device) return fail(SAIP_ERR_UNSUPPORTED, "saip_batch_wait_for: batches live on different devices");
	if (!producer->sync_event) HIP_TRY(hipEventCreateWithFlags(&producer->sync_event, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(producer->sync_event, producer->stream));
	HIP_TRY(hipStreamWaitEvent(waiter->stream, producer->sync_event, 0));
	return SAIP_OK;
}

extern "C" saip_status saip_batch_set_kernel(saip_batch* b, int which) {
	if (!b || which < 0 || which > 4) return fail(SAIP_ERR_INVALID_ARGUMENT, "kernel selector must be 0, 1, 2, 3 or 4");
	if (which >= 2 && b->model->dev.is_tree)
		return fail(SAIP_ERR_UNSUPPORTED, "saip_batch_set_kernel(%d): this robot is a kinematic tree; only the general kernel (0 or 1) covers trees", which);
	b->kernel_choice = (KernelChoice)which;
	return SAIP_OK;
}
extern "C" const char* saip_batch_kernel_name(saip_batch* b) { return b ? b->kernel_name.c_str() : ""; }

extern "C" saip_status saip_batch_set_torques_host(saip_batch* b, const double* tau) {
	saip_status st = need_ready(b, "saip_batch_set_torques_host");
	if (st) return st;
	if (!tau) return fail(SAIP_ERR_INVALID_ARGUMENT, "null torque pointer");
	return copy_h2d(b, commanded_tau(b), tau, b->model->n);
}
extern "C" saip_status saip_batch_get_state_host(saip_batch* b, double* q, double* dq) {
	saip_status st = need_state(b, "saip_batch_get_state_host");
	if (st) return st;
	if (q && (st = copy_d2h(b, q, b->q, b->model->n))) return st;
	if (dq && (st = copy_d2h(b, dq, b->dq, b->model->n))) return st;
	return SAIP_OK;
}

// desired state of a task = what its control law tracks: the internal OTG's output when enabled, else the goal (JointTask.h:185-200)
extern "C" saip_status saip_batch_get_desired_host(saip_batch* b, int t, double* desired) {
	saip_status st = need_ready(b, "saip_batch_get_desired_host");
	if (st) return st;
	if ((st = check_batch(b, t, "saip_batch_get_desired_host"))) return st;
	if (t < 0 || !desired) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_get_desired_host: bad argument");
	TaskHost& T = b->tasks[t];
	const bool otg = T.otg_enabled && T.otg_alloc && T.otg_inited;
	return copy_d2h(b, desired, otg ? T.desired_dev : T.goal_dev, T.dev.goal_comps);
}
extern "C" saip_status saip_batch_get_otg_status_host(saip_batch* b, int t, int* flags, int* result) {
	saip_status st = check_batch(b, t, "saip_batch_get_otg_status_host");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	if ((st = need_ready(b, "saip_batch_get_otg_status_host"))) return st;
	TaskHost& T = b->tasks[t];
	if (!T.otg_alloc) return fail(SAIP_ERR_ORDER, "saip_batch_get_otg_status_host: the internal OTG of task [%s] has not run", T.name.c_str());
	if (flags) HIP_TRY(hipMemcpyAsync(flags, T.otg.flags, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
	if (result) HIP_TRY(hipMemcpyAsync(result, T.otg.result, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}

extern "C" saip_status saip_batch_time_steps(saip_batch* b, int steps, int warmup, double* elapsed_ms) {
	saip_status st = need_ready(b, "saip_batch_time_steps");
	if (st) return st;
	if (steps <= 0 || warmup < 0 || !elapsed_ms) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad timing arguments");
	for (int i = 0; i < warmup; i++)
		if ((st = launch_cycle(b, false))) return st;
	if (!b->time_ev[0]) {
		HIP_TRY(hipEventCreate(&b->time_ev[0]));
		HIP_TRY(hipEventCreate(&b->time_ev[1]));
	}
	hipEvent_t e0 = b->time_ev[0], e1 = b->time_ev[1];
	HIP_TRY(hipEventRecord(e0, b->stream));
	for (int i = 0; i < steps; i++)
		if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipEventRecord(e1, b->stream));
	// one wait for the stream (not for the event and then, in the caller, for the stream or the device: each is its own ~15 us
	// marker round trip, tools/bench_overhead_probe.py)
	HIP_TRY(hipStreamSynchronize(b->stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	*elapsed_ms = ms;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_time_steps_begin(saip_batch* b, int steps) {
	saip_status st = need_ready(b, "saip_batch_time_steps_begin");
	if (st) return st;
	if (steps <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad timing arguments");
	if (!b->time_ev[0]) {
		HIP_TRY(hipEventCreate(&b->time_ev[0]));
		HIP_TRY(hipEventCreate(&b->time_ev[1]));
	}
	HIP_TRY(hipEventRecord(b->time_ev[0], b->stream));
	for (int i = 0; i < steps; i++)
		if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipEventRecord(b->time_ev[1], b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_time_steps_end(saip_batch* b, double* elapsed_ms) {
	saip_status st = need_ready(b, "saip_batch_time_steps_end");
	if (st) return st;
	if (!elapsed_ms || !b->time_ev[0]) return fail(SAIP_ERR_ORDER, "saip_batch_time_steps_end: call saip_batch_time_steps_begin first");
	HIP_TRY(hipEventSynchronize(b->time_ev[1]));  // (returns at once when the caller has waited for the device, as it should have)
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, b->time_ev[0], b->time_ev[1]));
	*elapsed_ms = ms;
	return SAIP_OK;
}

extern "C" const char* saip_last_error(void) { return g_err.c_str(); }
extern "C" const char* saip_version(void) { return "saip 0.1 (gfx950)"; }
