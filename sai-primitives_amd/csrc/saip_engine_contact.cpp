#include "saip_engine_internal.h"

// ---- contact planes and the simulated force sensor (saip_contact.hip): the resident simulator gets something to touch
static saip_status need_contact(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: no contact planes are attached (saip_batch_contact_attach)", fn);
	return SAIP_OK;
}
void saip::eng::contact_free(saip_batch* b) {
	auto& C = b->contact;
	env_release(b, saip::ENV_TARGET_PLANES, -1);  // an environment schedule writes into the planes: it goes first
	for (void* p : {(void*)C.planes, (void*)C.tau_sim, (void*)C.readout, (void*)C.summary})
		if (p) (void)hipFree(p);
	C = saip_batch::Contact();
}
// the plane table as the device keeps it: [P][8] or [P][8][B] with every normal normalised; nullptr: fine, else what is wrong
const char* saip::eng::contact_check_planes(const double* planes, int P, size_t cols, std::vector<double>& out) {
	out.assign(planes, planes + (size_t)P * saip::CONTACT_PLANE_WORDS * cols);
	for (size_t i = 0; i < out.size(); i++)
		if (!std::isfinite(out[i])) return "a plane value is not finite";
	for (int k = 0; k < P; k++)
		for (size_t i = 0; i < cols; i++) {
			double* w = out.data() + (size_t)k * saip::CONTACT_PLANE_WORDS * cols + i;
			const double nn = std::sqrt(w[0] * w[0] + w[cols] * w[cols] + w[2 * cols] * w[2 * cols]);
			if (!(nn > 0) || !std::isfinite(nn)) return "a plane normal is zero";
			for (int e = 0; e < 3; e++) w[e * cols] /= nn;
			if (!(w[4 * cols] > 0)) return "stiffness k > 0 required";
			if (!(w[5 * cols] >= 0)) return "damping c >= 0 required";
			if (!(w[6 * cols] >= 0)) return "friction mu >= 0 required";
			if (!(w[7 * cols] > 0)) return "slip-regularisation speed v_s > 0 required";
		}
	return nullptr;
}
// what saip_batch_contact_attach and saip_batch_contact_patch_attach ask of their arguments alike: the carrier ...
static saip_status contact_attach_task(const saip_batch* b, int task, const char* fn) {
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (b->tasks[task].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, task);
	return SAIP_OK;
}
// ... and the planes, the array sizes and the sensor against the task's goal schedule; `host` receives the table as the device keeps it
static saip_status contact_attach_planes(const saip_batch* b, int task, int n_planes, const double* planes, int per_instance, int sensor,
										 std::vector<double>& host, const char* fn) {
	if (n_planes < 1 || n_planes > saip::CONTACT_MAX_PLANES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d planes required (got %d)", fn, saip::CONTACT_MAX_PLANES, n_planes);
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	// [n][ld], [P][8][ld] doubles: the byte counts must fit a size_t
	const size_t widest = (size_t)(b->model->n > 32 ? b->model->n : 32) * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if (const char* bad = contact_check_planes(planes, n_planes, per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if (sensor && task < (int)b->sched.size() && b->sched[task].attached && contact_rows_overlap(b->sched[task].first, b->sched[task].count))
		return fail(SAIP_ERR_ORDER, "%s: the goal schedule of task %d covers sensed-wrench rows 30..35, which the simulated sensor writes", fn, task);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_attach(saip_batch* b, int task, const double* r_c, int n_planes, const double* planes, int per_instance,
												 int sensor) {
	const char* fn = "saip_batch_contact_attach";
	saip_status st = need_controller(b, fn);
	if (st || (st = contact_attach_task(b, task, fn))) return st;
	if (b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: contact planes are already attached (saip_batch_contact_detach first)", fn);
	if (b->n_patch > 0) return fail(SAIP_ERR_ORDER, "%s: a contact patch is attached (saip_batch_contact_patch_detach first)", fn);
	per_instance = per_instance ? 1 : 0;
	sensor = sensor ? 1 : 0;
	double rc[3] = {0, 0, 0};
	for (int e = 0; e < 3 && r_c; e++) {
		if (!std::isfinite(r_c[e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the contact point is not finite", fn);
		rc[e] = r_c[e];
	}
	std::vector<double> host;
	if ((st = contact_attach_planes(b, task, n_planes, planes, per_instance, sensor, host, fn)) || (st = need_ready(b, fn))) return st;
	auto& C = b->contact;
	const size_t ld = b->ld, rows = (size_t)n_planes * saip::CONTACT_PLANE_WORDS;
	if ((st = alloc_zero(b, &C.planes, rows * (per_instance ? ld : 1))) || (st = alloc_zero(b, &C.tau_sim, (size_t)b->model->n * ld)) ||
		(st = alloc_zero(b, &C.readout, (size_t)saip::CONTACT_READOUT_ROWS * ld)) || (st = alloc_zero(b, &C.summary, (size_t)saip::CONTACT_SUMMARY_ROWS * ld)) ||
		(st = upload_table(b, C.planes, host.data(), rows, per_instance, "plane", fn))) {
		contact_free(b);
		return st;
	}
	C.attached = true;
	C.task = task;
	C.n_planes = n_planes;
	C.per_instance = per_instance;
	C.sensor = sensor;
	for (int e = 0; e < 3; e++) C.rc[e] = rc[e];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_detach(saip_batch* b) {
	const char* fn = "saip_batch_contact_detach";
	saip_status st = need_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a contact substep may still be in flight
	contact_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_info(saip_batch* b, int* task, int* n_planes, int* per_instance, int* sensor, double* r_c) {
	saip_status st = need_contact(b, "saip_batch_contact_info");
	if (st) return st;
	const auto& C = b->contact;
	if (task) *task = C.task;
	if (n_planes) *n_planes = C.n_planes;
	if (per_instance) *per_instance = C.per_instance;
	if (sensor) *sensor = C.sensor;
	for (int e = 0; e < 3 && r_c; e++) r_c[e] = C.rc[e];
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_set_planes_host(saip_batch* b, const double* planes) {
	const char* fn = "saip_batch_contact_set_planes_host";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	if (env_slot(b, saip::ENV_TARGET_PLANES, -1) >= 0)
		return fail(SAIP_ERR_ORDER, "%s: the planes are written by an environment schedule (saip_batch_env_schedule_detach first)", fn);
	const auto& C = b->contact;
	std::vector<double> host;
	if (const char* bad = contact_check_planes(planes, C.n_planes, C.per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.planes, host.data(), (size_t)C.n_planes * saip::CONTACT_PLANE_WORDS, C.per_instance, "plane", fn);
}
extern "C" double* saip_batch_contact_planes_device(saip_batch* b) { return b ? b->contact.planes : nullptr; }
extern "C" double* saip_batch_contact_torques_device(saip_batch* b) { return b ? b->contact.tau_sim : nullptr; }
extern "C" double* saip_batch_contact_readout_device(saip_batch* b) { return b ? b->contact.readout : nullptr; }
extern "C" double* saip_batch_contact_summary_device(saip_batch* b) { return b ? b->contact.summary : nullptr; }
// one launch of the contact kernel at the resident state; dt: the substep an APPLY launch stands in front of
saip_status saip::eng::contact_launch(saip_batch* b, int mode, double dt) {
	const auto& C = b->contact;
	if (saip_status st = ensure_task_constants(b)) return st;
	saip::ContactMovingParams P;  // (the static launch takes its ContactParams part)
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.task = C.task;
	P.n_planes = C.n_planes;
	P.per_instance = C.per_instance;
	P.dt = dt;
	for (int e = 0; e < 3; e++) P.rc[e] = C.rc[e];
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.planes = C.planes;
	P.goal = b->tasks[C.task].goal_dev;
	P.tau_cmd = tau_buffer(b, sim_plan(b).contact_in);  // (read by APPLY only, which follows the plant and link-contact launches)
	P.tau_sim = tau_buffer(b, saip::TauBuf::Planes);
	P.readout = C.readout;
	P.summary = C.summary;
	// planes with an environment schedule move: the MOVING instantiation reads the velocities the schedule writes
	P.vel = env_plane_velocity(b, saip::ENV_TARGET_PLANES, -1);
	const bool tree = b->model->dev.is_tree != 0;
	hipError_t e = P.vel ? saip::launch_contact_apply_moving(P, tree, b->stream) : saip::launch_contact_apply(P, tree, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "contact launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_sense(saip_batch* b) {
	const char* fn = "saip_batch_contact_sense";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!b->contact.sensor) return fail(SAIP_ERR_ORDER, "%s: the contact planes were attached without the simulated sensor", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = contact_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
	// a sensing model perturbs the wrench just written (SENSE rewrites the rows: a second call does not stack the perturbation)
	return b->sensing.attached ? sensing_launch(b, saip::SENSE_MODE_WRENCH, sensing_sensor_slots(b, true, false)) : SAIP_OK;
}
extern "C" saip_status saip_batch_contact_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_contact_readout_host";
	const saip_status st = need_contact(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->contact.readout, saip::CONTACT_READOUT_ROWS, fn);
}
extern "C" saip_status saip_batch_contact_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_contact_summary_host";
	const saip_status st = need_contact(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->contact.summary, saip::CONTACT_SUMMARY_ROWS, fn);
}
extern "C" saip_status saip_batch_contact_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_contact_summary_reset";
	saip_status st = need_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return zero_rows(b, b->contact.summary, saip::CONTACT_SUMMARY_ROWS);
}

// ---- contact patches (saip_contact_patch.hip): up to eight points per patch, net force and moment, up to two patches on different tasks
// the slot of the patch on `task` (-1: of the first patch); < 0 with the error set
static int patch_slot(const saip_batch* b, int task, const char* fn, saip_status* st) {
	if ((*st = need_controller(b, fn))) return -1;
	if (b->n_patch == 0) {
		*st = fail(SAIP_ERR_ORDER, "%s: no contact patch is attached (saip_batch_contact_patch_attach)", fn);
		return -1;
	}
	if (task == -1) return 0;
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task) return i;
	*st = fail(SAIP_ERR_ORDER, "%s: task %d carries no contact patch", fn, task);
	return -1;
}
void saip::eng::patch_free(saip_batch* b, int slot) {
	auto& C = b->patch[slot];
	env_release(b, saip::ENV_TARGET_PATCH, C.task);  // an environment schedule writes into the planes: it goes first
	for (void* p : {(void*)C.planes, (void*)C.readout, (void*)C.summary})
		if (p) (void)hipFree(p);
	for (int i = slot; i + 1 < b->n_patch; i++) b->patch[i] = b->patch[i + 1];
	b->patch[b->n_patch - 1] = saip_batch::ContactPatch();
	if (--b->n_patch == 0 && b->patch_tau_sim) {
		(void)hipFree(b->patch_tau_sim);
		b->patch_tau_sim = nullptr;
	}
}
extern "C" saip_status saip_batch_contact_patch_attach(saip_batch* b, int task, int n_points, const double* points, int n_planes, const double* planes,
													   int per_instance, int sensor) {
	const char* fn = "saip_batch_contact_patch_attach";
	saip_status st = need_controller(b, fn);
	if (st || (st = contact_attach_task(b, task, fn))) return st;
	if (b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: single-point contact planes are attached (saip_batch_contact_detach first)", fn);
	if (b->n_patch == saip::PATCH_MAX) return fail(SAIP_ERR_ORDER, "%s: %d contact patches are attached already", fn, saip::PATCH_MAX);
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task) return fail(SAIP_ERR_ORDER, "%s: task %d already carries a contact patch (saip_batch_contact_patch_detach first)", fn, task);
	per_instance = per_instance ? 1 : 0;
	sensor = sensor ? 1 : 0;
	if (n_points < 1 || n_points > saip::PATCH_MAX_POINTS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d points required (got %d)", fn, saip::PATCH_MAX_POINTS, n_points);
	if (!points) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null points", fn);
	for (int i = 0; i < 3 * n_points; i++)
		if (!std::isfinite(points[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a contact point is not finite", fn);
	std::vector<double> host;
	if ((st = contact_attach_planes(b, task, n_planes, planes, per_instance, sensor, host, fn)) || (st = need_ready(b, fn))) return st;
	const size_t ld = b->ld, rows = (size_t)n_planes * saip::CONTACT_PLANE_WORDS;
	if (!b->patch_tau_sim && (st = alloc_zero(b, &b->patch_tau_sim, (size_t)b->model->n * ld))) return st;
	const int slot = b->n_patch++;
	auto& C = b->patch[slot];
	if ((st = alloc_zero(b, &C.planes, rows * (per_instance ? ld : 1))) || (st = alloc_zero(b, &C.readout, (size_t)saip::PATCH_READOUT_ROWS * ld)) ||
		(st = alloc_zero(b, &C.summary, (size_t)saip::PATCH_SUMMARY_ROWS * ld)) || (st = upload_table(b, C.planes, host.data(), rows, per_instance, "plane", fn))) {
		patch_free(b, slot);
		return st;
	}
	C.task = task;
	C.n_points = n_points;
	C.n_planes = n_planes;
	C.per_instance = per_instance;
	C.sensor = sensor;
	for (int i = 0; i < 3 * n_points; i++) C.r[i / 3][i % 3] = points[i];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_contact_patch_detach";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0 || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a contact substep may still be in flight
	if (task == -1)
		while (b->n_patch > 0) patch_free(b, b->n_patch - 1);
	else patch_free(b, slot);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_info(saip_batch* b, int task, int* n_patches, int* n_points, int* n_planes, int* per_instance, int* sensor,
													 double* points) {
	saip_status st;
	const int slot = patch_slot(b, task, "saip_batch_contact_patch_info", &st);
	if (slot < 0) return st;
	const auto& C = b->patch[slot];
	if (n_patches) *n_patches = b->n_patch;
	if (n_points) *n_points = C.n_points;
	if (n_planes) *n_planes = C.n_planes;
	if (per_instance) *per_instance = C.per_instance;
	if (sensor) *sensor = C.sensor;
	for (int i = 0; i < 3 * C.n_points && points; i++) points[i] = C.r[i / 3][i % 3];
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_set_planes_host(saip_batch* b, int task, const double* planes) {
	const char* fn = "saip_batch_contact_patch_set_planes_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0) return st;
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	const auto& C = b->patch[slot];
	if (env_slot(b, saip::ENV_TARGET_PATCH, C.task) >= 0)
		return fail(SAIP_ERR_ORDER, "%s: the planes of task %d are written by an environment schedule (saip_batch_env_schedule_detach first)", fn, C.task);
	std::vector<double> host;
	if (const char* bad = contact_check_planes(planes, C.n_planes, C.per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.planes, host.data(), (size_t)C.n_planes * saip::CONTACT_PLANE_WORDS, C.per_instance, "plane", fn);
}
static const saip_batch::ContactPatch* patch_of(const saip_batch* b, int task) {
	if (!b) return nullptr;
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task || task == -1) return &b->patch[i];
	return nullptr;
}
extern "C" double* saip_batch_contact_patch_planes_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->planes : nullptr; }
extern "C" double* saip_batch_contact_patch_readout_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->readout : nullptr; }
extern "C" double* saip_batch_contact_patch_summary_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->summary : nullptr; }
extern "C" double* saip_batch_contact_patch_torques_device(saip_batch* b) { return b ? b->patch_tau_sim : nullptr; }
// one launch of the patch kernel at the resident state, for every patch; dt: the substep an APPLY launch stands in front of
saip_status saip::eng::patch_launch(saip_batch* b, int mode, double dt) {
	if (saip_status st = ensure_task_constants(b)) return st;
	saip::ContactPatchMovingParams P;  // (the static launch takes its ContactPatchParams part)
	bool moving = false;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.n_patches = b->n_patch;
	P.dt = dt;
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau_cmd = tau_buffer(b, sim_plan(b).contact_in);  // (read by APPLY only, which follows the plant and link-contact launches)
	P.tau_sim = tau_buffer(b, saip::TauBuf::Patches);
	for (int i = 0; i < b->n_patch; i++) {
		const auto& C = b->patch[i];
		saip::PatchDev& D = P.patch[i];
		D.task = C.task;
		D.n_points = C.n_points;
		D.n_planes = C.n_planes;
		D.per_instance = C.per_instance;
		D.sensor = C.sensor;
		memcpy(D.r, C.r, sizeof(D.r));
		D.planes = C.planes;
		D.goal = b->tasks[C.task].goal_dev;
		D.readout = C.readout;
		D.summary = C.summary;
		P.vel[i] = env_plane_velocity(b, saip::ENV_TARGET_PATCH, C.task);
		moving = moving || P.vel[i];
	}
	const bool tree = b->model->dev.is_tree != 0;
	hipError_t e = moving ? saip::launch_contact_patch_apply_moving(P, tree, b->stream) : saip::launch_contact_patch_apply(P, tree, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "contact patch launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
bool saip::eng::patch_any_sensor(const saip_batch* b) {
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].sensor) return true;
	return false;
}
extern "C" saip_status saip_batch_contact_patch_sense(saip_batch* b) {
	const char* fn = "saip_batch_contact_patch_sense";
	saip_status st;
	if (patch_slot(b, -1, fn, &st) < 0) return st;
	if (!patch_any_sensor(b)) return fail(SAIP_ERR_ORDER, "%s: no contact patch was attached with the simulated sensor", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = patch_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
	return b->sensing.attached ? sensing_launch(b, saip::SENSE_MODE_WRENCH, sensing_sensor_slots(b, false, true)) : SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_readout_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_contact_patch_readout_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);  // (st is set exactly when slot < 0)
	return rows_to_host(b, st, out, slot < 0 ? nullptr : b->patch[slot].readout, saip::PATCH_READOUT_ROWS, fn);
}
extern "C" saip_status saip_batch_contact_patch_summary_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_contact_patch_summary_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	return rows_to_host(b, st, out, slot < 0 ? nullptr : b->patch[slot].summary, saip::PATCH_SUMMARY_ROWS, fn);
}
extern "C" saip_status saip_batch_contact_patch_summary_reset(saip_batch* b, int task) {
	const char* fn = "saip_batch_contact_patch_summary_reset";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0 || (st = need_ready(b, fn))) return st;
	for (int i = 0; i < b->n_patch; i++)
		if ((task == -1 || i == slot) && (st = zero_rows(b, b->patch[i].summary, saip::PATCH_SUMMARY_ROWS))) return st;
	return SAIP_OK;
}
