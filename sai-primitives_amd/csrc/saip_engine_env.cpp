#include "saip_engine_internal.h"

// ---- environment schedules (saip_env_schedule.hip): the obstacle and plane tables of every rollout period from keyframes resident on the
// device.  A schedule is known by its table: (target, task), the task counting for ENV_TARGET_PATCH only.
static const char* env_target_name(int target) {
	return target == saip::ENV_TARGET_OBSTACLES ? "clearance obstacles" : target == saip::ENV_TARGET_PLANES ? "contact planes" : "contact-patch planes";
}
int saip::eng::env_slot(const saip_batch* b, int target, int task) {
	for (int i = 0; i < saip::ENV_MAX_SCHEDULES; i++) {
		const auto& S = b->env[i];
		if (S.attached && S.target == target && (target != saip::ENV_TARGET_PATCH || S.task == task)) return i;
	}
	return -1;
}
static void env_free_slot(saip_batch* b, int slot) {
	auto& S = b->env[slot];
	for (void* p : {(void*)S.key, (void*)S.vel})
		if (p) (void)hipFree(p);
	S = saip_batch::EnvSchedule();
	b->n_env--;
}
void saip::eng::env_release(saip_batch* b, int target, int task) {
	const int slot = env_slot(b, target, task);
	if (slot >= 0) env_free_slot(b, slot);
}
const double* saip::eng::env_plane_velocity(const saip_batch* b, int target, int task) {
	if (b->n_env == 0) return nullptr;
	const int slot = env_slot(b, target, task);
	return slot < 0 ? nullptr : b->env[slot].vel;
}
// The table a schedule on (target, task) would write: its device array, items and layout.  task -1 of ENV_TARGET_PATCH is the first patch;
// *task receives the patch's task.  Not attached: SAIP_ERR_ORDER.
static saip_status env_table(const saip_batch* b, int target, int* task, double** table, int* items, int* per_instance, const char* fn) {
	if (target == saip::ENV_TARGET_OBSTACLES) {
		if (!b->clearance.attached) return fail(SAIP_ERR_ORDER, "%s: no clearance monitor is attached (saip_batch_clearance_attach)", fn);
		*table = b->clearance.obst;
		*items = b->clearance.geom.O;
		*per_instance = b->clearance.per_instance;
		*task = -1;
	} else if (target == saip::ENV_TARGET_PLANES) {
		if (!b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: no contact planes are attached (saip_batch_contact_attach)", fn);
		*table = b->contact.planes;
		*items = b->contact.n_planes;
		*per_instance = b->contact.per_instance;
		*task = -1;
	} else {
		const saip_batch::ContactPatch* C = nullptr;
		for (int i = 0; i < b->n_patch && !C; i++)
			if (*task == -1 || b->patch[i].task == *task) C = &b->patch[i];
		if (!C) return fail(SAIP_ERR_ORDER, "%s: task %d carries no contact patch (saip_batch_contact_patch_attach)", fn, *task);
		*table = C->planes;
		*items = C->n_planes;
		*per_instance = C->per_instance;
		*task = C->task;
	}
	return SAIP_OK;
}
static saip_status env_check_target(int target, const char* fn) {
	if (target != saip::ENV_TARGET_OBSTACLES && target != saip::ENV_TARGET_PLANES && target != saip::ENV_TARGET_PATCH)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown target %d (0 obstacles, 1 contact planes, 2 contact-patch planes)", fn, target);
	return SAIP_OK;
}
// the attached schedule on (target, task); < 0 with the error set
static int env_need(const saip_batch* b, int target, int task, const char* fn, saip_status* st) {
	if ((*st = need_controller(b, fn)) || (*st = env_check_target(target, fn))) return -1;
	if (target == saip::ENV_TARGET_PATCH && task == -1)
		for (int i = 0; i < b->n_patch && task == -1; i++)
			if (env_slot(b, target, b->patch[i].task) >= 0) task = b->patch[i].task;
	const int slot = env_slot(b, target, task);
	if (slot < 0) *st = fail(SAIP_ERR_ORDER, "%s: the %s have no environment schedule (saip_batch_env_schedule_attach)", fn, env_target_name(target));
	return slot;
}
extern "C" saip_status saip_batch_env_schedule_attach(saip_batch* b, int target, int task, int first, int n_items, const double* keyframes, int n_keyframes,
													  int stride, int mode) {
	const char* fn = "saip_batch_env_schedule_attach";
	saip_status st = need_controller(b, fn);
	if (st || (st = env_check_target(target, fn))) return st;
	if (mode != saip::ENV_HOLD && mode != saip::ENV_LINEAR) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown mode %d (0 hold, 1 linear)", fn, mode);
	if (n_keyframes < 1 || stride < 1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_keyframes >= 1 and stride >= 1 required (got %d, %d)", fn, n_keyframes, stride);
	if (!keyframes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null keyframes", fn);
	double* table = nullptr;
	int items = 0, per_instance = 0;
	if ((st = env_table(b, target, &task, &table, &items, &per_instance, fn))) return st;
	if (env_slot(b, target, task) >= 0) return fail(SAIP_ERR_ORDER, "%s: the %s already have an environment schedule (saip_batch_env_schedule_detach first)", fn, env_target_name(target));
	if (b->n_env == saip::ENV_MAX_SCHEDULES) return fail(SAIP_ERR_ORDER, "%s: %d environment schedules are attached already", fn, saip::ENV_MAX_SCHEDULES);
	if (first < 0 || n_items < 1 || n_items > items || first > items - n_items)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: items [%d, %d + %d) outside the %d items of the %s", fn, first, first, n_items, items, env_target_name(target));
	const bool planes = target != saip::ENV_TARGET_OBSTACLES;
	const size_t W = planes ? saip::ENV_PLANE_WORDS : saip::ENV_OBSTACLE_WORDS, cols = per_instance ? (size_t)b->B : 1, ld = per_instance ? (size_t)b->ld : 1;
	// [K][n_items][W][ld] doubles: the byte count must fit a size_t
	const size_t frame = (size_t)n_items * W, frame_bytes = frame * ld * sizeof(double);
	if ((size_t)n_keyframes > SIZE_MAX / frame_bytes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %d keyframes of %d items are too large", fn, n_keyframes, n_items);
	std::vector<double> host(keyframes, keyframes + (size_t)n_keyframes * frame * cols);
	for (size_t i = 0; i < host.size(); i++)
		if (!std::isfinite(host[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: keyframe %zu: a word is not finite", fn, i / (frame * cols));
	if (planes) {
		// the eight plane words of every keyframe under the rules of the plane table, normals normalised by the table's own routine
		std::vector<double> in((size_t)n_items * saip::CONTACT_PLANE_WORDS * cols), out;
		for (int k = 0; k < n_keyframes; k++) {
			for (int it = 0; it < n_items; it++)
				for (size_t w = 0; w < (size_t)saip::CONTACT_PLANE_WORDS; w++)
					memcpy(&in[((size_t)it * saip::CONTACT_PLANE_WORDS + w) * cols], &host[(((size_t)k * n_items + it) * W + w) * cols], cols * sizeof(double));
			if (const char* bad = contact_check_planes(in.data(), n_items, cols, out)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: keyframe %d: %s", fn, k, bad);
			for (int it = 0; it < n_items; it++)
				for (size_t w = 0; w < 3; w++)
					memcpy(&host[(((size_t)k * n_items + it) * W + w) * cols], &out[((size_t)it * saip::CONTACT_PLANE_WORDS + w) * cols], cols * sizeof(double));
		}
	}
	char msg[200];
	if (!saip::env_check_keyframes(host.data(), planes, n_keyframes, n_items, cols, mode, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	int slot = 0;
	while (b->env[slot].attached) slot++;
	auto& S = b->env[slot];
	const size_t rows = (size_t)n_keyframes * frame;
	if ((st = alloc_zero(b, &S.key, rows * ld)) || (planes && (st = alloc_zero(b, &S.vel, (size_t)items * saip::ENV_VELOCITY_WORDS * ld))) ||
		(st = upload_table(b, S.key, host.data(), rows, per_instance, "keyframe", fn))) {
		for (void* p : {(void*)S.key, (void*)S.vel})
			if (p) (void)hipFree(p);
		S = saip_batch::EnvSchedule();
		return st;
	}
	S.attached = true;
	S.target = target;
	S.task = task;
	S.first = first;
	S.n_items = n_items;
	S.K = n_keyframes;
	S.stride = stride;
	S.mode = mode;
	S.per_instance = per_instance;
	b->n_env++;
	b->env_period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_env_schedule_detach(saip_batch* b, int target, int task) {
	const char* fn = "saip_batch_env_schedule_detach";
	saip_status st;
	int slot = -1;
	if (target == -1) {
		if ((st = need_controller(b, fn))) return st;
		if (b->n_env == 0) return SAIP_OK;
	} else if ((slot = env_need(b, target, task, fn, &st)) < 0) {
		return st;
	}
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a scheduled period may still be in flight
	for (int i = 0; i < saip::ENV_MAX_SCHEDULES; i++)
		if (b->env[i].attached && (target == -1 || i == slot)) env_free_slot(b, i);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_env_schedule_rewind(saip_batch* b, long long period) {
	const char* fn = "saip_batch_env_schedule_rewind";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (period < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: period %lld below 0", fn, period);
	b->env_period = period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_env_schedule_info(saip_batch* b, int target, int task, int* first, int* n_items, int* n_keyframes, int* stride, int* mode,
													int* per_instance, long long* period) {
	saip_status st;
	const int slot = env_need(b, target, task, "saip_batch_env_schedule_info", &st);
	if (slot < 0) return st;
	const auto& S = b->env[slot];
	if (first) *first = S.first;
	if (n_items) *n_items = S.n_items;
	if (n_keyframes) *n_keyframes = S.K;
	if (stride) *stride = S.stride;
	if (mode) *mode = S.mode;
	if (per_instance) *per_instance = S.per_instance;
	if (period) *period = b->env_period;
	return SAIP_OK;
}
static const saip_batch::EnvSchedule* env_of(const saip_batch* b, int target, int task) {
	if (!b || b->n_env == 0) return nullptr;
	for (int i = 0; i < saip::ENV_MAX_SCHEDULES; i++) {
		const auto& S = b->env[i];
		if (S.attached && S.target == target && (target != saip::ENV_TARGET_PATCH || task == -1 || S.task == task)) return &S;
	}
	return nullptr;
}
extern "C" double* saip_batch_env_schedule_keyframes_device(saip_batch* b, int target, int task) { return env_of(b, target, task) ? env_of(b, target, task)->key : nullptr; }
extern "C" double* saip_batch_env_schedule_velocity_device(saip_batch* b, int target, int task) { return env_of(b, target, task) ? env_of(b, target, task)->vel : nullptr; }
// the tables of rollout period c = env_period, written at the head of the period: one launch for every schedule; index, fraction and span
// are computed here, at enqueue time (no device-side counter).  T: the length of the period
saip_status saip::eng::env_apply(saip_batch* b, double T) {
	saip::EnvScheduleParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	const long long c = b->env_period++;
	for (int i = 0; i < saip::ENV_MAX_SCHEDULES; i++) {
		const auto& S = b->env[i];
		if (!S.attached) continue;
		auto& E = P.e[P.n++];
		int task = S.task, items = 0, per_instance = 0;
		if (saip_status st = env_table(b, S.target, &task, &E.table, &items, &per_instance, "environment schedule")) return st;
		E.vel = S.vel;
		E.key = S.key;
		E.planes = S.target != saip::ENV_TARGET_OBSTACLES;
		E.per_instance = S.per_instance;
		E.first = S.first;
		E.n_items = S.n_items;
		saip::env_timing(saip::env_period_index(c, E.planes), S.K, S.stride, S.mode, &E.i, &E.s, &E.moving);
		E.span = (double)S.stride * T;
	}
	hipError_t e = saip::launch_env_schedule(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "environment schedule launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
