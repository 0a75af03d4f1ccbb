#include "saip_engine_internal.h"

// ---- the period plan (saip_period_plan.h): the facts of a batch, and the buffer behind each name of the torque chain
saip::SimPlan saip::eng::sim_plan(const saip_batch* b) {
	saip::SimFacts F;
	F.planes = b->contact.attached;
	F.patches = b->n_patch > 0;
	F.plant = b->plant.attached;
	F.link_contact = b->link_contact.attached;
	F.inertia = b->inertia.attached;
	F.sensing = b->sensing.attached;
	F.goals_written = b->n_sched > 0 || b->guard.attached;
	for (const auto& T : b->tasks) F.any_otg = F.any_otg || T.otg_enabled;
	F.tree = b->model->dev.is_tree != 0;
	F.n = b->model->n;
	return saip::plan_sim(F);
}
double* saip::eng::tau_buffer(const saip_batch* b, saip::TauBuf which) {
	switch (which) {
		case saip::TauBuf::Plant: return b->plant.tau_act;
		case saip::TauBuf::LinkContact: return b->link_contact.tau_sim;
		case saip::TauBuf::Planes: return b->contact.tau_sim;
		case saip::TauBuf::Patches: return b->patch_tau_sim;
		default: return commanded_tau(b);
	}
}
// the state moved: like after robot->setQ(), updateControllerTaskModels() is due; the integration closed one period of the plant's wrench
// windows and of the sensing model's noise counter
static void state_moved(saip_batch* b) {
	if (b->plant.attached) b->plant.period++;
	if (b->sensing.attached) b->sensing.period++;
	b->models_valid = false;
	b->state_epoch++;
}

// ---- the step after the path: forward dynamics + semi-implicit Euler on the resident state (saip_dynamics.hip)
// fuse_next_otg: the caller's half of SimPlan::may_fuse_next_otg (another period follows); otg_pair_ready has the last word
static saip_status enqueue_integrate(saip_batch* b, const saip::SimPlan& plan, double dt, int substeps, const double* gravity, double damping, bool fuse_next_otg = false) {
	SimParams S;
	S.B = b->B;
	S.ld = b->ld;
	S.n = b->model->n;
	S.substeps = substeps;
	S.dt = dt;
	S.damping = damping;
	for (int i = 0; i < 3; i++) S.gravity[i] = gravity ? gravity[i] : b->model->dev.gravity[i];
	S.model = b->model_dev;
	S.q = b->q;
	S.dq = b->dq;
	S.tau = tau_buffer(b, plan.integrator_in);
	S.ddq = nullptr;
	// the inertia table of the simulated robot, on every path below but the fused one (which is not taken while it is attached)
	S.inertia = b->inertia.attached ? b->inertia.rows : nullptr;
	S.inertia_stride = b->inertia.attached && b->inertia.per_instance ? b->ld : 1;
	hipError_t e = hipSuccess;
	const bool tree = b->model->dev.is_tree != 0;  // trees: the lane-per-instance tree kernel, whatever the dof (the eight-lane step is chain-only)
	if (plan.per_substep) {
		// every substep: the attached stages in the order of the torque chain, each at the state of that substep, then one step of the
		// integrator on the last buffer written.  The whole call belongs to one period of the plant.
		S.substeps = 1;
		for (int s = 0; s < substeps && e == hipSuccess; s++) {
			saip_status st = b->plant.attached ? plant_launch(b, dt, s) : SAIP_OK;  // s == 0: the actuation chain advances its delay line
			if (st) return st;
			if (b->link_contact.attached && (st = link_contact_launch(b, saip::LINK_CONTACT_APPLY, dt, S.gravity))) return st;
			if (b->n_patch > 0) st = patch_launch(b, saip::CONTACT_APPLY, dt);
			else if (b->contact.attached) st = contact_launch(b, saip::CONTACT_APPLY, dt);
			if (st) return st;
			e = saip::launch_integrate(S, tree, b->stream);
		}
	} else if (fuse_next_otg && otg_pair_ready(b)) {
		// rollouts: this integration and the NEXT period's trajectory generation in one launch (they are independent)
		e = saip::launch_integrate_otg_pair(S, b->tasks[0].otg, b->tasks[1].otg, b->B, b->ld, b->stream);
		b->otg_prelaunched = true;
	} else {
		e = saip::launch_integrate(S, tree, b->stream);
	}
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "integrate launch failed: %s", hipGetErrorString(e));
	state_moved(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_integrate(saip_batch* b, double dt, int substeps, const double* gravity, double damping) {
	saip_status st = need_ready(b, "saip_batch_integrate");
	if (st) return st;
	if (!(dt > 0) || substeps < 1 || damping < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_integrate: dt > 0, substeps >= 1, damping >= 0 required");
	return enqueue_integrate(b, sim_plan(b), dt, substeps, gravity, damping);
}
// ---- rollout recorder (saip_rollout_record.hip): per-period trajectory log and running summaries of saip_batch_rollout_async
static int record_rows(unsigned channels, int n) {
	return ((channels & saip::REC_Q) ? n : 0) + ((channels & saip::REC_DQ) ? n : 0) + ((channels & saip::REC_TAU) ? n : 0) +
		   ((channels & saip::REC_POSE) ? 12 : 0) + ((channels & saip::REC_ERROR) ? 6 : 0);
}
void saip::eng::record_free(saip_batch* b) {
	auto& R = b->rec;
	for (void* p : {(void*)R.log, (void*)R.status_log, (void*)R.summary})
		if (p) (void)hipFree(p);
	R = saip_batch::Recorder();
}
// the observation of the period that has just been integrated: the sample slot is computed here, at enqueue time (no device-side counter)
static saip_status record_period(saip_batch* b, double T) {
	auto& R = b->rec;
	const long long p = ++R.period;
	const bool sample = R.channels && p % R.stride == 0;
	if (!sample && !R.summary) return SAIP_OK;
	saip::RecordParams P;
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.slot = sample ? (int)((p / R.stride - 1) % R.capacity) : -1;
	P.channels = R.channels;
	P.rows = R.rows;
	P.task = R.task;
	P.pad_ = 0;
	P.T = T;
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau = commanded_tau(b);
	P.status = b->status;
	P.goal = R.task >= 0 ? b->tasks[R.task].goal_dev : nullptr;
	P.log = R.log;
	P.status_log = R.status_log;
	P.summary = R.summary;
	hipError_t e = saip::launch_rollout_record(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "rollout recorder launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
static saip_status need_recorder(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->rec.attached) return fail(SAIP_ERR_ORDER, "%s: no rollout recorder is attached (saip_batch_rollout_recorder_attach)", fn);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_attach(saip_batch* b, int capacity, int stride, unsigned channels, int task, int summaries) {
	const char* fn = "saip_batch_rollout_recorder_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->rec.attached) return fail(SAIP_ERR_ORDER, "%s: a recorder is already attached (saip_batch_rollout_recorder_detach first)", fn);
	if (capacity < 1 || stride < 1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: capacity >= 1 and stride >= 1 required", fn);
	if (channels & ~(unsigned)saip::REC_ALL) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown channel bits 0x%x", fn, channels & ~(unsigned)saip::REC_ALL);
	if (!channels && !summaries) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to record (empty channel mask and no summaries)", fn);
	if (task < -1 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task >= 0 && b->tasks[task].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, task);
	if ((channels & (saip::REC_POSE | saip::REC_ERROR)) && task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the pose and error channels need a motion-force task", fn);
	const int rows = record_rows(channels, b->model->n);
	// [capacity][rows][ld] doubles: the byte count must fit a size_t
	const size_t slot_bytes = (size_t)(rows > 0 ? rows : 1) * b->ld * sizeof(double);
	if ((size_t)capacity > SIZE_MAX / slot_bytes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a log of %d samples of %d rows is too large", fn, capacity, rows);
	if ((st = need_ready(b, fn))) return st;
	auto& R = b->rec;
	auto alloc_zero = [&](void** p, size_t bytes) -> saip_status {
		HIP_TRY(hipMalloc(p, bytes));
		HIP_TRY(hipMemset(*p, 0, bytes));
		HIP_TRY(hipStreamSynchronize(nullptr));  // (the null-stream fill is done before the rollout writes on the batch's non-blocking stream: see dev_alloc)
		return SAIP_OK;
	};
	if (channels) {
		if ((st = alloc_zero((void**)&R.log, (size_t)capacity * slot_bytes)) || (st = alloc_zero((void**)&R.status_log, (size_t)capacity * b->ld))) {
			record_free(b);
			return st;
		}
	}
	if (summaries && (st = alloc_zero((void**)&R.summary, (size_t)saip::REC_SUMMARY_ROWS * b->ld * sizeof(double)))) {
		record_free(b);
		return st;
	}
	R.attached = true;
	R.capacity = capacity;
	R.stride = stride;
	R.channels = channels;
	R.task = task;
	R.rows = rows;
	R.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_detach(saip_batch* b) {
	saip_status st = need_recorder(b, "saip_batch_rollout_recorder_detach");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_rollout_recorder_detach"))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a recorded period may still be in flight
	record_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_reset(saip_batch* b) {
	saip_status st = need_recorder(b, "saip_batch_rollout_recorder_reset");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_rollout_recorder_reset"))) return st;
	auto& R = b->rec;
	if (R.log) HIP_TRY(hipMemsetAsync(R.log, 0, (size_t)R.capacity * R.rows * b->ld * sizeof(double), b->stream));
	if (R.status_log) HIP_TRY(hipMemsetAsync(R.status_log, 0, (size_t)R.capacity * b->ld, b->stream));
	if (R.summary) HIP_TRY(hipMemsetAsync(R.summary, 0, (size_t)saip::REC_SUMMARY_ROWS * b->ld * sizeof(double), b->stream));
	R.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_log_info(saip_batch* b, int* n_samples, int* rows, int* first_period, int* stride) {
	saip_status st = need_recorder(b, "saip_batch_rollout_log_info");
	if (st) return st;
	const auto& R = b->rec;
	const long long taken = R.channels ? R.period / R.stride : 0;  // samples written so far; the ring keeps the last `capacity`
	const long long n = taken < R.capacity ? taken : R.capacity;
	if (n_samples) *n_samples = (int)n;
	if (rows) *rows = R.rows;
	if (first_period) *first_period = n ? (int)((taken - n + 1) * R.stride) : 0;
	if (stride) *stride = R.stride;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_log_host(saip_batch* b, double* out, uint8_t* status) {
	const char* fn = "saip_batch_rollout_log_host";
	saip_status st = need_recorder(b, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	const auto& R = b->rec;
	const long long taken = R.channels ? R.period / R.stride : 0;
	const long long n = taken < R.capacity ? taken : R.capacity;
	// chronological order: the ring from the oldest sample's slot to its end, then from slot 0 (rows of consecutive slots are consecutive
	// [ld] arrays, so each piece is one 2-D copy)
	const long long first = (taken - n) % R.capacity;
	const long long piece[2][2] = {{first, first + n <= R.capacity ? n : R.capacity - first}, {0, first + n <= R.capacity ? 0 : first + n - R.capacity}};
	long long done = 0;
	for (const auto& pc : piece) {
		if (pc[1] == 0) continue;
		if (out)
			HIP_TRY(hipMemcpy2DAsync(out + (size_t)done * R.rows * b->B, (size_t)b->B * sizeof(double), R.log + (size_t)pc[0] * R.rows * b->ld,
									 (size_t)b->ld * sizeof(double), (size_t)b->B * sizeof(double), (size_t)pc[1] * R.rows, hipMemcpyDeviceToHost, b->stream));
		if (status)
			HIP_TRY(hipMemcpy2DAsync(status + (size_t)done * b->B, (size_t)b->B, R.status_log + (size_t)pc[0] * b->ld, (size_t)b->ld, (size_t)b->B,
									 (size_t)pc[1], hipMemcpyDeviceToHost, b->stream));
		done += pc[1];
	}
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_rollout_summary_host";
	saip_status st = need_recorder(b, fn);
	if (st) return st;
	if (!b->rec.summary) return fail(SAIP_ERR_ORDER, "%s: the recorder was attached without summaries", fn);
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->rec.summary, saip::REC_SUMMARY_ROWS);
}
extern "C" double* saip_batch_rollout_log_device(saip_batch* b) { return b ? b->rec.log : nullptr; }
extern "C" double* saip_batch_rollout_summary_device(saip_batch* b) { return b ? b->rec.summary : nullptr; }

// ---- goal schedules (saip_goal_schedule.hip): the user goals of every rollout period from keyframes resident on the device
static saip_status need_schedule(const saip_batch* b, int task, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task >= (int)b->sched.size() || !b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d has no goal schedule (saip_batch_goal_schedule_attach)", fn, task);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_attach(saip_batch* b, int task, int first, int count, const double* keyframes, int n_keyframes,
													   int stride, int mode, int per_instance) {
	const char* fn = "saip_batch_goal_schedule_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task < (int)b->sched.size() && b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d already has a goal schedule (saip_batch_goal_schedule_detach first)", fn, task);
	if (!keyframes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null keyframes", fn);
	const auto& T = b->tasks[task];
	if (first < 0 || count <= 0 || count > T.dev.goal_comps || first > T.dev.goal_comps - count)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: components [%d, %d + %d) outside the %d goal components of task %d", fn, first, first, count, T.dev.goal_comps, task);
	if (n_keyframes < 1 || stride < 1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_keyframes >= 1 and stride >= 1 required", fn);
	if (b->contact.attached && b->contact.sensor && b->contact.task == task && contact_rows_overlap(first, count))
		return fail(SAIP_ERR_ORDER, "%s: rows 30..35 of task %d are written by the simulated sensor of the attached contact planes", fn, task);
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].sensor && b->patch[i].task == task && contact_rows_overlap(first, count))
			return fail(SAIP_ERR_ORDER, "%s: rows 30..35 of task %d are written by the simulated sensor of its contact patch", fn, task);
	if (mode != saip::SCHED_HOLD && mode != saip::SCHED_LINEAR) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", fn, mode);
	per_instance = per_instance ? 1 : 0;
	// [K][count][ld] (or [K][count]) doubles: the byte count must fit a size_t
	const size_t frame_bytes = (size_t)count * (per_instance ? (size_t)b->ld : 1) * sizeof(double);
	if ((size_t)n_keyframes > SIZE_MAX / frame_bytes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %d keyframes of %d components are too large", fn, n_keyframes, count);
	int rot = 0;
	if (mode == saip::SCHED_LINEAR && T.dev.type == saip::TASK_MOTION_FORCE && first < 12 && first + count > 3) {
		if (first > 3 || first + count < 12)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a linear schedule must cover all or none of the rotation rows 3..11 (got [%d, %d))", fn, first, first + count);
		rot = 1;
		const size_t B = b->B, r0 = 3 - first;
		const char* bad = nullptr;
		for (size_t i = 0; i < (per_instance ? B : 1) && !bad; i++)
			bad = sched_check_rotations(n_keyframes, [&](int k, int e) {
				const size_t row = (size_t)k * count + r0 + e;
				return per_instance ? keyframes[row * B + i] : keyframes[row];
			});
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	double* key = nullptr;
	const size_t bytes = (size_t)n_keyframes * frame_bytes;
	HIP_TRY(hipMalloc((void**)&key, bytes));
	hipError_t e;
	if (per_instance) {
		e = hipMemsetAsync(key, 0, bytes, b->stream);
		if (e == hipSuccess)
			e = hipMemcpy2DAsync(key, (size_t)b->ld * sizeof(double), keyframes, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double),
								 (size_t)n_keyframes * count, hipMemcpyHostToDevice, b->stream);
	} else {
		e = hipMemcpyAsync(key, keyframes, bytes, hipMemcpyHostToDevice, b->stream);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffer may be reused by the caller right away
	if (e != hipSuccess) {
		(void)hipFree(key);
		return fail(SAIP_ERR_DEVICE, "%s: keyframe upload failed: %s", fn, hipGetErrorString(e));
	}
	if (b->sched.size() < b->tasks.size()) b->sched.resize(b->tasks.size());
	auto& S = b->sched[task];
	S.attached = true;
	S.first = first;
	S.count = count;
	S.K = n_keyframes;
	S.stride = stride;
	S.mode = mode;
	S.per_instance = per_instance;
	S.rot = rot;
	S.key = key;
	b->n_sched++;
	b->sched_period = 0;
	return SAIP_OK;
}
// one attached schedule and what hangs on it; the stream is idle
void saip::eng::schedule_release(saip_batch* b, int task) {
	auto& S = b->sched[task];
	sampler_release(b, task);  // a sampler points into the keyframes: it goes first
	(void)hipFree(S.key);
	S = saip_batch::Schedule();
	b->n_sched--;
}
extern "C" saip_status saip_batch_goal_schedule_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_goal_schedule_detach";
	saip_status st = task == -1 ? need_controller(b, fn) : need_schedule(b, task, fn);
	if (st) return st;
	if (task == -1 && b->n_sched == 0) return SAIP_OK;
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a scheduled period may still be in flight
	for (int t = 0; t < (int)b->sched.size(); t++) {
		auto& S = b->sched[t];
		if (!S.attached || (task != -1 && t != task)) continue;
		schedule_release(b, t);
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_rewind(saip_batch* b) {
	saip_status st = need_controller(b, "saip_batch_goal_schedule_rewind");
	if (st) return st;
	b->sched_period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_info(saip_batch* b, int task, int* first, int* count, int* n_keyframes, int* stride, int* mode,
													 long long* period) {
	saip_status st = need_schedule(b, task, "saip_batch_goal_schedule_info");
	if (st) return st;
	const auto& S = b->sched[task];
	if (first) *first = S.first;
	if (count) *count = S.count;
	if (n_keyframes) *n_keyframes = S.K;
	if (stride) *stride = S.stride;
	if (mode) *mode = S.mode;
	if (period) *period = b->sched_period;
	return SAIP_OK;
}
extern "C" double* saip_batch_goal_schedule_device(saip_batch* b, int task) {
	return (b && task >= 0 && task < (int)b->sched.size()) ? b->sched[task].key : nullptr;
}
// the goals of rollout period c = sched_period, written in front of the period's OTG step and cycle: one launch for every schedule; the
// keyframe index and the fraction are computed here, at enqueue time (no device-side counter)
static saip_status apply_schedules(saip_batch* b) {
	saip::ScheduleParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	const long long c = b->sched_period++;
	for (int t = 0; t < (int)b->sched.size(); t++) {
		const auto& S = b->sched[t];
		if (!S.attached) continue;
		auto& E = P.e[P.n++];
		E.goal = b->tasks[t].goal_dev;
		E.key = S.key;
		E.first = S.first;
		E.count = S.count;
		E.K = S.K;
		const bool past = c >= (long long)(S.K - 1) * S.stride;  // the last keyframe is held
		E.i = past ? S.K - 1 : (int)(c / S.stride);
		E.s = past ? 0.0 : (double)(c % S.stride) / (double)S.stride;
		E.mode = S.mode;
		E.per_instance = S.per_instance;
		E.rot = S.rot;
	}
	hipError_t e = saip::launch_goal_schedule(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "goal schedule launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}

// steps x { internal OTGs, control cycle, integrate } on the engine stream, no host synchronisation.  One period is 3-5 small
// launches.  Plain back-to-back stream launches are the default: they were measured FASTER than replaying a hipGraph of the period
// (68.6 vs 74.2 us per period at B = 4096, 65.7 vs 70.4 us at B = 256, tools/rollout_bench.py) -- the host enqueues far ahead of the
// device either way, and the graph adds inter-node latency.
extern "C" saip_status saip_batch_rollout_async(saip_batch* b, int steps, double sim_dt, int substeps, const double* gravity, double damping) {
	saip_status st = need_ready(b, "saip_batch_rollout_async");
	if (st) return st;
	if (steps < 1 || !(sim_dt > 0) || substeps < 1 || damping < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_rollout_async: bad arguments");
	SimRequest sim = {substeps, sim_dt, damping, {0, 0, 0}};
	for (int i = 0; i < 3; i++) sim.gravity[i] = gravity ? gravity[i] : b->model->dev.gravity[i];
	const saip::SimPlan plan = sim_plan(b);  // once per call: nothing attaches or detaches between its periods
	const bool patch_sensor = patch_any_sensor(b);
	const int sense_slots = b->sensing.attached ? sensing_sensor_slots(b, true, true) : 0;
	auto period = [&](const bool more = false) -> saip_status {  // more: another period follows inside this call
		// goal schedules: every period starts with the launch that writes its goals
		if (b->n_sched > 0 && (st = apply_schedules(b))) return st;
		// environment schedules: this period's planes (held through its substeps) and the obstacles at the time of the state the monitor will
		// look at; the launch reads no state, so the fused forms below stay in use
		if (b->n_env > 0 && (st = env_apply(b, sim_dt * substeps))) return st;
		// contact planes with the simulated sensor: the sensed wrench of this period's state, in front of the OTGs (which pass it on) and the cycle
		if (b->contact.attached && b->contact.sensor && (st = contact_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
		if (patch_sensor && (st = patch_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
		// a sensing model: this period's measurement of q, dq and the perturbation of the wrench just sensed, in one launch
		if (b->sensing.attached &&
			(st = sensing_launch(b, (b->sensing.epoch != b->state_epoch ? saip::SENSE_MODE_JOINTS : 0) | saip::SENSE_MODE_WRENCH, sense_slots)))
			return st;
		// guards: this period's evaluation behind everything that writes what it reads (goals, sensed wrench, measurement) and in front of
		// the OTG step and the cycle, which see a goal it writes as they see a host setGoal
		if (b->guard.attached && (st = guard_launch(b))) return st;
		// no internal OTG in the stack: the cycle launch integrates the state itself when it can (eight-lane kernel, no slow path behind)
		bool integrated = false;
		saip_status s2 = launch_cycle(b, false, plan.offer_cycle_sim ? &sim : nullptr, &integrated);
		if (s2) {
			b->otg_prelaunched = false;  // a failed period must not leave the next standalone cycle believing its OTG step has already run
			return s2;
		}
		if (integrated) {
			state_moved(b);  // (no plant and no sensing model on this branch: the plan offers it with neither attached, so their counters stay)
		} else if ((s2 = enqueue_integrate(b, plan, sim_dt, substeps, gravity, damping, more && plan.may_fuse_next_otg))) {
			b->otg_prelaunched = false;
			return s2;
		}
		// the clearance monitor observes the integrated state, whichever form integrated it, in front of the recorder
		if (b->clearance.attached && (s2 = clearance_launch(b, saip::CLEARANCE_MONITOR, sim_dt * substeps))) return s2;
		return b->rec.attached ? record_period(b, sim_dt * substeps) : SAIP_OK;
	};
	for (int done = 0; done < steps; done++)
		if ((st = period(done + 1 < steps))) return st;
	return SAIP_OK;
}
