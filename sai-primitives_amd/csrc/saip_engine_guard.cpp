#include "saip_engine_internal.h"

// ---- resident guards (saip_guard.hip): event-triggered phases and goal switching inside the rollout periods
static saip_status need_guard(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->guard.attached) return fail(SAIP_ERR_ORDER, "%s: no guards are attached (saip_batch_guard_attach)", fn);
	return SAIP_OK;
}
void saip::eng::guard_free(saip_batch* b) {
	auto& H = b->guard;
	for (void* p : {(void*)H.guards, (void*)H.phases, (void*)H.ints, (void*)H.latch, (void*)H.readout})
		if (p) (void)hipFree(p);
	H = saip_batch::Guard();
}
static const char* const GUARD_WORD_NAMES[saip::GUARD_WORDS] = {"from", "to", "signal", "axis", "cmp", "threshold", "hold", "blank"};
static const char* const GUARD_PHASE_WORD_NAMES[saip::GUARD_PHASE_WORDS] = {"mode", "dx", "dy", "dz"};
// the guard table [G][8] (cols = 1) or [G][8][cols] against P phases: true when fine (*need: the GUARD_NEED_* bits of its signals), else msg
// names the guard, the word and the instance
static bool guard_check_guards(const double* t, int G, size_t cols, int P, int* need, char* msg, size_t len) {
	*need = 0;
	for (int g = 0; g < G; g++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)g * saip::GUARD_WORDS * cols + i;
			char where[48] = "";
			if (cols > 1) snprintf(where, sizeof(where), " of instance %zu", i);
			auto word = [&](int k) { return w[(size_t)k * cols]; };
			auto bad = [&](int k, const char* what) { return snprintf(msg, len, "guard %d%s: word %s = %g %s", g, where, GUARD_WORD_NAMES[k], word(k), what), false; };
			for (int k = 0; k < saip::GUARD_WORDS; k++) {
				if (!std::isfinite(word(k))) return bad(k, "is not finite");
				if (k != saip::GUARD_THRESHOLD && word(k) != std::floor(word(k))) return bad(k, "is not an integer");
			}
			for (int k : {saip::GUARD_FROM, saip::GUARD_TO})
				if (word(k) < 0 || word(k) >= P) return bad(k, "is outside the phases");
			const double sig = word(saip::GUARD_SIGNAL), axis = word(saip::GUARD_AXIS);
			if (sig < 0 || sig >= saip::GUARD_SIGNAL_COUNT) return bad(saip::GUARD_SIGNAL, "is no signal");
			const int s = (int)sig;
			const bool wrench = s == saip::GUARD_SIGNAL_FORCE || s == saip::GUARD_SIGNAL_MOMENT;
			const double top = wrench ? 3 : s == saip::GUARD_SIGNAL_POSITION ? 2 : 0;
			if (axis < 0 || axis > top) return bad(saip::GUARD_AXIS, "is no axis of the signal");
			if (word(saip::GUARD_CMP) != 0 && word(saip::GUARD_CMP) != 1) return bad(saip::GUARD_CMP, "is neither 0 (>=) nor 1 (<=)");
			if (word(saip::GUARD_HOLD) < 1) return bad(saip::GUARD_HOLD, "is below 1");
			if (word(saip::GUARD_BLANK) < 0) return bad(saip::GUARD_BLANK, "is below 0");
			*need |= s == saip::GUARD_SIGNAL_FORCE ? saip::GUARD_NEED_FORCE
					 : s == saip::GUARD_SIGNAL_MOMENT ? saip::GUARD_NEED_MOMENT
					 : s == saip::GUARD_SIGNAL_POSITION ? saip::GUARD_NEED_FK
					 : s == saip::GUARD_SIGNAL_POS_ERROR || s == saip::GUARD_SIGNAL_ORI_ERROR ? (saip::GUARD_NEED_FK | saip::GUARD_NEED_ERROR)
					 : s == saip::GUARD_SIGNAL_JOINT_SPEED ? saip::GUARD_NEED_SPEED : 0;
		}
	return true;
}
// the phase table [P][4]
static bool guard_check_phases(const double* t, int P, int* need, char* msg, size_t len) {
	*need = 0;
	for (int p = 0; p < P; p++) {
		const double* w = t + (size_t)p * saip::GUARD_PHASE_WORDS;
		if (!(w[0] == saip::GUARD_MODE_FREE || w[0] == saip::GUARD_MODE_HOLD || w[0] == saip::GUARD_MODE_OFFSET))
			return snprintf(msg, len, "phase %d: word mode = %g is no mode (0 FREE, 1 HOLD, 2 OFFSET)", p, w[0]), false;
		if (p == 0 && w[0] != saip::GUARD_MODE_FREE) return snprintf(msg, len, "phase 0: word mode = %g: phase 0 must be FREE (nothing is latched yet)", w[0]), false;
		for (int k = 1; k < saip::GUARD_PHASE_WORDS; k++)
			if (!std::isfinite(w[k])) return snprintf(msg, len, "phase %d: word %s is not finite", p, GUARD_PHASE_WORD_NAMES[k]), false;
		if (w[0] != saip::GUARD_MODE_FREE) *need |= saip::GUARD_NEED_FK;
	}
	return true;
}
static saip::GuardParams guard_params(const saip_batch* b) {
	const auto& H = b->guard;
	saip::GuardParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.task = H.task;
	P.G = H.G;
	P.P = H.P;
	P.per_instance = H.per_instance;
	P.need = H.need_guards | H.need_phases;
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = controller_q(b);
	P.dq = controller_dq(b);
	P.guards = H.guards;
	P.phases = H.phases;
	P.goal = b->tasks[H.task].goal_dev;
	const size_t ld = b->ld;
	P.phase = H.ints;
	P.since = H.ints + ld;
	P.clock = H.ints + 2 * ld;
	P.run = H.ints + 3 * ld;
	P.entry = P.run + (size_t)H.G * ld;
	P.fires = P.entry + (size_t)H.P * ld;
	P.latch = H.latch;
	P.readout = H.readout;
	return P;
}
// the state of _attach and _reset, on the stream
static saip_status guard_reset(saip_batch* b) {
	HIP_TRY(saip::launch_guard_reset(guard_params(b), b->stream));
	return SAIP_OK;
}
// one evaluation of every instance at the state the controller reads (made current first while a sensing model is attached)
saip_status saip::eng::guard_launch(saip_batch* b) {
	saip_status st = ensure_task_constants(b);
	if (st || (st = sensing_refresh(b))) return st;
	hipError_t e = saip::launch_guard_apply(guard_params(b), b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "guard launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
void saip::eng::guard_segments(const saip_batch* b, saip::GuardParams* P) { *P = guard_params(b); }

extern "C" saip_status saip_batch_guard_attach(saip_batch* b, int task, int n_guards, const double* guards, int per_instance, int n_phases, const double* phases) {
	const char* fn = "saip_batch_guard_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (b->tasks[task].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, task);
	if (b->guard.attached) return fail(SAIP_ERR_ORDER, "%s: guards are already attached (saip_batch_guard_detach first)", fn);
	const int G = n_guards, NP = n_phases;
	if (G < 1 || G > saip::GUARD_MAX_GUARDS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d guards required (got %d)", fn, saip::GUARD_MAX_GUARDS, G);
	if (NP < 1 || NP > saip::GUARD_MAX_PHASES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d phases required (got %d)", fn, saip::GUARD_MAX_PHASES, NP);
	if (!guards || !phases) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null guards or phases", fn);
	per_instance = per_instance ? 1 : 0;
	char msg[200];
	int need_g = 0, need_p = 0;
	if (!guard_check_phases(phases, NP, &need_p, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (!guard_check_guards(guards, G, per_instance ? (size_t)b->B : 1, NP, &need_g, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [G][8][ld] doubles: the byte count must fit a size_t
	const size_t widest = (size_t)saip::GUARD_MAX_GUARDS * saip::GUARD_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& H = b->guard;
	H = saip_batch::Guard();
	H.task = task;
	H.G = G;
	H.P = NP;
	H.per_instance = per_instance;
	H.need_guards = need_g;
	H.need_phases = need_p;
	const size_t ld = b->ld, rows = (size_t)G * saip::GUARD_WORDS;
	if ((st = alloc_zero(b, &H.guards, rows * (per_instance ? ld : 1))) || (st = alloc_zero(b, &H.phases, (size_t)NP * saip::GUARD_PHASE_WORDS)) ||
		(st = alloc_zero(b, &H.ints, (size_t)(3 + 2 * G + NP) * ld)) || (st = alloc_zero(b, &H.latch, (size_t)saip::GUARD_LATCH_ROWS * ld)) ||
		(st = alloc_zero(b, &H.readout, (size_t)saip::GUARD_READOUT_ROWS * ld)) || (st = upload_table(b, H.guards, guards, rows, per_instance, "guard", fn)) ||
		(st = upload_table(b, H.phases, phases, (size_t)NP * saip::GUARD_PHASE_WORDS, 0, "phase", fn)) || (st = guard_reset(b))) {
		guard_free(b);
		return st;
	}
	H.attached = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_guard_detach(saip_batch* b) {
	const char* fn = "saip_batch_guard_detach";
	saip_status st = need_guard(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // an evaluation may still be in flight
	guard_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_guard_info(saip_batch* b, int* task, int* n_guards, int* per_instance, int* n_phases, int* needs_pose) {
	saip_status st = need_guard(b, "saip_batch_guard_info");
	if (st) return st;
	const auto& H = b->guard;
	if (task) *task = H.task;
	if (n_guards) *n_guards = H.G;
	if (per_instance) *per_instance = H.per_instance;
	if (n_phases) *n_phases = H.P;
	if (needs_pose) *needs_pose = ((H.need_guards | H.need_phases) & saip::GUARD_NEED_FK) ? 1 : 0;
	return SAIP_OK;
}
// the state stays: the next evaluation runs the new table over the phases, counters and latches there are (_reset starts afresh)
extern "C" saip_status saip_batch_guard_set_guards_host(saip_batch* b, const double* guards) {
	const char* fn = "saip_batch_guard_set_guards_host";
	saip_status st = need_guard(b, fn);
	if (st) return st;
	if (!guards) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null guards", fn);
	auto& H = b->guard;
	char msg[200];
	int need = 0;
	if (!guard_check_guards(guards, H.G, H.per_instance ? (size_t)b->B : 1, H.P, &need, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	if ((st = upload_table(b, H.guards, guards, (size_t)H.G * saip::GUARD_WORDS, H.per_instance, "guard", fn))) return st;
	H.need_guards = need;
	return SAIP_OK;
}
extern "C" double* saip_batch_guard_guards_device(saip_batch* b) { return b ? b->guard.guards : nullptr; }
extern "C" saip_status saip_batch_guard_reset(saip_batch* b) {
	const char* fn = "saip_batch_guard_reset";
	saip_status st = need_guard(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return guard_reset(b);
}
extern "C" saip_status saip_batch_guard_evaluate(saip_batch* b) {
	const char* fn = "saip_batch_guard_evaluate";
	saip_status st = need_guard(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return guard_launch(b);
}
extern "C" saip_status saip_batch_guard_state_device(saip_batch* b, int** phase, int** since, int** clock, int** run, int** entry, int** fires, double** latch) {
	saip_status st = need_guard(b, "saip_batch_guard_state_device");
	if (st) return st;
	const saip::GuardParams P = guard_params(b);
	if (phase) *phase = P.phase;
	if (since) *since = P.since;
	if (clock) *clock = P.clock;
	if (run) *run = P.run;
	if (entry) *entry = P.entry;
	if (fires) *fires = P.fires;
	if (latch) *latch = P.latch;
	return SAIP_OK;
}
// the state for tests and sweeps: phase, since, clock [B]; run, fires [G][B]; entry [P][B]; latch [12][B]; any may be null
extern "C" saip_status saip_batch_guard_state_host(saip_batch* b, int* phase, int* since, int* clock, int* run, int* entry, int* fires, double* latch) {
	const char* fn = "saip_batch_guard_state_host";
	saip_status st = need_guard(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	const saip::GuardParams P = guard_params(b);
	const struct { int* host; const int* dev; int rows; } parts[6] = {{phase, P.phase, 1}, {since, P.since, 1}, {clock, P.clock, 1}, {run, P.run, P.G}, {entry, P.entry, P.P}, {fires, P.fires, P.G}};
	for (const auto& a : parts)
		if (a.host)
			HIP_TRY(hipMemcpy2DAsync(a.host, (size_t)b->B * sizeof(int), a.dev, (size_t)b->ld * sizeof(int), (size_t)b->B * sizeof(int), a.rows, hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return latch ? copy_d2h(b, latch, P.latch, saip::GUARD_LATCH_ROWS) : SAIP_OK;
}
extern "C" saip_status saip_batch_guard_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_guard_readout_host";
	const saip_status st = need_guard(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->guard.readout, saip::GUARD_READOUT_ROWS, fn);
}
extern "C" double* saip_batch_guard_readout_device(saip_batch* b) { return b ? b->guard.readout : nullptr; }
extern "C" saip_status saip_batch_guard_add_cost(saip_batch* b, int phase, double w_time, double w_miss) {
	const char* fn = "saip_batch_guard_add_cost";
	saip_status st = need_guard(b, fn);
	if (st) return st;
	if (b->n_samp == 0) return fail(SAIP_ERR_ORDER, "%s: no sampler is attached (saip_batch_sampler_attach): there is no cost to add to", fn);
	if (phase < 0 || phase >= b->guard.P) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: phase %d outside the %d phases", fn, phase, b->guard.P);
	if (w_time != w_time || w_miss != w_miss) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a weight is NaN", fn);
	if ((st = need_ready(b, fn))) return st;
	const saip::GuardParams P = guard_params(b);
	HIP_TRY(saip::launch_guard_add_cost(b->B, P.entry + (size_t)phase * b->ld, b->samp_cost, w_time, w_miss, b->stream));
	return SAIP_OK;
}
