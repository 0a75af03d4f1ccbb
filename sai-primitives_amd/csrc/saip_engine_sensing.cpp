#include "saip_engine_internal.h"

// ---- the sensing model (saip_sense.hip): offset, noise and quantisation between the resident state and what the controller reads of it
static saip_status need_sensing(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->sensing.attached) return fail(SAIP_ERR_ORDER, "%s: no sensing model is attached (saip_batch_sensing_attach)", fn);
	return SAIP_OK;
}
void saip::eng::sensing_free(saip_batch* b) {
	auto& C = b->sensing;
	chain_free(C.chain);  // the chain goes with its carrier
	for (void* p : {(void*)C.joints, (void*)C.wrenches, (void*)C.q_meas, (void*)C.dq_meas, (void*)C.bounds})
		if (p) (void)hipFree(p);
	C = saip_batch::Sensing();
}
static const char* const SENSE_JOINT_WORD_NAMES[saip::SENSE_JOINT_WORDS] = {"q_off", "q_res", "q_sigma", "dq_off", "dq_res", "dq_sigma"};
static const char* const SENSE_AXIS_WORD_NAMES[saip::SENSE_AXIS_WORDS] = {"off", "res", "sigma"};
static const char* const SENSE_AXIS_NAMES[6] = {"F[0]", "F[1]", "F[2]", "M[0]", "M[1]", "M[2]"};
// one word: an offset finite, a resolution or a sigma finite and not negative; nullptr when fine
static const char* sense_check_word(double v, int kind, char* buf, size_t len, const char* name) {
	if (v != v) return snprintf(buf, len, "word %s is NaN", name), buf;
	if (!std::isfinite(v)) return snprintf(buf, len, "word %s is not finite", name), buf;
	if (kind != saip::SENSE_OFF && v < 0) return snprintf(buf, len, "word %s = %g is below 0", name, v), buf;
	return nullptr;
}
// a joint table [n][6] (cols = 1) or [n][6][cols]: true when fine, else msg names the joint and the word (and the instance)
static bool sense_check_joints(const double* t, int n, size_t cols, char* msg, size_t len) {
	using namespace saip;
	char buf[96];
	for (int j = 0; j < n; j++)
		for (size_t i = 0; i < cols; i++)
			for (int k = 0; k < SENSE_JOINT_WORDS; k++)
				if (const char* bad = sense_check_word(t[((size_t)j * SENSE_JOINT_WORDS + k) * cols + i], k % SENSE_AXIS_WORDS, buf, sizeof(buf), SENSE_JOINT_WORD_NAMES[k])) {
					if (cols > 1) snprintf(msg, len, "joint %d of instance %zu: %s", j, i, bad);
					else snprintf(msg, len, "joint %d: %s", j, bad);
					return false;
				}
	return true;
}
// the wrench tables [S][6][3] or [S][6][3][cols]; msg names the task, the axis and the word (and the instance)
static bool sense_check_wrenches(const double* t, int S, const int* tasks, size_t cols, char* msg, size_t len) {
	using namespace saip;
	char buf[96];
	for (int s = 0; s < S; s++)
		for (int a = 0; a < 6; a++)
			for (size_t i = 0; i < cols; i++)
				for (int k = 0; k < SENSE_AXIS_WORDS; k++)
					if (const char* bad = sense_check_word(t[((size_t)s * SENSE_WRENCH_WORDS + a * SENSE_AXIS_WORDS + k) * cols + i], k, buf, sizeof(buf), SENSE_AXIS_WORD_NAMES[k])) {
						if (cols > 1) snprintf(msg, len, "task %d: axis %s of instance %zu: %s", tasks[s], SENSE_AXIS_NAMES[a], i, bad);
						else snprintf(msg, len, "task %d: axis %s: %s", tasks[s], SENSE_AXIS_NAMES[a], bad);
						return false;
					}
	return true;
}
extern "C" saip_status saip_batch_sensing_attach(saip_batch* b, const double* joint_table, int per_instance_joints, int n_wrench_tasks, const int* tasks,
												  const double* wrench_tables, int per_instance_wrenches, unsigned long long seed) {
	const char* fn = "saip_batch_sensing_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->sensing.attached) return fail(SAIP_ERR_ORDER, "%s: a sensing model is already attached (saip_batch_sensing_detach first)", fn);
	const int S = n_wrench_tasks, n = b->model->n;
	if (S < 0 || S > saip::SENSE_MAX_WRENCH_TASKS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d wrench tasks required (got %d)", fn, saip::SENSE_MAX_WRENCH_TASKS, S);
	if (S > 0 && (!tasks || !wrench_tables)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null tasks or wrench tables", fn);
	for (int s = 0; s < S; s++) {
		if (tasks[s] < 0 || tasks[s] >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, tasks[s]);
		if (b->tasks[tasks[s]].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, tasks[s]);
		if (s > 0 && tasks[s] == tasks[0]) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is named twice", fn, tasks[s]);
	}
	per_instance_joints = per_instance_joints ? 1 : 0;
	per_instance_wrenches = per_instance_wrenches && S > 0 ? 1 : 0;
	const size_t jcols = per_instance_joints ? (size_t)b->B : 1, wcols = per_instance_wrenches ? (size_t)b->B : 1;
	std::vector<double> neutral;
	if (!joint_table) {
		neutral.assign((size_t)n * saip::SENSE_JOINT_WORDS * jcols, 0.0);
		joint_table = neutral.data();
	}
	char msg[200];
	if (!sense_check_joints(joint_table, n, jcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (S > 0 && !sense_check_wrenches(wrench_tables, S, tasks, wcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [n][6][ld] doubles: the byte count must fit a size_t
	const size_t widest = (size_t)(n > 6 ? n : 6) * saip::SENSE_JOINT_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->sensing;
	C = saip_batch::Sensing();
	const size_t ld = b->ld, jrows = (size_t)n * saip::SENSE_JOINT_WORDS, wrows = (size_t)S * saip::SENSE_WRENCH_WORDS;
	if ((st = alloc_zero(b, &C.joints, jrows * (per_instance_joints ? ld : 1))) || (S > 0 && (st = alloc_zero(b, &C.wrenches, wrows * (per_instance_wrenches ? ld : 1)))) ||
		(st = alloc_zero(b, &C.q_meas, (size_t)n * ld)) || (st = alloc_zero(b, &C.dq_meas, (size_t)n * ld)) ||
		((per_instance_joints || per_instance_wrenches) && (st = alloc_zero(b, &C.bounds, 2 * (jrows + wrows)))) ||
		(st = upload_table(b, C.joints, joint_table, jrows, per_instance_joints, "table", fn)) ||
		(S > 0 && (st = upload_table(b, C.wrenches, wrench_tables, wrows, per_instance_wrenches, "table", fn)))) {
		sensing_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance_joints = per_instance_joints;
	C.n_wrench_tasks = S;
	C.per_instance_wrenches = per_instance_wrenches;
	C.seed = seed;
	C.period = 0;
	C.epoch = -1;
	for (int s = 0; s < S; s++) C.task[s] = tasks[s];
	// as the plant's and the inertia table's attach: the flag is only ever set between two periods of one rollout call (its last period
	// does not run the next OTG step ahead), so it is false here already and no OTG step can run twice; cleared to say so
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_detach(saip_batch* b) {
	const char* fn = "saip_batch_sensing_detach";
	saip_status st = need_sensing(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a cycle that reads the measured arrays may still be in flight
	sensing_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_info(saip_batch* b, int* per_instance_joints, int* n_wrench_tasks, int* per_instance_wrenches, long long* period) {
	saip_status st = need_sensing(b, "saip_batch_sensing_info");
	if (st) return st;
	const auto& C = b->sensing;
	if (per_instance_joints) *per_instance_joints = C.per_instance_joints;
	if (n_wrench_tasks) *n_wrench_tasks = C.n_wrench_tasks;
	if (per_instance_wrenches) *per_instance_wrenches = C.per_instance_wrenches;
	if (period) *period = C.period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_set_joints_host(saip_batch* b, const double* joint_table) {
	const char* fn = "saip_batch_sensing_set_joints_host";
	saip_status st = need_sensing(b, fn);
	if (st) return st;
	if (!joint_table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null joint table", fn);
	auto& C = b->sensing;
	char msg[200];
	if (!sense_check_joints(joint_table, b->model->n, C.per_instance_joints ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	C.epoch = -1;
	return upload_table(b, C.joints, joint_table, (size_t)b->model->n * saip::SENSE_JOINT_WORDS, C.per_instance_joints, "table", fn);
}
extern "C" saip_status saip_batch_sensing_set_wrenches_host(saip_batch* b, const double* wrench_tables) {
	const char* fn = "saip_batch_sensing_set_wrenches_host";
	saip_status st = need_sensing(b, fn);
	if (st) return st;
	auto& C = b->sensing;
	if (C.n_wrench_tasks == 0) return fail(SAIP_ERR_ORDER, "%s: the sensing model was attached without wrench tasks", fn);
	if (!wrench_tables) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null wrench tables", fn);
	char msg[200];
	if (!sense_check_wrenches(wrench_tables, C.n_wrench_tasks, C.task, C.per_instance_wrenches ? (size_t)b->B : 1, msg, sizeof(msg)))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	C.epoch = -1;
	return upload_table(b, C.wrenches, wrench_tables, (size_t)C.n_wrench_tasks * saip::SENSE_WRENCH_WORDS, C.per_instance_wrenches, "table", fn);
}
extern "C" saip_status saip_batch_sensing_seed(saip_batch* b, unsigned long long seed) {
	saip_status st = need_sensing(b, "saip_batch_sensing_seed");
	if (st) return st;
	b->sensing.seed = seed;
	b->sensing.epoch = -1;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_set_period(saip_batch* b, long long period) {
	const char* fn = "saip_batch_sensing_set_period";
	saip_status st = need_sensing(b, fn);
	if (st) return st;
	if (period < 0 || period > 0xFFFFFFFFLL) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0 <= period < 2^32 required (got %lld)", fn, period);
	b->sensing.period = period;
	b->sensing.epoch = -1;
	return SAIP_OK;
}
// Per-instance tables drawn on the device between two batch-uniform tables (host pointers: joints [n][6], wrenches [S][6][3]); a null pair
// leaves that table alone.  Both bounds of every word have to be valid words, so every draw between them is.
extern "C" saip_status saip_batch_sensing_randomize(saip_batch* b, unsigned long long seed, long long round, const double* joint_lo, const double* joint_hi,
													 const double* wrench_lo, const double* wrench_hi) {
	using namespace saip;
	const char* fn = "saip_batch_sensing_randomize";
	saip_status st = need_sensing(b, fn);
	if (st) return st;
	auto& C = b->sensing;
	const int n = b->model->n, S = C.n_wrench_tasks;
	if ((st = check_bound_pairs(fn, joint_lo, joint_hi, wrench_lo, wrench_hi))) return st;
	if (joint_lo && !C.per_instance_joints) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the joint table is batch-uniform (attach it per instance)", fn);
	if (wrench_lo && (S == 0 || !C.per_instance_wrenches)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the wrench tables are batch-uniform or empty (attach them per instance)", fn);
	const size_t jrows = (size_t)n * SENSE_JOINT_WORDS, wrows = (size_t)S * SENSE_WRENCH_WORDS;
	// no word of either table may be infinite: nothing to scan for a bound infinite on one side only
	if (joint_lo && (st = check_bound_pair(fn, joint_lo, joint_hi, [&](const double* t, char* msg, size_t len) { return sense_check_joints(t, n, 1, msg, len); }))) return st;
	if (wrench_lo && (st = check_bound_pair(fn, wrench_lo, wrench_hi, [&](const double* t, char* msg, size_t len) { return sense_check_wrenches(t, S, C.task, 1, msg, len); })))
		return st;
	if ((st = need_ready(b, fn))) return st;
	SenseRandomParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = n;
	P.n_slots = S;
	P.seed_lo = (uint32_t)seed;
	P.seed_hi = (uint32_t)(seed >> 32);
	P.round = (uint32_t)round;
	double* jb = C.bounds;
	double* wb = C.bounds + 2 * jrows;
	if (joint_lo) {
		if ((st = upload_bound_pair(b, jb, joint_lo, joint_hi, jrows, fn))) return st;
		P.joints = C.joints;
		P.joint_lo = jb;
		P.joint_hi = jb + jrows;
	}
	if (wrench_lo) {
		if ((st = upload_bound_pair(b, wb, wrench_lo, wrench_hi, wrows, fn))) return st;
		P.wrenches = C.wrenches;
		P.wrench_lo = wb;
		P.wrench_hi = wb + wrows;
	}
	hipError_t e = saip::launch_sense_randomize(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "sensing randomize launch failed: %s", hipGetErrorString(e));
	C.epoch = -1;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_measure(saip_batch* b) {
	const char* fn = "saip_batch_sensing_measure";
	saip_status st = need_sensing(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return sensing_launch(b, saip::SENSE_MODE_JOINTS, 0);
}
extern "C" saip_status saip_batch_sensing_measured_host(saip_batch* b, double* q, double* dq) {
	const char* fn = "saip_batch_sensing_measured_host";
	saip_status st = need_sensing(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	if (q && (st = copy_d2h(b, q, b->sensing.q_meas, b->model->n))) return st;
	if (dq && (st = copy_d2h(b, dq, b->sensing.dq_meas, b->model->n))) return st;
	return SAIP_OK;
}
extern "C" double* saip_batch_sensing_joints_device(saip_batch* b) { return b ? b->sensing.joints : nullptr; }
extern "C" double* saip_batch_sensing_wrenches_device(saip_batch* b) { return b ? b->sensing.wrenches : nullptr; }
extern "C" double* saip_batch_sensing_measured_q_device(saip_batch* b) { return b ? b->sensing.q_meas : nullptr; }
extern "C" double* saip_batch_sensing_measured_dq_device(saip_batch* b) { return b ? b->sensing.dq_meas : nullptr; }
// the wrench slots whose task's simulated sensor is written by the SENSE launch of the contact planes (planes) or of the patches
int saip::eng::sensing_sensor_slots(const saip_batch* b, bool planes, bool patches) {
	const auto& C = b->sensing;
	int mask = 0;
	for (int s = 0; s < C.n_wrench_tasks; s++) {
		if (planes && b->contact.attached && b->contact.sensor && b->contact.task == C.task[s]) mask |= 1 << s;
		for (int i = 0; patches && i < b->n_patch; i++)
			if (b->patch[i].sensor && b->patch[i].task == C.task[s]) mask |= 1 << s;
	}
	return mask;
}
// one launch of the sensing kernel: the JOINTS part takes the measurement of the resident state as it is now (and marks it current), the
// WRENCH part perturbs the sensed wrench of the slots in slot_mask, which a SENSE launch has just written
saip_status saip::eng::sensing_launch(saip_batch* b, int mode, int slot_mask) {
	auto& C = b->sensing;
	if (!slot_mask) mode &= ~saip::SENSE_MODE_WRENCH;
	if (!mode) return SAIP_OK;
	saip::SenseParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.per_instance_joints = C.per_instance_joints;
	P.per_instance_wrenches = C.per_instance_wrenches;
	P.n_slots = C.n_wrench_tasks;
	P.slot_mask = slot_mask;
	P.seed_lo = (uint32_t)C.seed;
	P.seed_hi = (uint32_t)(C.seed >> 32);
	P.period = (uint32_t)C.period;
	P.q = b->q;
	P.dq = b->dq;
	P.joints = C.joints;
	P.q_meas = C.q_meas;
	P.dq_meas = C.dq_meas;
	P.wrenches = C.wrenches;
	for (int s = 0; s < C.n_wrench_tasks; s++) P.goal[s] = b->tasks[C.task[s]].goal_dev;
	hipError_t e;
	if (C.chain.attached) {
		// the chain's kernel in place of the sensing model's, wherever that would be enqueued: every JOINTS launch is one sample of the chain
		const auto& H = C.chain;
		saip::SenseChainParams Q;
		memset(&Q, 0, sizeof(Q));
		Q.S = P;
		Q.per_instance = H.per_instance;
		Q.depth = H.depth;
		Q.sample_time = C.chain_sample_time;
		Q.table = H.table;
		Q.taps = H.taps;
		Q.filt = H.filt;
		Q.primed = H.primed;
		e = saip::launch_sense_chain_apply(Q, b->stream);
	} else e = saip::launch_sense_apply(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "sensing launch failed: %s", hipGetErrorString(e));
	if (mode & saip::SENSE_MODE_JOINTS) C.epoch = b->state_epoch;
	return SAIP_OK;
}
// in front of a launch that reads the controller's state: the measurement made current when the state (or the model) changed since
saip_status saip::eng::sensing_refresh(saip_batch* b) {
	if (!b->sensing.attached || b->sensing.epoch == b->state_epoch) return SAIP_OK;
	return sensing_launch(b, saip::SENSE_MODE_JOINTS, 0);
}

// ---- the sensing chain (saip_sense_chain.hip): delay line, finite-difference velocity and low-pass behind the sensing model's joint rows.
// The host side is saip_engine_chain.cpp's; its own here: the sample time, and the measured copy gone stale (epoch = -1) whenever the
// chain that wrote it comes, goes or starts afresh.
static saip_status need_chain(const saip_batch* b, const char* fn) {
	saip_status st = need_sensing(b, fn);
	return st ? st : chain_need(sense_chain_kind(), b->sensing.chain, fn);
}
extern "C" saip_status saip_batch_sensing_chain_attach(saip_batch* b, const double* table, int per_instance, int depth, double sample_time) {
	const char* fn = "saip_batch_sensing_chain_attach";
	saip_status st = chain_attach_depth(sense_chain_kind(), b, depth, fn);
	if (st) return st;
	if (!(sample_time > 0) || !std::isfinite(sample_time)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a finite sample time > 0 required (got %g)", fn, sample_time);
	if ((st = chain_attach(sense_chain_kind(), b, b->sensing.chain, b->sensing.attached, table, per_instance, depth, fn))) return st;
	b->sensing.chain_sample_time = sample_time;
	b->sensing.epoch = -1;  // the next read of the state takes the chain's first sample, which primes it
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_chain_detach(saip_batch* b) {
	const char* fn = "saip_batch_sensing_chain_detach";
	saip_status st = need_chain(b, fn);
	if (st || (st = chain_detach(b, b->sensing.chain, fn))) return st;
	b->sensing.chain_sample_time = 0;
	b->sensing.epoch = -1;  // the measured copy holds the chain's output: the sensing model alone measures again
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_chain_info(saip_batch* b, int* attached, int* per_instance, int* depth, double* sample_time, size_t* state_bytes) {
	saip_status st = need_sensing(b, "saip_batch_sensing_chain_info");
	if (st) return st;
	chain_info(sense_chain_kind(), b, b->sensing.chain, attached, per_instance, depth, state_bytes);
	if (sample_time) *sample_time = b->sensing.chain_sample_time;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_chain_set_table_host(saip_batch* b, const double* table) {
	const char* fn = "saip_batch_sensing_chain_set_table_host";
	saip_status st = need_chain(b, fn);
	return st ? st : chain_set_table(sense_chain_kind(), b, b->sensing.chain, table, fn);
}
// a_q and a_dq of both bounds have to be valid words; delay and vel_mode only finite: the draw is rounded to the nearest integer and
// clamped to its range
extern "C" saip_status saip_batch_sensing_chain_randomize(saip_batch* b, unsigned long long seed, long long round, const double* lo, const double* hi) {
	const char* fn = "saip_batch_sensing_chain_randomize";
	saip_status st = need_chain(b, fn);
	if (st || (st = chain_randomize_bounds(sense_chain_kind(), b, b->sensing.chain, lo, hi, fn))) return st;
	const auto& H = b->sensing.chain;
	saip::SenseChainRandomParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.depth = H.depth;
	P.seed_lo = (uint32_t)seed;
	P.seed_hi = (uint32_t)(seed >> 32);
	P.round = (uint32_t)round;
	P.table = H.table;
	P.lo = H.bounds;
	P.hi = H.bounds + (size_t)P.n * saip::SENSE_CHAIN_WORDS;
	hipError_t e = saip::launch_sense_chain_randomize(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "sensing chain randomize launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sensing_chain_reset(saip_batch* b) {
	const char* fn = "saip_batch_sensing_chain_reset";
	saip_status st = need_chain(b, fn);
	if (st || (st = chain_reset(b, b->sensing.chain, fn))) return st;
	b->sensing.epoch = -1;  // the measured copy is the old chain's output: the next read takes the priming sample
	return SAIP_OK;
}
extern "C" double* saip_batch_sensing_chain_table_device(saip_batch* b) { return b ? b->sensing.chain.table : nullptr; }
extern "C" saip_status saip_batch_sensing_chain_state_device(saip_batch* b, double** taps, double** filt, int** primed) {
	saip_status st = need_chain(b, "saip_batch_sensing_chain_state_device");
	return st ? st : chain_state_device(b->sensing.chain, taps, filt, primed);
}
extern "C" saip_status saip_batch_sensing_chain_state_host(saip_batch* b, double* taps, double* filt, int* primed) {
	const char* fn = "saip_batch_sensing_chain_state_host";
	saip_status st = need_chain(b, fn);
	return st ? st : chain_state_host(sense_chain_kind(), b, b->sensing.chain, taps, filt, primed, fn);
}

