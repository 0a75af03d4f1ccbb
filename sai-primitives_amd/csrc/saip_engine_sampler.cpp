#include "saip_engine_internal.h"

// ---- resident rollout sampler (saip_sampler.hip): perturb the resident keyframes around a nominal plan, one cost per instance from
// the recorder, softmin update of the plan -- the steps of a sampling-MPC round that would otherwise go through the host
static_assert(saip::SAMP_MAXT == SAIP_MAXT && saip::SAMP_SUMMARY_ROWS == saip::REC_SUMMARY_ROWS, "saip_sampler.h restates them");
static_assert(saip::SAMP_MAX_SCENARIOS == SAIP_SAMPLER_MAX_SCENARIOS && saip::SAMP_RISK_MEAN == SAIP_SAMPLER_RISK_MEAN && saip::SAMP_RISK_MAX == SAIP_SAMPLER_RISK_MAX &&
				  saip::SAMP_RISK_CVAR == SAIP_SAMPLER_RISK_CVAR,
			  "saip_sampler.h restates them");
// what the samplers of a batch share: allocated by the first attach, gone with the last detach, and the scenario setting with it
static void sampler_free_shared(saip_batch* b) {
	for (void* p : {(void*)b->samp_cost, (void*)b->samp_w, (void*)b->samp_best_map, (void*)b->samp_result, (void*)b->samp_group})
		if (p) (void)hipFree(p);
	b->samp_cost = b->samp_w = b->samp_group = nullptr;
	b->samp_best_map = nullptr;
	b->samp_result = nullptr;
	b->samp_scenarios = 1;
	b->samp_risk = b->samp_tail = 0;
}
void saip::eng::sampler_release(saip_batch* b, int task) {  // the stream is idle
	if (task >= (int)b->samp.size() || !b->samp[task].attached) return;
	(void)hipFree(b->samp[task].nominal);
	b->samp[task] = saip_batch::Sampler();
	if (--b->n_samp > 0) return;
	sampler_free_shared(b);
}
// any sampler entry: a controller with at least one sampler (task >= 0: that task's)
static saip_status need_sampler(const saip_batch* b, int task, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (b->n_samp == 0 || (task >= 0 && (task >= (int)b->samp.size() || !b->samp[task].attached)))
		return fail(SAIP_ERR_ORDER, "%s: no sampler is attached%s (saip_batch_sampler_attach)", fn, task >= 0 ? " to this task" : "");
	return SAIP_OK;
}
static void sampler_params(const saip_batch* b, saip::SamplerParams& P) {
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.C = b->B / b->samp_scenarios;
	P.seed_lo = (uint32_t)b->samp_seed;
	P.seed_hi = (uint32_t)(b->samp_seed >> 32);
	P.round = (uint32_t)b->samp_round;
	for (int t = 0; t < (int)b->samp.size(); t++) {
		const auto& S = b->samp[t];
		if (!S.attached) continue;
		const auto& H = b->sched[t];
		auto& E = P.e[P.n++];
		E.key = H.key;
		E.nominal = S.nominal;
		E.sigma = S.nominal + (size_t)H.K * H.count;
		E.count = H.count;
		E.K = H.K;
		E.d = S.d;
		E.rot = S.rot;
		E.r_rot = S.r_rot;
		E.task = t;
		E.exempt = S.exempt;
	}
}
extern "C" saip_status saip_batch_sampler_attach(saip_batch* b, int task, const double* sigma, const double* nominal, int exempt) {
	const char* fn = "saip_batch_sampler_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (!sigma) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null sigma", fn);
	const int C = b->B / b->samp_scenarios;  // the candidates; B unless saip_batch_sampler_set_scenarios grouped the batch
	if (exempt < 0 || exempt > C) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: exempt = %d outside 0 .. %d", fn, exempt, C);
	if (task >= (int)b->sched.size() || !b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d has no goal schedule (saip_batch_goal_schedule_attach first)", fn, task);
	if (task < (int)b->samp.size() && b->samp[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d already has a sampler (saip_batch_sampler_detach first)", fn, task);
	const auto& H = b->sched[task];
	if (!H.per_instance) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the schedule of task %d is batch-uniform; a sampler needs per-instance keyframes", fn, task);
	int rot = 0, r_rot = H.count;
	if (b->tasks[task].dev.type == saip::TASK_MOTION_FORCE && H.first < 12 && H.first + H.count > 3) {
		if (H.first > 3 || H.first + H.count < 12)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a sampled schedule must cover all or none of the rotation rows 3..11 (got [%d, %d))", fn, H.first, H.first + H.count);
		rot = 1;
		r_rot = 3 - H.first;
	}
	if (H.count > saip::SAMP_MAX_ROWS)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the schedule of task %d covers %d rows; a sampler takes at most %d", fn, task, H.count, (int)saip::SAMP_MAX_ROWS);
	const int d = rot ? H.count - 6 : H.count;
	for (int j = 0; j < d; j++)
		if (!(sigma[j] >= 0) || !std::isfinite(sigma[j])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sigma[%d] = %g is negative or not finite", fn, j, sigma[j]);
	if (nominal && rot && H.mode == saip::SCHED_LINEAR) {
		const int count = H.count;
		const char* bad = sched_check_rotations(H.K, [&](int k, int e) { return nominal[(size_t)k * count + r_rot + e]; });
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nominal plan: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	const size_t plan = (size_t)H.K * H.count;
	double* dev = nullptr;
	HIP_TRY(hipMalloc((void**)&dev, (plan + d) * sizeof(double)));
	const bool first = b->n_samp == 0;
	hipError_t e = hipSuccess;
	if (first) {
		const size_t ld = b->ld;
		if ((e = hipMalloc((void**)&b->samp_cost, ld * sizeof(double))) == hipSuccess && (e = hipMalloc((void**)&b->samp_w, ld * sizeof(double))) == hipSuccess &&
			(e = hipMalloc((void**)&b->samp_best_map, ld * sizeof(int))) == hipSuccess && (e = hipMalloc((void**)&b->samp_result, sizeof(saip::SamplerResult))) == hipSuccess &&
			(e = hipMalloc((void**)&b->samp_group, ld * sizeof(double))) == hipSuccess && (e = hipMemsetAsync(b->samp_group, 0, ld * sizeof(double), b->stream)) == hipSuccess &&
			(e = hipMemsetAsync(b->samp_cost, 0, ld * sizeof(double), b->stream)) == hipSuccess && (e = hipMemsetAsync(b->samp_w, 0, ld * sizeof(double), b->stream)) == hipSuccess &&
			(e = hipMemsetAsync(b->samp_best_map, 0xff, ld * sizeof(int), b->stream)) == hipSuccess) {  // the map starts at -1: no best yet
			saip::SamplerResult none = {-1, 0, 0.0, 0.0, 0.0};
			e = hipMemcpyAsync(b->samp_result, &none, sizeof(none), hipMemcpyHostToDevice, b->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // `none` is a stack object
		}
	}
	if (e == hipSuccess) {
		if (nominal) e = hipMemcpyAsync(dev, nominal, plan * sizeof(double), hipMemcpyHostToDevice, b->stream);
		else {  // column 0 of the resident keyframes, through the host (an attach waits for the stream anyway)
			std::vector<double> col(plan);
			e = hipMemcpy2DAsync(col.data(), sizeof(double), H.key, (size_t)b->ld * sizeof(double), sizeof(double), plan, hipMemcpyDeviceToHost, b->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
			if (e == hipSuccess) e = hipMemcpy(dev, col.data(), plan * sizeof(double), hipMemcpyHostToDevice);
		}
	}
	if (e == hipSuccess) e = hipMemcpyAsync(dev + plan, sigma, (size_t)d * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffers may be reused by the caller right away
	if (e != hipSuccess) {
		(void)hipFree(dev);
		if (first) sampler_free_shared(b);
		return fail(SAIP_ERR_DEVICE, "%s: upload failed: %s", fn, hipGetErrorString(e));
	}
	if (b->samp.size() < b->tasks.size()) b->samp.resize(b->tasks.size());
	auto& S = b->samp[task];
	S.attached = true;
	S.d = d;
	S.rot = rot;
	S.r_rot = r_rot;
	S.exempt = exempt;
	S.nominal = dev;
	b->n_samp++;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_sampler_detach";
	if (task < -1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a sampler launch may still be in flight
	for (int t = (int)b->samp.size() - 1; t >= 0; t--)
		if (task == -1 || t == task) sampler_release(b, t);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_seed(saip_batch* b, unsigned long long seed) {
	saip_status st = need_sampler(b, -1, "saip_batch_sampler_seed");
	if (st) return st;
	b->samp_seed = seed;
	b->samp_round = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_perturb(saip_batch* b) {
	const char* fn = "saip_batch_sampler_perturb";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = saip::launch_sampler_perturb(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	b->samp_round++;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_cost(saip_batch* b, const double* w_summary, const double* target, double w_path, double w_final) {
	const char* fn = "saip_batch_sampler_cost";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	const auto& R = b->rec;
	saip::SamplerCostParams P;
	memset(&P, 0, sizeof(P));
	bool any_w = false;
	for (int r = 0; w_summary && r < saip::REC_SUMMARY_ROWS; r++) {
		P.w[r] = w_summary[r];
		any_w = any_w || w_summary[r] != 0.0;
	}
	if (any_w && !(R.attached && R.summary)) return fail(SAIP_ERR_ORDER, "%s: a summary weight is set but no recorder keeps summaries (saip_batch_rollout_recorder_attach)", fn);
	if (target) {
		if (!R.attached || !(R.channels & saip::REC_POSE)) return fail(SAIP_ERR_ORDER, "%s: a target needs the recorder's POSE channel", fn);
		const long long taken = R.period / R.stride;
		if (taken < 1) return fail(SAIP_ERR_ORDER, "%s: a target needs at least one recorded sample", fn);
		const long long n = taken < R.capacity ? taken : R.capacity;
		const int dof = b->model->n;
		P.log = R.log;
		P.rows = R.rows;
		P.pose_row0 = ((R.channels & saip::REC_Q) ? dof : 0) + ((R.channels & saip::REC_DQ) ? dof : 0) + ((R.channels & saip::REC_TAU) ? dof : 0);
		P.capacity = R.capacity;
		P.first_slot = (int)((taken - n) % R.capacity);  // the ring in chronological order, as saip_batch_rollout_log_host reads it
		P.n_samples = (int)n;
		P.has_target = 1;
		for (int i = 0; i < 3; i++) P.target[i] = target[i];
		P.w_path = w_path;
		P.w_final = w_final;
	}
	if ((st = need_ready(b, fn))) return st;
	P.B = b->B;
	P.ld = b->ld;
	P.summary = any_w ? R.summary : nullptr;
	P.cost = b->samp_cost;
	hipError_t e = saip::launch_sampler_cost(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_set_cost_host(saip_batch* b, const double* cost) {
	const char* fn = "saip_batch_sampler_set_cost_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (!cost) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null cost", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_h2d(b, b->samp_cost, cost, 1);
}
extern "C" saip_status saip_batch_sampler_get_cost_host(saip_batch* b, double* cost) {
	const char* fn = "saip_batch_sampler_get_cost_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (!cost) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, cost, b->samp_cost, 1);
}
extern "C" double* saip_batch_sampler_cost_device(saip_batch* b) { return b ? b->samp_cost : nullptr; }
extern "C" const int* saip_batch_sampler_best_map_device(saip_batch* b) { return b ? b->samp_best_map : nullptr; }
extern "C" saip_status saip_batch_sampler_update(saip_batch* b, double temperature) {
	const char* fn = "saip_batch_sampler_update";
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!(temperature > 0) || !std::isfinite(temperature)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: temperature = %g: a finite value > 0 is required", fn, temperature);
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = b->samp_scenarios == 1 ? saip::launch_sampler_update(P, b->samp_cost, temperature, b->samp_w, b->samp_result, b->samp_best_map, b->stream)
										  : saip::launch_sampler_update_grouped(P, b->samp_cost, b->samp_risk, b->samp_tail, b->samp_group, temperature, b->samp_w, b->samp_result,
																				b->samp_best_map, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_shift(saip_batch* b, int n) {
	const char* fn = "saip_batch_sampler_shift";
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (n < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n = %d is negative", fn, n);
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (n == 0) return SAIP_OK;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = saip::launch_sampler_shift(P, n, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_result_host(saip_batch* b, int* best, int* n_valid, double* min_cost, double* sum_w, double* ess) {
	const char* fn = "saip_batch_sampler_result_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerResult r;
	HIP_TRY(hipMemcpyAsync(&r, b->samp_result, sizeof(r), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (best) *best = r.best;
	if (n_valid) *n_valid = r.n_valid;
	if (min_cost) *min_cost = r.min_cost;
	if (sum_w) *sum_w = r.sum_w;
	if (ess) *ess = r.ess;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_get_nominal_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_sampler_get_nominal_host";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemcpyAsync(out, b->samp[task].nominal, (size_t)b->sched[task].K * b->sched[task].count * sizeof(double), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_set_nominal_host(saip_batch* b, int task, const double* in) {
	const char* fn = "saip_batch_sampler_set_nominal_host";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (!in) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null nominal plan", fn);
	if (b->samp[task].rot && b->sched[task].mode == saip::SCHED_LINEAR) {  // as _attach checks it
		const int count = b->sched[task].count, r_rot = b->samp[task].r_rot;
		const char* bad = sched_check_rotations(b->sched[task].K, [&](int k, int e) { return in[(size_t)k * count + r_rot + e]; });
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nominal plan: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemcpyAsync(b->samp[task].nominal, in, (size_t)b->sched[task].K * b->sched[task].count * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the host buffer may be reused by the caller right away
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_info(saip_batch* b, int task, int* d, int* exempt, unsigned long long* seed, long long* round) {
	const char* fn = "saip_batch_sampler_info";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (d) *d = b->samp[task].d;
	if (exempt) *exempt = b->samp[task].exempt;
	if (seed) *seed = b->samp_seed;
	if (round) *round = b->samp_round;
	return SAIP_OK;
}
// ---- scenario groups: B = C M instances as C candidate plans rolled out in M scenarios each (saip.h)
extern "C" saip_status saip_batch_sampler_set_scenarios(saip_batch* b, int n_scenarios, int risk, int tail) {
	const char* fn = "saip_batch_sampler_set_scenarios";
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (n_scenarios < 1 || n_scenarios > SAIP_SAMPLER_MAX_SCENARIOS)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_scenarios = %d outside 1 .. %d", fn, n_scenarios, SAIP_SAMPLER_MAX_SCENARIOS);
	if (risk != SAIP_SAMPLER_RISK_MEAN && risk != SAIP_SAMPLER_RISK_MAX && risk != SAIP_SAMPLER_RISK_CVAR)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown risk measure %d (SAIP_SAMPLER_RISK_MEAN, _MAX or _CVAR)", fn, risk);
	if (risk == SAIP_SAMPLER_RISK_CVAR ? (tail < 1 || tail > n_scenarios) : tail != 0)
		return risk == SAIP_SAMPLER_RISK_CVAR ? fail(SAIP_ERR_INVALID_ARGUMENT, "%s: tail = %d outside 1 .. %d (the scenarios)", fn, tail, n_scenarios)
											  : fail(SAIP_ERR_INVALID_ARGUMENT, "%s: tail = %d must be 0 unless the risk measure is SAIP_SAMPLER_RISK_CVAR", fn, tail);
	if (b->B % n_scenarios != 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the batch of %d instances is no multiple of n_scenarios = %d", fn, b->B, n_scenarios);
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	const int C = b->B / n_scenarios;
	for (int t = 0; t < (int)b->samp.size(); t++)
		if (b->samp[t].attached && b->samp[t].exempt > C)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the sampler of task %d has exempt = %d, more than the %d candidates of %d scenarios", fn, t, b->samp[t].exempt, C, n_scenarios);
	b->samp_scenarios = n_scenarios;
	b->samp_risk = risk;
	b->samp_tail = tail;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_scenarios_info(saip_batch* b, int* n_scenarios, int* n_candidates, int* risk, int* tail) {
	saip_status st = need_sampler(b, -1, "saip_batch_sampler_scenarios_info");
	if (st) return st;
	if (n_scenarios) *n_scenarios = b->samp_scenarios;
	if (n_candidates) *n_candidates = b->B / b->samp_scenarios;
	if (risk) *risk = b->samp_risk;
	if (tail) *tail = b->samp_tail;
	return SAIP_OK;
}
extern "C" const double* saip_batch_sampler_weights_device(saip_batch* b) { return b ? b->samp_w : nullptr; }
// with M = 1 the group cost is the cost array itself: no launch forms a copy
extern "C" double* saip_batch_sampler_group_cost_device(saip_batch* b) { return !b ? nullptr : b->samp_scenarios == 1 ? b->samp_cost : b->samp_group; }
extern "C" saip_status saip_batch_sampler_get_group_cost_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_sampler_get_group_cost_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemcpyAsync(out, saip_batch_sampler_group_cost_device(b), (size_t)(b->B / b->samp_scenarios) * sizeof(double), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_share_scenario_tables(saip_batch* b, int* n_arrays) {
	const char* fn = "saip_batch_sampler_share_scenario_tables";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (b->samp_scenarios == 1) return fail(SAIP_ERR_ORDER, "%s: the batch has one scenario (saip_batch_sampler_set_scenarios first)", fn);
	if ((st = need_ready(b, fn))) return st;
	// every resident per-instance table a _randomize entry can fill, as (array, rows of [ld]); the inertia rows last: composed per column
	const int n = b->model->n;
	const auto& P = b->plant;
	const auto& I = b->inertia;
	const auto& S = b->sensing;
	const struct {
		double* a;
		int rows;
	} tables[] = {
		{P.attached && P.per_instance_joints ? P.joints : nullptr, n * saip::PLANT_JOINT_WORDS},
		{P.attached && P.per_instance_wrenches ? P.wrenches : nullptr, P.n_wrenches * saip::PLANT_WRENCH_WORDS},
		{P.chain.attached && P.chain.per_instance ? P.chain.table : nullptr, n * plant_chain_kind().words},
		{I.attached && I.per_instance ? I.parts : nullptr, n * saip::INERTIA_BODY_WORDS + I.n_payloads * saip::INERTIA_PAYLOAD_WORDS},
		{I.attached && I.per_instance ? I.rows : nullptr, n * saip::INERTIA_ROW_WORDS},
		{S.attached && S.per_instance_joints ? S.joints : nullptr, n * saip::SENSE_JOINT_WORDS},
		{S.attached && S.per_instance_wrenches ? S.wrenches : nullptr, S.n_wrench_tasks * saip::SENSE_WRENCH_WORDS},
		{S.chain.attached && S.chain.per_instance ? S.chain.table : nullptr, n * sense_chain_kind().words},
	};
	int count = 0;
	for (const auto& T : tables) {
		if (!T.a || T.rows == 0) continue;
		hipError_t e = saip::launch_sampler_share_columns(T.a, T.rows, b->B, b->ld, b->B / b->samp_scenarios, b->stream);
		if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
		count++;
	}
	if (S.attached) b->sensing.epoch = -1;  // the measured copy was taken under the old tables, as after saip_batch_sensing_randomize
	if (n_arrays) *n_arrays = count;
	return SAIP_OK;
}
