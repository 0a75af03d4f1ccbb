#include "saip_engine_internal.h"

// ---- the clearance monitor (saip_clearance.hip): link spheres against world-fixed obstacles and against each other
static saip_status need_clearance(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->clearance.attached) return fail(SAIP_ERR_ORDER, "%s: no clearance monitor is attached (saip_batch_clearance_attach)", fn);
	return SAIP_OK;
}
void saip::eng::clearance_free(saip_batch* b) {
	auto& C = b->clearance;
	env_release(b, saip::ENV_TARGET_OBSTACLES, -1);  // an environment schedule writes into the obstacles: it goes first
	for (void* p : {(void*)C.geom_dev, (void*)C.obst, (void*)C.readout, (void*)C.summary, (void*)C.centres})
		if (p) (void)hipFree(p);
	C = saip_batch::Clearance();
}
// the obstacle table [O][8] or [O][8][B]; false: `msg` says what is wrong with which entry
bool saip::eng::clearance_check_obstacles(const double* obst, int O, size_t cols, char* msg, size_t len) {
	for (int o = 0; o < O; o++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = obst + (size_t)o * saip::CLEARANCE_OBSTACLE_WORDS * cols + i;
			char where[48] = "";
			if (cols > 1) snprintf(where, sizeof(where), " of instance %zu", i);
			for (int k = 0; k < saip::CLEARANCE_OBSTACLE_WORDS; k++)
				if (!std::isfinite(w[k * cols])) return snprintf(msg, len, "obstacle %d%s: word %d is not finite", o, where, k), false;
			if (w[0] == (double)saip::CLEARANCE_CAPSULE) {
				if (w[7 * cols] < 0) return snprintf(msg, len, "obstacle %d%s: radius %g below 0", o, where, w[7 * cols]), false;
			} else if (w[0] == (double)saip::CLEARANCE_HALF_SPACE) {
				const double nn = std::sqrt(w[cols] * w[cols] + w[2 * cols] * w[2 * cols] + w[3 * cols] * w[3 * cols]);
				if (!(std::fabs(nn - 1.0) <= 1e-6)) return snprintf(msg, len, "obstacle %d%s: the half-space normal has length %.9g, not 1", o, where, nn), false;
			} else {
				return snprintf(msg, len, "obstacle %d%s: unknown kind %g (0 capsule, 1 half-space)", o, where, w[0]), false;
			}
		}
	return true;
}
extern "C" saip_status saip_batch_clearance_attach(saip_batch* b, int n_spheres, const int* links, const double* centres, const double* radii,
												   int n_obstacles, const double* obstacles, int per_instance, int n_pairs, const int* pairs, double margin,
												   int keep_centres) {
	const char* fn = "saip_batch_clearance_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->clearance.attached) return fail(SAIP_ERR_ORDER, "%s: a clearance monitor is already attached (saip_batch_clearance_detach first)", fn);
	const int S = n_spheres, O = n_obstacles, NP = n_pairs;
	if (S < 1 || S > saip::CLEARANCE_MAX_SPHERES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d spheres required (got %d)", fn, saip::CLEARANCE_MAX_SPHERES, S);
	if (O < 0 || O > saip::CLEARANCE_MAX_OBSTACLES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d obstacles required (got %d)", fn, saip::CLEARANCE_MAX_OBSTACLES, O);
	if (NP < 0 || NP > saip::CLEARANCE_MAX_PAIRS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d pairs required (got %d)", fn, saip::CLEARANCE_MAX_PAIRS, NP);
	if (O == 0 && NP == 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to measure against: 0 obstacles and 0 pairs", fn);
	if (!links || !centres || !radii) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links, centres or radii", fn);
	if (O > 0 && !obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	if (NP > 0 && !pairs) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null pairs", fn);
	if (!(margin >= 0) || !std::isfinite(margin)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: margin %g is negative or not finite", fn, margin);
	per_instance = per_instance ? 1 : 0;
	keep_centres = keep_centres ? 1 : 0;
	const int nl = (int)b->model->links.size();
	for (int s = 0; s < S; s++) {
		if (links[s] < 0 || links[s] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: link index %d out of range (%d links)", fn, s, links[s], nl);
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(centres[3 * s + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the centre is not finite", fn, s);
		if (!std::isfinite(radii[s])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the radius is not finite", fn, s);
		if (radii[s] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: radius %g below 0", fn, s, radii[s]);
	}
	for (int p = 0; p < NP; p++) {
		const int s1 = pairs[2 * p], s2 = pairs[2 * p + 1];
		if (s1 < 0 || s1 >= S || s2 < 0 || s2 >= S) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: pair %d: sphere index (%d, %d) out of range (%d spheres)", fn, p, s1, s2, S);
		if (s1 == s2) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: pair %d: sphere %d against itself", fn, p, s1);
	}
	char msg[160];
	if (!clearance_check_obstacles(obstacles, O, per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [O][8][ld], [3 S][ld] doubles: the byte counts must fit a size_t
	const size_t widest = (size_t)saip::CLEARANCE_MAX_OBSTACLES * saip::CLEARANCE_OBSTACLE_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->clearance;
	C = saip_batch::Clearance();
	saip::ClearanceGeom& G = C.geom;
	memset(&G, 0, sizeof(G));
	G.S = S;
	G.O = O;
	G.P = NP;
	// the spheres sorted by body (stable), their constants composed exactly as saip_batch_model_frames_* composes a frame's point, so that a
	// centre differs from that query's position by the contraction of the walk alone
	int order[saip::CLEARANCE_MAX_SPHERES];
	for (int s = 0; s < S; s++) order[s] = s;
	for (int i = 1; i < S; i++)
		for (int k = i; k > 0 && b->model->links[links[order[k - 1]]].body > b->model->links[links[order[k]]].body; k--) std::swap(order[k - 1], order[k]);
	for (int i = 0; i < S; i++) {
		const int s = order[i];
		const LinkInfo& L = b->model->links[links[s]];
		double t[3];
		m3_vec(L.R, centres + 3 * s, t);
		for (int e = 0; e < 3; e++) G.r[i][e] = L.p[e] + t[e];
		G.body[i] = L.body;
		G.slot[i] = s;
		G.radius[s] = radii[s];
	}
	for (int p = 0; p < NP; p++) {
		G.pair[p][0] = (uint8_t)pairs[2 * p];
		G.pair[p][1] = (uint8_t)pairs[2 * p + 1];
	}
	auto alloc_zero = [&](double** p, size_t count) -> saip_status {
		HIP_TRY(hipMalloc((void**)p, count * sizeof(double)));
		HIP_TRY(hipMemsetAsync(*p, 0, count * sizeof(double), b->stream));
		return SAIP_OK;
	};
	auto upload_geom = [&]() -> saip_status {
		HIP_TRY(hipMalloc((void**)&C.geom_dev, sizeof(G)));
		HIP_TRY(hipMemcpyAsync(C.geom_dev, &G, sizeof(G), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
		return SAIP_OK;
	};
	auto reset = [&]() -> saip_status {
		HIP_TRY(saip::launch_clearance_summary_reset(b->B, b->ld, C.summary, b->stream));
		return SAIP_OK;
	};
	const size_t ld = b->ld, rows = (size_t)O * saip::CLEARANCE_OBSTACLE_WORDS;
	if ((st = upload_geom()) || (O > 0 && (st = alloc_zero(&C.obst, rows * (per_instance ? ld : 1)))) ||
		(st = alloc_zero(&C.readout, (size_t)saip::CLEARANCE_READOUT_ROWS * ld)) || (st = alloc_zero(&C.summary, (size_t)saip::CLEARANCE_SUMMARY_ROWS * ld)) ||
		(keep_centres && (st = alloc_zero(&C.centres, (size_t)3 * S * ld))) || (O > 0 && (st = upload_table(b, C.obst, obstacles, rows, per_instance, "obstacle", fn))) ||
		(st = reset())) {
		clearance_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance = per_instance;
	C.keep_centres = keep_centres;
	C.margin = margin;
	C.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_detach(saip_batch* b) {
	const char* fn = "saip_batch_clearance_detach";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a launch may still be in flight
	clearance_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_info(saip_batch* b, int* n_spheres, int* n_obstacles, int* per_instance, int* n_pairs, double* margin,
												 int* keep_centres, long long* period) {
	saip_status st = need_clearance(b, "saip_batch_clearance_info");
	if (st) return st;
	const auto& C = b->clearance;
	if (n_spheres) *n_spheres = C.geom.S;
	if (n_obstacles) *n_obstacles = C.geom.O;
	if (per_instance) *per_instance = C.per_instance;
	if (n_pairs) *n_pairs = C.geom.P;
	if (margin) *margin = C.margin;
	if (keep_centres) *keep_centres = C.keep_centres;
	if (period) *period = C.period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_set_obstacles_host(saip_batch* b, const double* obstacles) {
	const char* fn = "saip_batch_clearance_set_obstacles_host";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	const auto& C = b->clearance;
	if (C.geom.O == 0) return fail(SAIP_ERR_ORDER, "%s: the monitor was attached without obstacles", fn);
	if (!obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	if (env_slot(b, saip::ENV_TARGET_OBSTACLES, -1) >= 0)
		return fail(SAIP_ERR_ORDER, "%s: the obstacles are written by an environment schedule (saip_batch_env_schedule_detach first)", fn);
	char msg[160];
	if (!clearance_check_obstacles(obstacles, C.geom.O, C.per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.obst, obstacles, (size_t)C.geom.O * saip::CLEARANCE_OBSTACLE_WORDS, C.per_instance, "obstacle", fn);
}
extern "C" double* saip_batch_clearance_obstacles_device(saip_batch* b) { return b ? b->clearance.obst : nullptr; }
extern "C" double* saip_batch_clearance_readout_device(saip_batch* b) { return b ? b->clearance.readout : nullptr; }
extern "C" double* saip_batch_clearance_summary_device(saip_batch* b) { return b ? b->clearance.summary : nullptr; }
extern "C" double* saip_batch_clearance_centres_device(saip_batch* b) { return b ? b->clearance.centres : nullptr; }
// one launch of the clearance kernel at the resident state; MONITOR takes the next period index from the host counter (as the goal schedules do)
saip_status saip::eng::clearance_launch(saip_batch* b, int mode, double dt) {
	auto& C = b->clearance;
	saip::ClearanceParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.per_instance = C.per_instance;
	P.dt = dt;
	P.period = mode == saip::CLEARANCE_MONITOR ? (double)C.period++ : 0.0;
	P.margin = C.margin;
	P.model = b->model_dev;
	P.geom = C.geom_dev;
	P.q = b->q;
	P.obst = C.obst;
	P.readout = C.readout;
	P.summary = C.summary;
	P.centres = C.centres;
	hipError_t e = saip::launch_clearance_eval(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "clearance launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_evaluate(saip_batch* b) {
	const char* fn = "saip_batch_clearance_evaluate";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return clearance_launch(b, saip::CLEARANCE_EVALUATE, 0.0);
}
extern "C" saip_status saip_batch_clearance_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_clearance_readout_host";
	const saip_status st = need_clearance(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->clearance.readout, saip::CLEARANCE_READOUT_ROWS, fn);
}
extern "C" saip_status saip_batch_clearance_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_clearance_summary_host";
	const saip_status st = need_clearance(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->clearance.summary, saip::CLEARANCE_SUMMARY_ROWS, fn);
}
// row 0 to +inf, row 3 to -1 (a memset cannot), the period counter to 0
extern "C" saip_status saip_batch_clearance_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_clearance_summary_reset";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_clearance_summary_reset(b->B, b->ld, b->clearance.summary, b->stream));
	b->clearance.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_add_cost(saip_batch* b, double w_penalty, double w_collision, double d_safe) {
	const char* fn = "saip_batch_clearance_add_cost";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	if (b->n_samp == 0) return fail(SAIP_ERR_ORDER, "%s: no sampler is attached (saip_batch_sampler_attach): there is no cost to add to", fn);
	if (w_penalty != w_penalty || w_collision != w_collision || d_safe != d_safe) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a weight or d_safe is NaN", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_clearance_add_cost(b->B, b->ld, b->clearance.summary, b->samp_cost, w_penalty, w_collision, d_safe, b->stream));
	return SAIP_OK;
}
