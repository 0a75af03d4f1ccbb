#include "saip_engine_internal.h"

// ---- the plant model (saip_plant.hip): actuator limits, friction, joint stops and external wrenches in front of every integration substep
static saip_status need_plant(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->plant.attached) return fail(SAIP_ERR_ORDER, "%s: no plant model is attached (saip_batch_plant_attach)", fn);
	return SAIP_OK;
}
void saip::eng::plant_free(saip_batch* b) {
	auto& C = b->plant;
	chain_free(C.chain);  // the chain goes with its carrier
	for (void* p : {(void*)C.joints, (void*)C.wrenches, (void*)C.tau_act, (void*)C.summary, (void*)C.bounds})
		if (p) (void)hipFree(p);
	C = saip_batch::Plant();
}
static const char* const PLANT_JOINT_WORD_NAMES[saip::PLANT_JOINT_WORDS] = {"gain", "bias", "tau_max", "fv", "fc", "v_s", "q_lo", "q_hi", "k_stop", "c_stop"};
static const char* const PLANT_WRENCH_WORD_NAMES[saip::PLANT_WRENCH_WORDS] = {"F[0]", "F[1]", "F[2]", "M[0]", "M[1]", "M[2]", "p_start", "p_end"};
// a joint table [n][10] (cols = 1) or [n][10][cols]: true when fine, else msg names the joint and the word (and the instance)
static bool plant_check_joints(const double* t, int n, size_t cols, char* msg, size_t len) {
	using namespace saip;
	for (int j = 0; j < n; j++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)j * PLANT_JOINT_WORDS * cols + i;
			char who[64];
			if (cols > 1) snprintf(who, sizeof(who), "joint %d of instance %zu", j, i);
			else snprintf(who, sizeof(who), "joint %d", j);
			for (int k = 0; k < PLANT_JOINT_WORDS; k++) {
				const double v = w[k * cols];
				if (v != v) return snprintf(msg, len, "%s: word %s is NaN", who, PLANT_JOINT_WORD_NAMES[k]), false;
				const bool may_be_infinite = k == PLANT_TAU_MAX || k == PLANT_VS || k == PLANT_Q_LO || k == PLANT_Q_HI;
				if (!may_be_infinite && !std::isfinite(v)) return snprintf(msg, len, "%s: word %s is not finite", who, PLANT_JOINT_WORD_NAMES[k]), false;
				const bool not_negative = k == PLANT_TAU_MAX || k == PLANT_FV || k == PLANT_FC || k == PLANT_K_STOP || k == PLANT_C_STOP;
				if (not_negative && v < 0) return snprintf(msg, len, "%s: word %s = %g is below 0", who, PLANT_JOINT_WORD_NAMES[k], v), false;
			}
			if (w[PLANT_FC * cols] > 0 && !(w[PLANT_VS * cols] > 0)) return snprintf(msg, len, "%s: word v_s = %g must be positive when fc > 0", who, w[PLANT_VS * cols]), false;
			if (w[PLANT_Q_LO * cols] > w[PLANT_Q_HI * cols])
				return snprintf(msg, len, "%s: word q_lo = %g is above q_hi = %g", who, w[PLANT_Q_LO * cols], w[PLANT_Q_HI * cols]), false;
		}
	return true;
}
// a wrench table [W][8] or [W][8][cols]: F and M finite, the window words anything but NaN
static bool plant_check_wrenches(const double* t, int W, size_t cols, char* msg, size_t len) {
	for (int k = 0; k < W; k++)
		for (size_t i = 0; i < cols; i++)
			for (int e = 0; e < saip::PLANT_WRENCH_WORDS; e++) {
				const double v = t[((size_t)k * saip::PLANT_WRENCH_WORDS + e) * cols + i];
				if (v != v || (e < 6 && !std::isfinite(v))) {
					if (cols > 1) snprintf(msg, len, "wrench %d of instance %zu: word %s is not finite", k, i, PLANT_WRENCH_WORD_NAMES[e]);
					else snprintf(msg, len, "wrench %d: word %s is not finite", k, PLANT_WRENCH_WORD_NAMES[e]);
					return false;
				}
			}
	return true;
}
extern "C" saip_status saip_batch_plant_attach(saip_batch* b, const double* joint_table, int per_instance_joints, int n_wrenches, const int* links,
												const double* points, const int* frames, const double* wrench_table, int per_instance_wrenches) {
	const char* fn = "saip_batch_plant_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->plant.attached) return fail(SAIP_ERR_ORDER, "%s: a plant model is already attached (saip_batch_plant_detach first)", fn);
	const int W = n_wrenches, n = b->model->n;
	if (W < 0 || W > saip::PLANT_MAX_WRENCHES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d wrenches required (got %d)", fn, saip::PLANT_MAX_WRENCHES, W);
	if (W > 0 && (!links || !points || !frames || !wrench_table)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links, points, frames or wrench table", fn);
	per_instance_joints = per_instance_joints ? 1 : 0;
	per_instance_wrenches = per_instance_wrenches && W > 0 ? 1 : 0;
	saip::PlantSite site[saip::PLANT_MAX_WRENCHES] = {};
	const int nl = (int)b->model->links.size();
	double I3[9];
	m3_eye(I3);
	for (int k = 0; k < W; k++) {
		if (links[k] < 0 || links[k] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: link index %d out of range (%d links)", fn, k, links[k], nl);
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(points[3 * k + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: the point is not finite", fn, k);
		if (frames[k] != saip::PLANT_FRAME_WORLD && frames[k] != saip::PLANT_FRAME_LINK)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: unknown frame %d (0 world, 1 link)", fn, k, frames[k]);
		// the site composed exactly as saip_batch_model_frames_* composes a frame's point and rotation
		const LinkInfo& L = b->model->links[links[k]];
		double t[3];
		m3_vec(L.R, points + 3 * k, t);
		for (int e = 0; e < 3; e++) site[k].pos[e] = L.p[e] + t[e];
		m3_mul(L.R, I3, site[k].rot);
		site[k].body = L.body;
		site[k].frame = frames[k];
	}
	// the neutral table: gain 1, no offset, no limit, no friction, the model's joint limits as stops of stiffness 0
	const size_t jcols = per_instance_joints ? (size_t)b->B : 1, wcols = per_instance_wrenches ? (size_t)b->B : 1;
	std::vector<double> neutral;
	if (!joint_table) {
		neutral.assign((size_t)n * saip::PLANT_JOINT_WORDS * jcols, 0.0);
		for (int j = 0; j < n; j++) {
			const double lo = b->model->q_lower[j], hi = b->model->q_upper[j];
			const bool limits = lo <= hi;
			for (size_t i = 0; i < jcols; i++) {
				double* w = neutral.data() + (size_t)j * saip::PLANT_JOINT_WORDS * jcols + i;
				w[saip::PLANT_GAIN * jcols] = 1.0;
				w[saip::PLANT_TAU_MAX * jcols] = INFINITY;
				w[saip::PLANT_Q_LO * jcols] = limits ? lo : -INFINITY;
				w[saip::PLANT_Q_HI * jcols] = limits ? hi : INFINITY;
			}
		}
		joint_table = neutral.data();
	}
	char msg[200];
	if (!plant_check_joints(joint_table, n, jcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (W > 0 && !plant_check_wrenches(wrench_table, W, wcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [n][10][ld] doubles: the byte count must fit a size_t
	const size_t widest = (size_t)(n > 4 ? n : 4) * saip::PLANT_JOINT_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->plant;
	C = saip_batch::Plant();
	const size_t ld = b->ld, jrows = (size_t)n * saip::PLANT_JOINT_WORDS, wrows = (size_t)W * saip::PLANT_WRENCH_WORDS;
	if ((st = alloc_zero(b, &C.joints, jrows * (per_instance_joints ? ld : 1))) || (W > 0 && (st = alloc_zero(b, &C.wrenches, wrows * (per_instance_wrenches ? ld : 1)))) ||
		(st = alloc_zero(b, &C.tau_act, (size_t)n * ld)) || (st = alloc_zero(b, &C.summary, (size_t)saip::PLANT_SUMMARY_ROWS * ld)) ||
		((per_instance_joints || per_instance_wrenches) && (st = alloc_zero(b, &C.bounds, 2 * (jrows + wrows)))) ||
		(st = upload_table(b, C.joints, joint_table, jrows, per_instance_joints, "table", fn)) ||
		(W > 0 && (st = upload_table(b, C.wrenches, wrench_table, wrows, per_instance_wrenches, "table", fn)))) {
		plant_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance_joints = per_instance_joints;
	C.n_wrenches = W;
	C.per_instance_wrenches = per_instance_wrenches;
	C.period = 0;
	for (int k = 0; k < W; k++) C.site[k] = site[k];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_detach(saip_batch* b) {
	const char* fn = "saip_batch_plant_detach";
	saip_status st = need_plant(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a plant substep may still be in flight
	plant_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_info(saip_batch* b, int* per_instance_joints, int* n_wrenches, int* per_instance_wrenches, long long* period) {
	saip_status st = need_plant(b, "saip_batch_plant_info");
	if (st) return st;
	const auto& C = b->plant;
	if (per_instance_joints) *per_instance_joints = C.per_instance_joints;
	if (n_wrenches) *n_wrenches = C.n_wrenches;
	if (per_instance_wrenches) *per_instance_wrenches = C.per_instance_wrenches;
	if (period) *period = C.period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_set_joints_host(saip_batch* b, const double* joint_table) {
	const char* fn = "saip_batch_plant_set_joints_host";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	if (!joint_table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null joint table", fn);
	const auto& C = b->plant;
	char msg[200];
	if (!plant_check_joints(joint_table, b->model->n, C.per_instance_joints ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.joints, joint_table, (size_t)b->model->n * saip::PLANT_JOINT_WORDS, C.per_instance_joints, "table", fn);
}
extern "C" saip_status saip_batch_plant_set_wrenches_host(saip_batch* b, const double* wrench_table) {
	const char* fn = "saip_batch_plant_set_wrenches_host";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	const auto& C = b->plant;
	if (C.n_wrenches == 0) return fail(SAIP_ERR_ORDER, "%s: the plant model was attached without wrenches", fn);
	if (!wrench_table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null wrench table", fn);
	char msg[200];
	if (!plant_check_wrenches(wrench_table, C.n_wrenches, C.per_instance_wrenches ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.wrenches, wrench_table, (size_t)C.n_wrenches * saip::PLANT_WRENCH_WORDS, C.per_instance_wrenches, "table", fn);
}
// Per-instance tables drawn on the device between two batch-uniform tables (host pointers: joints [n][10], wrenches [W][8]); a null pair
// leaves that table alone.  Whatever the draw, the tables stay valid: both bounds of every word have to be, and so has every combination
// the two-word conditions can meet (the largest q_lo against the smallest q_hi, the smallest v_s when fc can be positive).
extern "C" saip_status saip_batch_plant_randomize(saip_batch* b, unsigned long long seed, long long round, const double* joint_lo, const double* joint_hi,
												   const double* wrench_lo, const double* wrench_hi) {
	using namespace saip;
	const char* fn = "saip_batch_plant_randomize";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	const auto& C = b->plant;
	const int n = b->model->n, W = C.n_wrenches;
	if ((st = check_bound_pairs(fn, joint_lo, joint_hi, wrench_lo, wrench_hi))) return st;
	if (joint_lo && !C.per_instance_joints) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the joint table is batch-uniform (attach it per instance)", fn);
	if (wrench_lo && (W == 0 || !C.per_instance_wrenches)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the wrench table is batch-uniform or empty (attach it per instance)", fn);
	const size_t jrows = (size_t)n * PLANT_JOINT_WORDS, wrows = (size_t)W * PLANT_WRENCH_WORDS;
	if (joint_lo) {
		if ((st = check_bound_pair(fn, joint_lo, joint_hi, [&](const double* t, char* msg, size_t len) { return plant_check_joints(t, n, 1, msg, len); }))) return st;
		for (int j = 0; j < n; j++) {
			const double *l = joint_lo + (size_t)j * PLANT_JOINT_WORDS, *h = joint_hi + (size_t)j * PLANT_JOINT_WORDS;
			if ((st = check_bound_infinities(fn, "joint", j, l, h, PLANT_JOINT_WORDS, PLANT_JOINT_WORD_NAMES))) return st;
			if (std::max(l[PLANT_Q_LO], h[PLANT_Q_LO]) > std::min(l[PLANT_Q_HI], h[PLANT_Q_HI]))
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: joint %d: the ranges of words q_lo and q_hi overlap", fn, j);
			if (std::max(l[PLANT_FC], h[PLANT_FC]) > 0 && !(std::min(l[PLANT_VS], h[PLANT_VS]) > 0))
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: joint %d: word v_s must be positive over its whole range when fc can be", fn, j);
		}
	}
	if (wrench_lo) {
		if ((st = check_bound_pair(fn, wrench_lo, wrench_hi, [&](const double* t, char* msg, size_t len) { return plant_check_wrenches(t, W, 1, msg, len); }))) return st;
		for (int k = 0; k < W; k++)
			if ((st = check_bound_infinities(fn, "wrench", k, wrench_lo + (size_t)k * PLANT_WRENCH_WORDS, wrench_hi + (size_t)k * PLANT_WRENCH_WORDS, PLANT_WRENCH_WORDS, PLANT_WRENCH_WORD_NAMES)))
				return st;
	}
	if ((st = need_ready(b, fn))) return st;
	PlantRandomParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = n;
	P.n_wrenches = W;
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
	hipError_t e = saip::launch_plant_randomize(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "plant randomize launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_set_period(saip_batch* b, long long period) {
	saip_status st = need_plant(b, "saip_batch_plant_set_period");
	if (st) return st;
	b->plant.period = period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_plant_summary_host";
	const saip_status st = need_plant(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->plant.summary, saip::PLANT_SUMMARY_ROWS, fn);
}
extern "C" saip_status saip_batch_plant_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_plant_summary_reset";
	saip_status st = need_plant(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return zero_rows(b, b->plant.summary, saip::PLANT_SUMMARY_ROWS);
}
extern "C" double* saip_batch_plant_joints_device(saip_batch* b) { return b ? b->plant.joints : nullptr; }
extern "C" double* saip_batch_plant_wrenches_device(saip_batch* b) { return b ? b->plant.wrenches : nullptr; }
extern "C" double* saip_batch_plant_torques_device(saip_batch* b) { return b ? b->plant.tau_act : nullptr; }
extern "C" double* saip_batch_plant_summary_device(saip_batch* b) { return b ? b->plant.summary : nullptr; }
// one launch of the plant kernel at the resident state, in front of an integration substep of length dt
// (substep: its index inside the period; the actuation chain advances its delay line in substep 0 only)
saip_status saip::eng::plant_launch(saip_batch* b, double dt, int substep) {
	const auto& C = b->plant;
	saip::PlantParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.n_wrenches = C.n_wrenches;
	P.per_instance_joints = C.per_instance_joints;
	P.per_instance_wrenches = C.per_instance_wrenches;
	P.period = C.period;
	P.dt = dt;
	P.model = b->model_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau_cmd = commanded_tau(b);
	P.joints = C.joints;
	P.wrenches = C.wrenches;
	P.tau_act = tau_buffer(b, saip::TauBuf::Plant);
	P.summary = C.summary;
	for (int k = 0; k < C.n_wrenches; k++) P.site[k] = C.site[k];
	hipError_t e;
	if (C.chain.attached) {
		// the chain's instantiation in place of the plant's: the same launch, pc_step in front of every pl_joint
		const auto& H = C.chain;
		saip::PlantChainParams Q;
		memset(&Q, 0, sizeof(Q));
		Q.P = P;
		Q.per_instance = H.per_instance;
		Q.depth = H.depth;
		Q.advance = substep == 0 ? 1 : 0;
		Q.table = H.table;
		Q.taps = H.taps;
		Q.filt = H.filt;
		Q.primed = H.primed;
		e = saip::launch_plant_chain_apply(Q, b->model->dev.is_tree != 0, b->stream);
	} else e = saip::launch_plant_apply(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "plant launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}

// ---- the actuation chain (saip_plant_chain.h): delay line, slew-rate limit and first-order lag in front of the plant's joint rows.  The
// host side is saip_engine_chain.cpp's; nothing but the draw's parameters is its own here.
static saip_status need_plant_chain(const saip_batch* b, const char* fn) {
	saip_status st = need_plant(b, fn);
	return st ? st : chain_need(plant_chain_kind(), b->plant.chain, fn);
}
extern "C" saip_status saip_batch_plant_chain_attach(saip_batch* b, const double* table, int per_instance, int depth) {
	const char* fn = "saip_batch_plant_chain_attach";
	saip_status st = chain_attach_depth(plant_chain_kind(), b, depth, fn);
	return st ? st : chain_attach(plant_chain_kind(), b, b->plant.chain, b->plant.attached, table, per_instance, depth, fn);
}
extern "C" saip_status saip_batch_plant_chain_detach(saip_batch* b) {
	const char* fn = "saip_batch_plant_chain_detach";
	saip_status st = need_plant_chain(b, fn);
	return st ? st : chain_detach(b, b->plant.chain, fn);
}
extern "C" saip_status saip_batch_plant_chain_info(saip_batch* b, int* attached, int* per_instance, int* depth, size_t* state_bytes) {
	saip_status st = need_plant(b, "saip_batch_plant_chain_info");
	if (st) return st;
	chain_info(plant_chain_kind(), b, b->plant.chain, attached, per_instance, depth, state_bytes);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_chain_set_table_host(saip_batch* b, const double* table) {
	const char* fn = "saip_batch_plant_chain_set_table_host";
	saip_status st = need_plant_chain(b, fn);
	return st ? st : chain_set_table(plant_chain_kind(), b, b->plant.chain, table, fn);
}
// rate_max and tau_lag of both bounds have to be valid words, an infinite rate_max on both sides or on neither; delay only finite: the
// draw is rounded to the nearest integer and clamped to its range
extern "C" saip_status saip_batch_plant_chain_randomize(saip_batch* b, unsigned long long seed, long long round, const double* lo, const double* hi) {
	const char* fn = "saip_batch_plant_chain_randomize";
	saip_status st = need_plant_chain(b, fn);
	if (st || (st = chain_randomize_bounds(plant_chain_kind(), b, b->plant.chain, lo, hi, fn))) return st;
	const auto& H = b->plant.chain;
	saip::PlantChainRandomParams P;
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
	P.hi = H.bounds + (size_t)P.n * saip::PLANT_CHAIN_WORDS;
	hipError_t e = saip::launch_plant_chain_randomize(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "actuation chain randomize launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_chain_reset(saip_batch* b) {
	const char* fn = "saip_batch_plant_chain_reset";
	saip_status st = need_plant_chain(b, fn);
	return st ? st : chain_reset(b, b->plant.chain, fn);
}
extern "C" double* saip_batch_plant_chain_table_device(saip_batch* b) { return b ? b->plant.chain.table : nullptr; }
extern "C" saip_status saip_batch_plant_chain_state_device(saip_batch* b, double** taps, double** filt, int** primed) {
	saip_status st = need_plant_chain(b, "saip_batch_plant_chain_state_device");
	return st ? st : chain_state_device(b->plant.chain, taps, filt, primed);
}
extern "C" saip_status saip_batch_plant_chain_state_host(saip_batch* b, double* taps, double* filt, int* primed) {
	const char* fn = "saip_batch_plant_chain_state_host";
	saip_status st = need_plant_chain(b, fn);
	return st ? st : chain_state_host(plant_chain_kind(), b, b->plant.chain, taps, filt, primed, fn);
}

