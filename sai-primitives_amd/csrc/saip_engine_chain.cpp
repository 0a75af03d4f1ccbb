#include "saip_engine_internal.h"

// ---- the host side of the sensing chain and of the actuation chain: one implementation over saip_batch::Chain, and a ChainKind for what
// differs.  The chain's state (taps, filt, primed) is on the snapshot directory while attached (saip_engine_snapshot.cpp).
static const char* chain_delay_rule(double v, const char* name, int depth, bool bounds, char* buf, size_t len) {
	if (bounds || (v == std::floor(v) && v >= 0 && v <= depth)) return nullptr;
	return snprintf(buf, len, "word %s = %g is not an integer in 0..%d", name, v, depth), buf;
}
// delay an integer in 0..depth, vel_mode 0 or 1 (a draw rounds and clamps both), a_q and a_dq in [0, 1]
static const char* sense_chain_rule(int k, double v, const char* name, int depth, bool bounds, char* buf, size_t len) {
	if (!std::isfinite(v)) return snprintf(buf, len, "word %s is not finite", name), buf;
	if (k == saip::SENSE_CHAIN_DELAY) return chain_delay_rule(v, name, depth, bounds, buf, len);
	if (k == saip::SENSE_CHAIN_VEL_MODE) return bounds || v == 0.0 || v == 1.0 ? nullptr : (snprintf(buf, len, "word %s = %g is neither 0 nor 1", name, v), buf);
	return v < 0 || v > 1 ? (snprintf(buf, len, "word %s = %g is outside [0, 1]", name, v), buf) : nullptr;
}
// delay as above, rate_max above 0 and possibly infinite, tau_lag not negative
static const char* plant_chain_rule(int k, double v, const char* name, int depth, bool bounds, char* buf, size_t len) {
	if (k != saip::PLANT_CHAIN_RATE_MAX && !std::isfinite(v)) return snprintf(buf, len, "word %s is not finite", name), buf;
	if (k == saip::PLANT_CHAIN_DELAY) return chain_delay_rule(v, name, depth, bounds, buf, len);
	if (k == saip::PLANT_CHAIN_RATE_MAX) return v > 0 ? nullptr : (snprintf(buf, len, "word %s = %g is not above 0", name, v), buf);
	return v < 0 ? (snprintf(buf, len, "word %s = %g is below 0", name, v), buf) : nullptr;
}
static const char* const SENSE_CHAIN_WORD_NAMES[saip::SENSE_CHAIN_WORDS] = {"delay", "vel_mode", "a_q", "a_dq"};
static const char* const PLANT_CHAIN_WORD_NAMES[saip::PLANT_CHAIN_WORDS] = {"delay", "rate_max", "tau_lag"};
static const double SENSE_CHAIN_NEUTRAL[saip::SENSE_CHAIN_WORDS] = {0, 0, 0, 0};
static const double PLANT_CHAIN_NEUTRAL[saip::PLANT_CHAIN_WORDS] = {0, INFINITY, 0};
// the sensing chain's draw has no scan for a bound infinite on one side only: no word of it may be infinite, its checker refuses that first
const ChainKind& saip::eng::sense_chain_kind() {
	static const ChainKind K = {saip::SENSE_CHAIN_WORDS, saip::SENSE_CHAIN_FILT_ROWS, 2, saip::SENSE_CHAIN_MAX_DEPTH, SENSE_CHAIN_WORD_NAMES, SENSE_CHAIN_NEUTRAL,
								"a", "sensing chain", "saip_batch_sensing_chain", "sensing model", "saip_batch_sensing_attach; an all-zero table is a valid carrier",
								"sense.chain", false, sense_chain_rule};
	return K;
}
const ChainKind& saip::eng::plant_chain_kind() {
	static const ChainKind K = {saip::PLANT_CHAIN_WORDS, saip::PLANT_CHAIN_FILT_ROWS, 1, saip::PLANT_CHAIN_MAX_DEPTH, PLANT_CHAIN_WORD_NAMES, PLANT_CHAIN_NEUTRAL,
								"an", "actuation chain", "saip_batch_plant_chain", "plant model", "saip_batch_plant_attach; an all-neutral table is a valid carrier",
								"plant.chain", true, plant_chain_rule};
	return K;
}

void saip::eng::chain_free(Chain& H) {
	for (void* p : {(void*)H.table, (void*)H.taps, (void*)H.filt, (void*)H.primed, (void*)H.bounds})
		if (p) (void)hipFree(p);
	H = Chain();
}
// a chain table [n][W] (cols = 1) or [n][W][cols]: true when fine, else msg names the joint and the word (and the instance)
static bool chain_check_table(const ChainKind& K, const double* t, int n, size_t cols, int depth, bool bounds, char* msg, size_t len) {
	char buf[96];
	for (int j = 0; j < n; j++)
		for (size_t i = 0; i < cols; i++)
			for (int k = 0; k < K.words; k++) {
				const double v = t[((size_t)j * K.words + k) * cols + i];
				const char* bad = v != v ? (snprintf(buf, sizeof(buf), "word %s is NaN", K.names[k]), buf) : K.rule(k, v, K.names[k], depth, bounds, buf, sizeof(buf));
				if (!bad) continue;
				if (cols > 1) snprintf(msg, len, "joint %d of instance %zu: %s", j, i, bad);
				else snprintf(msg, len, "joint %d: %s", j, bad);
				return false;
			}
	return true;
}
static size_t chain_state_bytes(const ChainKind& K, const saip_batch* b, int depth) {
	const size_t n = b->model->n, ld = b->ld;
	return ((size_t)K.tap_rows * depth * n + K.filt_rows * n) * ld * sizeof(double) + n * ld * sizeof(int);
}
saip_status saip::eng::chain_need(const ChainKind& K, const Chain& H, const char* fn) {
	if (!H.attached) return fail(SAIP_ERR_ORDER, "%s: no %s is attached (%s_attach)", fn, K.noun, K.entry);
	return SAIP_OK;
}
// attach: the arguments first (nothing there needs the carrier or the device), then the call order.  In two halves, so that a carrier
// can check an argument of its own in between
saip_status saip::eng::chain_attach_depth(const ChainKind& K, const saip_batch* b, int depth, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (depth < 0 || depth > K.max_depth) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a depth of 0..%d required (got %d)", fn, K.max_depth, depth);
	return SAIP_OK;
}
saip_status saip::eng::chain_attach(const ChainKind& K, saip_batch* b, Chain& H, bool carrier_attached, const double* table, int per_instance, int depth, const char* fn) {
	const int n = b->model->n;
	per_instance = per_instance ? 1 : 0;
	const size_t cols = per_instance ? (size_t)b->B : 1;
	std::vector<double> neutral;
	if (!table) {
		neutral.resize((size_t)n * K.words * cols);
		for (size_t r = 0; r < (size_t)n * K.words; r++)
			for (size_t i = 0; i < cols; i++) neutral[r * cols + i] = K.neutral[r % K.words];
		table = neutral.data();
	}
	char msg[200];
	if (!chain_check_table(K, table, n, cols, depth, false, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (!carrier_attached) return fail(SAIP_ERR_ORDER, "%s: no %s is attached (%s)", fn, K.carrier, K.carrier_hint);
	if (H.attached) return fail(SAIP_ERR_ORDER, "%s: %s %s is already attached (%s_detach first)", fn, K.article, K.noun, K.entry);
	saip_status st = need_ready(b, fn);
	if (st) return st;
	H = Chain();
	const size_t ld = b->ld, rows = (size_t)n * K.words;
	if ((st = alloc_zero(b, &H.table, rows * (per_instance ? ld : 1))) || (depth > 0 && (st = alloc_zero(b, &H.taps, (size_t)K.tap_rows * depth * n * ld))) ||
		(st = alloc_zero(b, &H.filt, (size_t)K.filt_rows * n * ld)) || (st = alloc_zero(b, &H.primed, (size_t)n * ld)) ||
		(per_instance && (st = alloc_zero(b, &H.bounds, 2 * rows))) || (st = upload_table(b, H.table, table, rows, per_instance, "table", fn))) {
		chain_free(H);
		return st;
	}
	H.attached = true;
	H.per_instance = per_instance;
	H.depth = depth;
	return SAIP_OK;
}
saip_status saip::eng::chain_detach(saip_batch* b, Chain& H, const char* fn) {
	saip_status st = need_ready(b, fn);
	if (st) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a launch that writes the chain's state may still be in flight
	chain_free(H);
	return SAIP_OK;
}
void saip::eng::chain_info(const ChainKind& K, const saip_batch* b, const Chain& H, int* attached, int* per_instance, int* depth, size_t* state_bytes) {
	if (attached) *attached = H.attached ? 1 : 0;
	if (per_instance) *per_instance = H.per_instance;
	if (depth) *depth = H.depth;
	if (state_bytes) *state_bytes = H.attached ? chain_state_bytes(K, b, H.depth) : 0;
}
saip_status saip::eng::chain_set_table(const ChainKind& K, saip_batch* b, Chain& H, const double* table, const char* fn) {
	if (!table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null table", fn);
	char msg[200];
	if (!chain_check_table(K, table, b->model->n, H.per_instance ? (size_t)b->B : 1, H.depth, false, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	saip_status st = need_ready(b, fn);
	if (st) return st;
	// the state stays: the next launch runs the new words over the history there is (the chain's _reset starts afresh)
	return upload_table(b, H.table, table, (size_t)b->model->n * K.words, H.per_instance, "table", fn);
}
// The per-instance table is drawn on the device between two batch-uniform tables [n][W] (host pointers): both checked as bounds and
// uploaded to H.bounds, lo then hi.  The carrier's entry launches the draw.
saip_status saip::eng::chain_randomize_bounds(const ChainKind& K, saip_batch* b, Chain& H, const double* lo, const double* hi, const char* fn) {
	const int n = b->model->n;
	if (!lo || !hi) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null bounds", fn);
	if (!H.per_instance) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the chain table is batch-uniform (attach it per instance)", fn);
	saip_status st = check_bound_pair(fn, lo, hi, [&](const double* t, char* msg, size_t len) { return chain_check_table(K, t, n, 1, H.depth, true, msg, len); });
	for (int j = 0; !st && K.scan_infinities && j < n; j++) st = check_bound_infinities(fn, "joint", j, lo + (size_t)j * K.words, hi + (size_t)j * K.words, K.words, K.names);
	if (st || (st = need_ready(b, fn))) return st;
	return upload_bound_pair(b, H.bounds, lo, hi, (size_t)n * K.words, fn);
}
// primed cleared on the stream, without a synchronisation: the next launch primes every (joint, instance) again
saip_status saip::eng::chain_reset(saip_batch* b, Chain& H, const char* fn) {
	saip_status st = need_ready(b, fn);
	if (st) return st;
	HIP_TRY(hipMemsetAsync(H.primed, 0, (size_t)b->model->n * b->ld * sizeof(int), b->stream));
	return SAIP_OK;
}
// the state arrays themselves, [rows][ld] (taps null at depth 0); any output may be null
saip_status saip::eng::chain_state_device(const Chain& H, double** taps, double** filt, int** primed) {
	if (taps) *taps = H.taps;
	if (filt) *filt = H.filt;
	if (primed) *primed = H.primed;
	return SAIP_OK;
}
// the state for tests and debugging: taps [n][tap_rows][depth][B], filt [n][filt_rows][B], primed [n][B]; any may be null
saip_status saip::eng::chain_state_host(const ChainKind& K, saip_batch* b, const Chain& H, double* taps, double* filt, int* primed, const char* fn) {
	saip_status st = need_ready(b, fn);
	if (st) return st;
	const int n = b->model->n;
	if (taps && H.depth > 0 && (st = copy_d2h(b, taps, H.taps, K.tap_rows * H.depth * n))) return st;
	if (filt && (st = copy_d2h(b, filt, H.filt, K.filt_rows * n))) return st;
	if (primed) {
		HIP_TRY(hipMemcpy2DAsync(primed, (size_t)b->B * sizeof(int), H.primed, (size_t)b->ld * sizeof(int), (size_t)b->B * sizeof(int), n, hipMemcpyDeviceToHost, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
	}
	return SAIP_OK;
}
