#include "saip_engine_internal.h"

// ---- the inertia table of the simulated robot (saip_inertia.hip): what the resident integrator reads in place of the model's masses,
// centres of mass and inertias.  enqueue_integrate (saip_engine_rollout.cpp) hands it to every integrate launch while it is attached.
static saip_status need_inertia(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->inertia.attached) return fail(SAIP_ERR_ORDER, "%s: no inertia table is attached (saip_batch_inertia_attach)", fn);
	return SAIP_OK;
}
void saip::eng::inertia_free(saip_batch* b) {
	auto& C = b->inertia;
	for (void* p : {(void*)C.rows, (void*)C.parts, (void*)C.bounds})
		if (p) (void)hipFree(p);
	C = saip_batch::Inertia();
}
static const char* const INERTIA_ROW_WORD_NAMES[saip::INERTIA_ROW_WORDS] = {"m", "cx", "cy", "cz", "Ixx", "Iyy", "Izz", "Ixy", "Ixz", "Iyz"};
static const char* const INERTIA_BODY_WORD_NAMES[saip::INERTIA_BODY_WORDS] = {"s", "dx", "dy", "dz"};
static const char* const INERTIA_PAYLOAD_WORD_NAMES[saip::INERTIA_PAYLOAD_WORDS] = {"m_p", "c_p[0]", "c_p[1]", "c_p[2]", "hx", "hy", "hz"};
// "body 3 of instance 5" / "body 3"
static void inertia_who(char* who, size_t len, const char* what, int j, size_t i, size_t cols) {
	if (cols > 1) snprintf(who, len, "%s %d of instance %zu", what, j, i);
	else snprintf(who, len, "%s %d", what, j);
}
// the smallest eigenvalue of the symmetric 3 x 3 matrix with the six words xx yy zz xy xz yz (the trigonometric closed form)
static double sym3_min_eig(const double* I) {
	const double p1 = I[3] * I[3] + I[4] * I[4] + I[5] * I[5];
	if (p1 == 0) return std::fmin(I[0], std::fmin(I[1], I[2]));
	const double q = (I[0] + I[1] + I[2]) / 3;
	const double a = I[0] - q, b = I[1] - q, c = I[2] - q;
	const double p = std::sqrt((a * a + b * b + c * c + 2 * p1) / 6);
	const double det = a * (b * c - I[5] * I[5]) - I[3] * (I[3] * c - I[5] * I[4]) + I[4] * (I[3] * I[5] - b * I[4]);
	const double r = std::fmax(-1.0, std::fmin(1.0, det / (2 * p * p * p)));
	return q + 2 * p * std::cos(std::acos(r) / 3 + 2 * M_PI / 3);
}
// a table of rows [n][10] (cols = 1) or [n][10][cols]: true when fine, else msg names the body, the word (and the instance)
static bool inertia_check_rows(const double* t, int n, size_t cols, char* msg, size_t len) {
	using namespace saip;
	for (int j = 0; j < n; j++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)j * INERTIA_ROW_WORDS * cols + i;
			char who[64];
			inertia_who(who, sizeof(who), "body", j, i, cols);
			double I[6];
			for (int k = 0; k < INERTIA_ROW_WORDS; k++) {
				const double v = w[k * cols];
				if (!std::isfinite(v)) return snprintf(msg, len, "%s: word %s is not finite", who, INERTIA_ROW_WORD_NAMES[k]), false;
				if (k >= 4) I[k - 4] = v;
			}
			if (w[0] < 0) return snprintf(msg, len, "%s: word m = %g is below 0", who, w[0]), false;
			const double trace = I[0] + I[1] + I[2], lam = sym3_min_eig(I);
			if (lam < -1e-12 * std::fmax(1.0, trace))
				return snprintf(msg, len, "%s: words Ixx..Iyz: the inertia has the eigenvalue %g, below 0", who, lam), false;
		}
	return true;
}
// body parts [n][4] or [n][4][cols]: finite, s > 0, and s m > 0 wherever the model's m is
static bool inertia_check_bodies(const saip_model* M, const double* t, size_t cols, char* msg, size_t len) {
	using namespace saip;
	for (int j = 0; j < M->n; j++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)j * INERTIA_BODY_WORDS * cols + i;
			char who[64];
			inertia_who(who, sizeof(who), "body", j, i, cols);
			for (int k = 0; k < INERTIA_BODY_WORDS; k++)
				if (!std::isfinite(w[k * cols])) return snprintf(msg, len, "%s: word %s is not finite", who, INERTIA_BODY_WORD_NAMES[k]), false;
			if (!(w[0] > 0)) return snprintf(msg, len, "%s: word s = %g must be positive", who, w[0]), false;
			if (M->dev.mass[j] > 0 && !(w[0] * M->dev.mass[j] > 0)) return snprintf(msg, len, "%s: word s = %g leaves the body without mass", who, w[0]), false;
		}
	return true;
}
// payload words [P][7] or [P][7][cols]: finite, m_p >= 0, h >= 0
static bool inertia_check_payloads(const double* t, int P, size_t cols, char* msg, size_t len) {
	using namespace saip;
	for (int p = 0; p < P; p++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)p * INERTIA_PAYLOAD_WORDS * cols + i;
			char who[64];
			inertia_who(who, sizeof(who), "payload", p, i, cols);
			for (int k = 0; k < INERTIA_PAYLOAD_WORDS; k++) {
				const double v = w[k * cols];
				if (!std::isfinite(v)) return snprintf(msg, len, "%s: word %s is not finite", who, INERTIA_PAYLOAD_WORD_NAMES[k]), false;
				if ((k == 0 || k >= 4) && v < 0) return snprintf(msg, len, "%s: word %s = %g is below 0", who, INERTIA_PAYLOAD_WORD_NAMES[k], v), false;
			}
		}
	return true;
}
static void inertia_model_rows(const saip_model* M, size_t cols, std::vector<double>& out) {
	out.assign((size_t)M->n * saip::INERTIA_ROW_WORDS * cols, 0.0);
	for (int j = 0; j < M->n; j++) {
		const double w[saip::INERTIA_ROW_WORDS] = {M->dev.mass[j],       M->dev.com[j][0],     M->dev.com[j][1],     M->dev.com[j][2],     M->dev.inertia[j][0],
													M->dev.inertia[j][1], M->dev.inertia[j][2], M->dev.inertia[j][3], M->dev.inertia[j][4], M->dev.inertia[j][5]};
		for (int k = 0; k < saip::INERTIA_ROW_WORDS; k++)
			for (size_t i = 0; i < cols; i++) out[((size_t)j * saip::INERTIA_ROW_WORDS + k) * cols + i] = w[k];
	}
}
extern "C" saip_status saip_batch_inertia_attach(saip_batch* b, const double* rows, int per_instance, int n_payloads, const int* payload_links) {
	using namespace saip;
	const char* fn = "saip_batch_inertia_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->inertia.attached) return fail(SAIP_ERR_ORDER, "%s: an inertia table is already attached (saip_batch_inertia_detach first)", fn);
	const int P = n_payloads, n = b->model->n;
	if (P < 0 || P > INERTIA_MAX_PAYLOADS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d payloads required (got %d)", fn, INERTIA_MAX_PAYLOADS, P);
	if (P > 0 && !payload_links) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null payload links", fn);
	per_instance = per_instance ? 1 : 0;
	InertiaSite site[INERTIA_MAX_PAYLOADS] = {};
	const int nl = (int)b->model->links.size();
	for (int p = 0; p < P; p++) {
		if (payload_links[p] < 0 || payload_links[p] >= nl)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: payload %d: link index %d out of range (%d links)", fn, p, payload_links[p], nl);
		// the site link's frame in its movable body: a welded link brings its fixed transform, as a plant wrench's site does
		const LinkInfo& L = b->model->links[payload_links[p]];
		if (L.body < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: payload %d: link %s is welded to the fixed base (a payload there moves nothing)", fn, p, L.name.c_str());
		site[p].body = L.body;
		memcpy(site[p].pos, L.p, sizeof(L.p));
		memcpy(site[p].rot, L.R, sizeof(L.R));
	}
	const size_t cols = per_instance ? (size_t)b->B : 1;
	std::vector<double> own;
	if (!rows) {
		inertia_model_rows(b->model, cols, own);
		rows = own.data();
	}
	char msg[200];
	if (!inertia_check_rows(rows, n, cols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [n][10][ld] doubles: the byte count must fit a size_t
	if ((size_t)b->ld > SIZE_MAX / ((size_t)n * INERTIA_ROW_WORDS * sizeof(double))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->inertia;
	C = saip_batch::Inertia();
	const size_t ld = b->ld, wide = per_instance ? ld : 1, nrows = (size_t)n * INERTIA_ROW_WORDS, nparts = (size_t)n * INERTIA_BODY_WORDS + (size_t)P * INERTIA_PAYLOAD_WORDS;
	if ((st = alloc_zero(b, &C.rows, nrows * wide)) || (st = alloc_zero(b, &C.parts, nparts * wide)) || (per_instance && (st = alloc_zero(b, &C.bounds, 2 * nparts))) ||
		(st = upload_table(b, C.rows, rows, nrows, per_instance, "table", fn))) {
		inertia_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance = per_instance;
	C.n_payloads = P;
	for (int p = 0; p < P; p++) C.site[p] = site[p];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_inertia_detach(saip_batch* b) {
	const char* fn = "saip_batch_inertia_detach";
	saip_status st = need_inertia(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // an integration may still be reading the table
	inertia_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_inertia_info(saip_batch* b, int* per_instance, int* n_payloads, int* payload_bodies, double* payload_frames) {
	saip_status st = need_inertia(b, "saip_batch_inertia_info");
	if (st) return st;
	const auto& C = b->inertia;
	if (per_instance) *per_instance = C.per_instance;
	if (n_payloads) *n_payloads = C.n_payloads;
	if (payload_bodies)
		for (int p = 0; p < C.n_payloads; p++) payload_bodies[p] = C.site[p].body;
	if (payload_frames)
		for (int p = 0; p < C.n_payloads; p++) {
			memcpy(payload_frames + 12 * p, C.site[p].pos, 3 * sizeof(double));
			memcpy(payload_frames + 12 * p + 3, C.site[p].rot, 9 * sizeof(double));
		}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_inertia_set_rows_host(saip_batch* b, const double* rows) {
	const char* fn = "saip_batch_inertia_set_rows_host";
	saip_status st = need_inertia(b, fn);
	if (st) return st;
	if (!rows) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null table", fn);
	const auto& C = b->inertia;
	char msg[200];
	if (!inertia_check_rows(rows, b->model->n, C.per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.rows, rows, (size_t)b->model->n * saip::INERTIA_ROW_WORDS, C.per_instance, "table", fn);
}
// the launch both front ends share: the parts (or their bounds) are on the device already
static saip_status inertia_compose(saip_batch* b, saip::InertiaComposeParams& P) {
	const auto& C = b->inertia;
	P.cols = C.per_instance ? b->B : 1;
	P.ld = b->ld;
	P.n = b->model->n;
	P.n_payloads = C.n_payloads;
	P.stride = C.per_instance ? b->ld : 1;
	P.model = b->model_dev;
	P.rows = C.rows;
	for (int p = 0; p < C.n_payloads; p++) P.site[p] = C.site[p];
	hipError_t e = saip::launch_inertia_compose(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "inertia compose launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_inertia_set_parts_host(saip_batch* b, const double* bodies, int per_instance_bodies, const double* payloads, int per_instance_payloads) {
	using namespace saip;
	const char* fn = "saip_batch_inertia_set_parts_host";
	saip_status st = need_inertia(b, fn);
	if (st) return st;
	const auto& C = b->inertia;
	const int n = b->model->n, P = C.n_payloads;
	per_instance_bodies = per_instance_bodies && bodies ? 1 : 0;
	per_instance_payloads = per_instance_payloads && payloads && P > 0 ? 1 : 0;
	if ((per_instance_bodies || per_instance_payloads) && !C.per_instance)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: per-instance parts on a batch-uniform table (attach it per instance)", fn);
	const size_t nb = (size_t)n * INERTIA_BODY_WORDS, np = (size_t)P * INERTIA_PAYLOAD_WORDS;
	std::vector<double> neutral_b, neutral_p;
	if (!bodies) {
		neutral_b.assign(nb, 0.0);
		for (int j = 0; j < n; j++) neutral_b[(size_t)j * INERTIA_BODY_WORDS] = 1.0;
		bodies = neutral_b.data();
	}
	if (!payloads) {
		neutral_p.assign(np + 1, 0.0);
		payloads = neutral_p.data();
	}
	char msg[200];
	if (!inertia_check_bodies(b->model, bodies, per_instance_bodies ? (size_t)b->B : 1, msg, sizeof(msg)) ||
		!inertia_check_payloads(payloads, P, per_instance_payloads ? (size_t)b->B : 1, msg, sizeof(msg)))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	double* pb = C.parts;
	double* pp = C.parts + nb * (C.per_instance ? (size_t)b->ld : 1);
	if ((st = upload_table(b, pb, bodies, nb, per_instance_bodies, "table", fn)) || (P > 0 && (st = upload_table(b, pp, payloads, np, per_instance_payloads, "table", fn)))) return st;
	InertiaComposeParams K;
	memset(&K, 0, sizeof(K));
	K.per_instance_bodies = per_instance_bodies;
	K.per_instance_payloads = per_instance_payloads;
	K.bodies = pb;
	K.payloads = pp;
	return inertia_compose(b, K);
}
// The parts drawn on the device between two batch-uniform tables (host pointers: bodies [n][4], payloads [P][7]) and composed; a null pair
// stands for the neutral words.  Whatever the draw, the rows stay valid: both bounds of every word have to be.
extern "C" saip_status saip_batch_inertia_randomize(saip_batch* b, unsigned long long seed, long long round, const double* body_lo, const double* body_hi,
													 const double* payload_lo, const double* payload_hi) {
	using namespace saip;
	const char* fn = "saip_batch_inertia_randomize";
	saip_status st = need_inertia(b, fn);
	if (st) return st;
	const auto& C = b->inertia;
	const int n = b->model->n, P = C.n_payloads;
	if ((st = check_bound_pairs(fn, body_lo, body_hi, payload_lo, payload_hi))) return st;
	if (payload_lo && P == 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the table was attached without payloads", fn);
	if (!C.per_instance) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the table is batch-uniform (attach it per instance)", fn);
	const size_t nb = (size_t)n * INERTIA_BODY_WORDS, np = (size_t)P * INERTIA_PAYLOAD_WORDS;
	std::vector<double> neutral_b, neutral_p;
	if (!body_lo) {
		neutral_b.assign(nb, 0.0);
		for (int j = 0; j < n; j++) neutral_b[(size_t)j * INERTIA_BODY_WORDS] = 1.0;
		body_lo = body_hi = neutral_b.data();
	}
	if (!payload_lo) {
		neutral_p.assign(np + 1, 0.0);
		payload_lo = payload_hi = neutral_p.data();
	}
	// every word of both tables has to be finite: nothing to scan for a bound infinite on one side only
	if ((st = check_bound_pair(fn, body_lo, body_hi, [&](const double* t, char* msg, size_t len) { return inertia_check_bodies(b->model, t, 1, msg, len); })) ||
		(st = check_bound_pair(fn, payload_lo, payload_hi, [&](const double* t, char* msg, size_t len) { return inertia_check_payloads(t, P, 1, msg, len); })) || (st = need_ready(b, fn)))
		return st;
	double* bl = C.bounds;
	double* bh = bl + nb;
	double* pl = bh + nb;
	double* ph = pl + np;
	if ((st = upload_bound_pair(b, bl, body_lo, body_hi, nb, fn)) || (P > 0 && (st = upload_bound_pair(b, pl, payload_lo, payload_hi, np, fn)))) return st;
	InertiaComposeParams K;
	memset(&K, 0, sizeof(K));
	K.draw = 1;
	K.seed_lo = (uint32_t)seed;
	K.seed_hi = (uint32_t)(seed >> 32);
	K.round = (uint32_t)round;
	K.bodies = bl;
	K.bodies_hi = bh;
	K.payloads = pl;
	K.payloads_hi = ph;
	return inertia_compose(b, K);
}
extern "C" saip_status saip_batch_inertia_rows_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_inertia_rows_host";
	saip_status st = need_inertia(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	const auto& C = b->inertia;
	const int rows = b->model->n * saip::INERTIA_ROW_WORDS;
	if (C.per_instance) return copy_d2h(b, out, C.rows, rows);
	HIP_TRY(hipMemcpyAsync(out, C.rows, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" double* saip_batch_inertia_rows_device(saip_batch* b) { return b ? b->inertia.rows : nullptr; }
