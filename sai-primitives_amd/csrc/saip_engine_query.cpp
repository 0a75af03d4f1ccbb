#include "saip_engine_internal.h"

// ---- robot-model queries (saip_model_query.hip): the batched SaiModel accessors at the resident state
extern "C" saip_status saip_batch_finalize_model_only(saip_batch* b) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return b->model_only ? SAIP_OK : fail(SAIP_ERR_ORDER, "saip_batch_finalize_model_only: the batch is already finalized as a controller");
	if (!b->tasks.empty()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_finalize_model_only: the batch has tasks (use saip_batch_finalize)");
	if (has_device(b)) {
		HIP_TRY(hipSetDevice(b->device));
		HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
		const size_t n = b->model->n, ld = b->ld;
		saip_status st;
		if ((st = dev_alloc(b, &b->q, n * ld)) || (st = dev_alloc(b, &b->dq, n * ld)) || (st = dev_alloc(b, &b->model_dev, 1))) return st;
		HIP_TRY(hipMemcpy(b->model_dev, &b->model->dev, sizeof(ModelDev), hipMemcpyHostToDevice));
	}
	b->finalized = true;
	b->model_only = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_robot_base(saip_batch* b, const double R[9], const double p[3]) {
	if (!b || !R || !p) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: null argument");
	for (int i = 0; i < 9; i++)
		if (!std::isfinite(R[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: non-finite rotation");
	for (int i = 0; i < 3; i++)
		if (!std::isfinite(p[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: non-finite translation");
	memcpy(b->base_R, R, sizeof(b->base_R));
	memcpy(b->base_p, p, sizeof(b->base_p));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_robot_base(const saip_batch* b, double R[9], double p[3]) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_get_robot_base: null batch");
	if (R) memcpy(R, b->base_R, sizeof(b->base_R));
	if (p) memcpy(p, b->base_p, sizeof(b->base_p));
	return SAIP_OK;
}
extern "C" int saip_batch_model_frame_rows(const saip_batch* b, int flags) {
	if (!b || !b->model || (flags & ~(SAIP_QUERY_JACOBIAN | SAIP_QUERY_WORLD))) return 0;
	return 18 + ((flags & SAIP_QUERY_JACOBIAN) ? 6 * b->model->n : 0);
}
// the _host scratch: grown to the largest query seen, never shrunk
static saip_status query_scratch(saip_batch* b, size_t rows) {
	if (rows <= b->query_rows) return SAIP_OK;
	saip_status st = dev_alloc(b, &b->query_dev, rows * b->ld);
	if (st) return st;
	b->query_rows = rows;
	return SAIP_OK;
}
// argument errors come before the device check, so that they show on a configuration-only batch as well
static saip_status check_frames(saip_batch* b, int nf, const int* links, int flags, const double* out, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (nf < 1 || nf > SAIP_MAX_QUERY_FRAMES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_frames %d outside 1..%d", fn, nf, SAIP_MAX_QUERY_FRAMES);
	if (!links || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links or output", fn);
	if (flags & ~(SAIP_QUERY_JACOBIAN | SAIP_QUERY_WORLD)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", fn, flags);
	const int nl = (int)b->model->links.size();
	for (int f = 0; f < nf; f++)
		if (links[f] < 0 || links[f] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: link index %d out of range (%d links)", fn, links[f], nl);
	return need_state(b, fn);
}
static saip_status launch_frames(saip_batch* b, int nf, const int* links, const double* pos_in_link, int flags, double* out_dev, const char* fn) {
	saip_status st = check_frames(b, nf, links, flags, out_dev, fn);
	if (st) return st;
	saip::FrameQuery Q;
	memset(&Q, 0, sizeof(Q));
	Q.B = b->B;
	Q.ld = b->ld;
	Q.n = b->model->n;
	Q.nf = nf;
	Q.rows = saip_batch_model_frame_rows(b, flags);
	Q.jac = (flags & SAIP_QUERY_JACOBIAN) ? 1 : 0;
	Q.world = (flags & SAIP_QUERY_WORLD) ? 1 : 0;
	// frames sorted by body (stable: one walk emits them in order); the constants are composed exactly as saip_batch_add_motion_force_task
	// composes a task's control frame, so that a frame equal to one is bit-identical to the pose readback
	int order[SAIP_MAX_QUERY_FRAMES];
	for (int f = 0; f < nf; f++) order[f] = f;
	for (int i = 1; i < nf; i++)
		for (int k = i; k > 0 && b->model->links[links[order[k - 1]]].body > b->model->links[links[order[k]]].body; k--) std::swap(order[k - 1], order[k]);
	double I3[9];
	m3_eye(I3);
	for (int i = 0; i < nf; i++) {
		const int f = order[i];
		const LinkInfo& L = b->model->links[links[f]];
		const double zero[3] = {0, 0, 0};
		double t[3];
		m3_vec(L.R, pos_in_link ? pos_in_link + 3 * f : zero, t);
		for (int e = 0; e < 3; e++) Q.pos[i][e] = L.p[e] + t[e];
		m3_mul(L.R, I3, Q.rot[i]);
		Q.body[i] = L.body;
		Q.slot[i] = f;
	}
	memcpy(Q.Rwb, b->base_R, sizeof(Q.Rwb));
	memcpy(Q.pwb, b->base_p, sizeof(Q.pwb));
	Q.model = b->model_dev;
	Q.q = b->q;
	Q.dq = b->dq;
	Q.out = out_dev;
	hipError_t e = saip::launch_model_frames(Q, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "model frames kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_model_frames_device(saip_batch* b, int n_frames, const int* links, const double* pos_in_link, int flags, double* out_dev) {
	return launch_frames(b, n_frames, links, pos_in_link, flags, out_dev, "saip_batch_model_frames_device");
}
extern "C" saip_status saip_batch_model_frames_host(saip_batch* b, int n_frames, const int* links, const double* pos_in_link, int flags, double* out) {
	const char* fn = "saip_batch_model_frames_host";
	saip_status st = check_frames(b, n_frames, links, flags, out, fn);
	if (st) return st;
	const int rows = saip_batch_model_frame_rows(b, flags);
	if ((st = query_scratch(b, (size_t)n_frames * rows))) return st;
	if ((st = launch_frames(b, n_frames, links, pos_in_link, flags, b->query_dev, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, out, b->query_dev, n_frames * rows);
}
static saip_status check_dynamics(saip_batch* b, bool any_output, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (!any_output) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: every output is NULL", fn);
	return need_state(b, fn);
}
static saip_status launch_dynamics(saip_batch* b, double* M, double* Minv, double* g, double* h, const char* fn) {
	saip_status st = check_dynamics(b, M || Minv || g || h, fn);
	if (st) return st;
	saip::DynQuery Q;
	memset(&Q, 0, sizeof(Q));
	Q.B = b->B;
	Q.ld = b->ld;
	Q.n = b->model->n;
	Q.model = b->model_dev;
	Q.q = b->q;
	Q.dq = b->dq;
	Q.M = M;
	Q.Minv = Minv;
	Q.g = g;
	Q.h = h;
	hipError_t e = saip::launch_model_dynamics(Q, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "model dynamics kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_model_dynamics_device(saip_batch* b, double* M_dev, double* M_inv_dev, double* g_dev, double* b_dev) {
	return launch_dynamics(b, M_dev, M_inv_dev, g_dev, b_dev, "saip_batch_model_dynamics_device");
}
extern "C" saip_status saip_batch_model_dynamics_host(saip_batch* b, double* M, double* M_inv, double* g, double* bias) {
	const char* fn = "saip_batch_model_dynamics_host";
	saip_status st = check_dynamics(b, M || M_inv || g || bias, fn);
	if (st) return st;
	const size_t n = b->model->n, ld = b->ld;
	if ((st = query_scratch(b, 2 * n * n + 2 * n))) return st;  // M, M^-1, g, b blocks
	double* d = b->query_dev;
	if ((st = launch_dynamics(b, M ? d : nullptr, M_inv ? d + n * n * ld : nullptr, g ? d + 2 * n * n * ld : nullptr, bias ? d + (2 * n * n + n) * ld : nullptr, fn)))
		return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (M && (st = copy_d2h(b, M, d, (int)(n * n)))) return st;
	if (M_inv && (st = copy_d2h(b, M_inv, d + n * n * ld, (int)(n * n)))) return st;
	if (g && (st = copy_d2h(b, g, d + 2 * n * n * ld, (int)n))) return st;
	if (bias && (st = copy_d2h(b, bias, d + (2 * n * n + n) * ld, (int)n))) return st;
	return SAIP_OK;
}
