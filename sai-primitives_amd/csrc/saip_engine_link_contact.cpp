#include "saip_engine_internal.h"

// ---- link contact (saip_link_contact.hip): world-fixed obstacles push back on the robot's link spheres in front of every integration substep
static saip_status need_link_contact(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->link_contact.attached) return fail(SAIP_ERR_ORDER, "%s: no link contact is attached (saip_batch_link_contact_attach)", fn);
	return SAIP_OK;
}
void saip::eng::link_contact_free(saip_batch* b) {
	link_object_free(b);  // the second stage goes with the first
	auto& C = b->link_contact;
	for (void* p : {(void*)C.geom_dev, (void*)C.obst, (void*)C.mat, (void*)C.tau_sim, (void*)C.readout, (void*)C.summary, (void*)C.keep_dev})
		if (p) (void)hipFree(p);
	C = saip_batch::LinkContact();
}
// the material table [O][4] = { k, c, mu, v_s }; false: `msg` says what is wrong with which word
static bool link_contact_check_materials(const double* mat, int O, char* msg, size_t len) {
	static const char* const names[saip::LINK_CONTACT_MATERIAL_WORDS] = {"k", "c", "mu", "v_s"};
	for (int o = 0; o < O; o++) {
		const double* w = mat + (size_t)o * saip::LINK_CONTACT_MATERIAL_WORDS;
		for (int k = 0; k < saip::LINK_CONTACT_MATERIAL_WORDS; k++)
			if (w[k] != w[k]) return snprintf(msg, len, "material %d: word %d (%s) is NaN", o, k, names[k]), false;
		for (int k = 0; k < 3; k++)
			if (!(w[k] >= 0) || !std::isfinite(w[k])) return snprintf(msg, len, "material %d: word %d (%s) = %g is negative or not finite", o, k, names[k], w[k]), false;
		if (w[2] > 0 && !(w[3] > 0)) return snprintf(msg, len, "material %d: word 3 (v_s) = %g with friction mu > 0: v_s > 0 required", o, w[3]), false;
	}
	return true;
}
extern "C" saip_status saip_batch_link_contact_attach(saip_batch* b, int n_spheres, const int* links, const double* centres, const double* radii, int n_obstacles,
													  const double* obstacles, const double* materials, int per_instance, int keep) {
	const char* fn = "saip_batch_link_contact_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->link_contact.attached) return fail(SAIP_ERR_ORDER, "%s: link contact is already attached (saip_batch_link_contact_detach first)", fn);
	const int S = n_spheres, O = n_obstacles;
	if (S < 1 || S > saip::LINK_CONTACT_MAX_SPHERES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d spheres required (got %d)", fn, saip::LINK_CONTACT_MAX_SPHERES, S);
	if (O < 1 || O > saip::LINK_CONTACT_MAX_OBSTACLES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d obstacles required (got %d)", fn, saip::LINK_CONTACT_MAX_OBSTACLES, O);
	if (!links || !centres || !radii) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links, centres or radii", fn);
	if (!obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	if (!materials) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null materials", fn);
	per_instance = per_instance ? 1 : 0;
	keep = keep ? 1 : 0;
	const int nl = (int)b->model->links.size();
	for (int s = 0; s < S; s++) {
		if (links[s] < 0 || links[s] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: link index %d out of range (%d links)", fn, s, links[s], nl);
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(centres[3 * s + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the centre is not finite", fn, s);
		if (!std::isfinite(radii[s])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the radius is not finite", fn, s);
		if (radii[s] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: radius %g below 0", fn, s, radii[s]);
	}
	char msg[200];
	if (!clearance_check_obstacles(obstacles, O, per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (!link_contact_check_materials(materials, O, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [O][8][ld], [9 S][ld], [n][ld] doubles: the byte counts must fit a size_t
	const size_t widest = (size_t)9 * saip::LINK_CONTACT_MAX_SPHERES * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->link_contact;
	C = saip_batch::LinkContact();
	saip::LinkContactGeom& G = C.geom;
	memset(&G, 0, sizeof(G));
	G.S = S;
	G.O = O;
	G.jmax = -1;
	// the spheres sorted by body (stable), their constants composed exactly as saip_batch_clearance_attach composes them
	const ModelDev& md = b->model->dev;
	int order[saip::LINK_CONTACT_MAX_SPHERES];
	for (int s = 0; s < S; s++) order[s] = s;
	for (int i = 1; i < S; i++)
		for (int k = i; k > 0 && b->model->links[links[order[k - 1]]].body > b->model->links[links[order[k]]].body; k--) std::swap(order[k - 1], order[k]);
	for (int j = 0; j < saip::LINK_CONTACT_MAX_JOINTS; j++) G.owner[j] = -1;
	for (int i = 0; i < S; i++) {
		const int s = order[i];
		const LinkInfo& L = b->model->links[links[s]];
		double t[3];
		m3_vec(L.R, centres + 3 * s, t);
		for (int e = 0; e < 3; e++) G.r[i][e] = L.p[e] + t[e];
		G.body[i] = L.body;
		G.slot[i] = s;
		G.radius[i] = radii[s];
		G.anc[i] = L.body < 0 ? 0u : md.is_tree ? md.anc[L.body] : (uint32_t)(((uint64_t)2 << L.body) - 1);
		if (L.body > G.jmax) G.jmax = L.body;
		for (int j = 0; j <= L.body; j++)
			if (((G.anc[i] >> j) & 1u) && G.owner[j] < 0) G.owner[j] = i;
	}
	auto upload_geom = [&]() -> saip_status {
		HIP_TRY(hipMalloc((void**)&C.geom_dev, sizeof(G)));
		HIP_TRY(hipMemcpyAsync(C.geom_dev, &G, sizeof(G), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
		return SAIP_OK;
	};
	const size_t ld = b->ld, rows = (size_t)O * saip::LINK_CONTACT_OBSTACLE_WORDS, mrows = (size_t)O * saip::LINK_CONTACT_MATERIAL_WORDS;
	if ((st = upload_geom()) || (st = alloc_zero(b, &C.obst, rows * (per_instance ? ld : 1))) || (st = alloc_zero(b, &C.mat, mrows)) ||
		(st = alloc_zero(b, &C.tau_sim, (size_t)b->model->n * ld)) || (st = alloc_zero(b, &C.readout, (size_t)saip::LINK_CONTACT_READOUT_ROWS * ld)) ||
		(st = alloc_zero(b, &C.summary, (size_t)saip::LINK_CONTACT_SUMMARY_ROWS * ld)) || (keep && (st = alloc_zero(b, &C.keep_dev, (size_t)9 * S * ld))) ||
		(st = upload_table(b, C.obst, obstacles, rows, per_instance, "obstacle", fn)) || (st = upload_table(b, C.mat, materials, mrows, 0, "material", fn))) {
		link_contact_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance = per_instance;
	C.keep = keep;
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_contact_detach(saip_batch* b) {
	const char* fn = "saip_batch_link_contact_detach";
	saip_status st = need_link_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a substep may still be in flight
	link_contact_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_contact_info(saip_batch* b, int* n_spheres, int* n_obstacles, int* per_instance, int* keep) {
	saip_status st = need_link_contact(b, "saip_batch_link_contact_info");
	if (st) return st;
	const auto& C = b->link_contact;
	if (n_spheres) *n_spheres = C.geom.S;
	if (n_obstacles) *n_obstacles = C.geom.O;
	if (per_instance) *per_instance = C.per_instance;
	if (keep) *keep = C.keep;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_contact_set_obstacles_host(saip_batch* b, const double* obstacles) {
	const char* fn = "saip_batch_link_contact_set_obstacles_host";
	saip_status st = need_link_contact(b, fn);
	if (st) return st;
	const auto& C = b->link_contact;
	if (!obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	char msg[200];
	if (!clearance_check_obstacles(obstacles, C.geom.O, C.per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.obst, obstacles, (size_t)C.geom.O * saip::LINK_CONTACT_OBSTACLE_WORDS, C.per_instance, "obstacle", fn);
}
extern "C" saip_status saip_batch_link_contact_set_materials_host(saip_batch* b, const double* materials) {
	const char* fn = "saip_batch_link_contact_set_materials_host";
	saip_status st = need_link_contact(b, fn);
	if (st) return st;
	const auto& C = b->link_contact;
	if (!materials) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null materials", fn);
	char msg[200];
	if (!link_contact_check_materials(materials, C.geom.O, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, C.mat, materials, (size_t)C.geom.O * saip::LINK_CONTACT_MATERIAL_WORDS, 0, "material", fn);
}
extern "C" double* saip_batch_link_contact_obstacles_device(saip_batch* b) { return b ? b->link_contact.obst : nullptr; }
extern "C" double* saip_batch_link_contact_torques_device(saip_batch* b) { return b ? b->link_contact.tau_sim : nullptr; }
extern "C" double* saip_batch_link_contact_readout_device(saip_batch* b) { return b ? b->link_contact.readout : nullptr; }
extern "C" double* saip_batch_link_contact_summary_device(saip_batch* b) { return b ? b->link_contact.summary : nullptr; }
extern "C" double* saip_batch_link_contact_keep_device(saip_batch* b) { return b ? b->link_contact.keep_dev : nullptr; }
// one launch of the link-contact kernel at the resident state; dt: the substep an APPLY launch stands in front of
saip_status saip::eng::link_contact_launch(saip_batch* b, int mode, double dt, const double* gravity) {
	const auto& C = b->link_contact;
	saip::LinkContactParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.per_instance = C.per_instance;
	P.S = C.geom.S;
	P.O = C.geom.O;
	P.dt = dt;
	P.model = b->model_dev;
	P.geom = C.geom_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.obst = C.obst;
	P.mat = C.mat;
	P.tau_cmd = tau_buffer(b, sim_plan(b).link_contact_in);  // (read by APPLY only, which follows the plant launch)
	P.tau_sim = tau_buffer(b, saip::TauBuf::LinkContact);
	P.readout = C.readout;
	P.summary = C.summary;
	P.keep = C.keep_dev;
	hipError_t e;
	if (b->link_object.attached) {
		// the launch with the object replaces the plain one
		const auto& J = b->link_object;
		saip::LinkObjectParams Q;
		memset(&Q, 0, sizeof(Q));
		Q.lc = P;
		Q.geom = J.geom_dev;
		Q.inertial = J.inertial;
		Q.inertial_per_instance = J.per_instance;
		for (int i = 0; i < 3; i++) Q.gravity[i] = gravity ? gravity[i] : b->model->dev.gravity[i];
		Q.state = J.state;
		Q.readout = J.readout;
		Q.summary = J.summary;
		e = saip::launch_link_object_apply(Q, b->model->dev.is_tree != 0, b->stream);
	} else {
		e = saip::launch_link_contact_apply(P, b->model->dev.is_tree != 0, b->stream);
	}
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "link contact launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_contact_evaluate(saip_batch* b) {
	const char* fn = "saip_batch_link_contact_evaluate";
	saip_status st = need_link_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return link_contact_launch(b, saip::LINK_CONTACT_EVALUATE, 0.0);
}
extern "C" saip_status saip_batch_link_contact_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_link_contact_readout_host";
	const saip_status st = need_link_contact(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->link_contact.readout, saip::LINK_CONTACT_READOUT_ROWS, fn);
}
extern "C" saip_status saip_batch_link_contact_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_link_contact_summary_host";
	const saip_status st = need_link_contact(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->link_contact.summary, saip::LINK_CONTACT_SUMMARY_ROWS, fn);
}
extern "C" saip_status saip_batch_link_contact_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_link_contact_summary_reset";
	saip_status st = need_link_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_link_contact_summary_reset(b->B, b->ld, b->link_contact.summary, b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_contact_add_cost(saip_batch* b, double w_impulse, double w_peak) {
	const char* fn = "saip_batch_link_contact_add_cost";
	saip_status st = need_link_contact(b, fn);
	if (st) return st;
	if (b->n_samp == 0) return fail(SAIP_ERR_ORDER, "%s: no sampler is attached (saip_batch_sampler_attach): there is no cost to add to", fn);
	if (w_impulse != w_impulse || w_peak != w_peak) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a weight is NaN", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_link_contact_add_cost(b->B, b->ld, b->link_contact.summary, b->samp_cost, w_impulse, w_peak, b->stream));
	return SAIP_OK;
}

// ---- the pushed object (saip_link_object.h): a free rigid body of spheres, the optional second stage of link contact
static saip_status need_link_object(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->link_object.attached) return fail(SAIP_ERR_ORDER, "%s: no link object is attached (saip_batch_link_object_attach)", fn);
	return SAIP_OK;
}
void saip::eng::link_object_free(saip_batch* b) {
	auto& J = b->link_object;
	for (void* p : {(void*)J.geom_dev, (void*)J.inertial, (void*)J.state, (void*)J.readout, (void*)J.summary})
		if (p) (void)hipFree(p);
	J = saip_batch::LinkObject();
}
// the inertial words [4] or [4][cols] = { m, Ix, Iy, Iz }: all > 0 and finite
static bool link_object_check_inertial(const double* in, size_t cols, bool per_instance, char* msg, size_t len) {
	static const char* const names[saip::LINK_OBJECT_INERTIAL_WORDS] = {"m", "Ix", "Iy", "Iz"};
	for (int k = 0; k < saip::LINK_OBJECT_INERTIAL_WORDS; k++)
		for (size_t i = 0; i < cols; i++) {
			const double v = in[(size_t)k * cols + i];
			if (v > 0 && std::isfinite(v)) continue;
			if (per_instance) snprintf(msg, len, "inertial word %d (%s) of instance %zu = %g: > 0 and finite required", k, names[k], i, v);
			else snprintf(msg, len, "inertial word %d (%s) = %g: > 0 and finite required", k, names[k], v);
			return false;
		}
	return true;
}
// state [13] or [13][cols] -> out [13][cols] with unit quaternions; false: `msg` names the instance whose quaternion cannot be normalised
static bool link_object_prepare_state(const double* state, size_t cols, bool per_instance, std::vector<double>& out, char* msg, size_t len) {
	out.assign((size_t)saip::LINK_OBJECT_STATE_ROWS * cols, 0.0);
	for (size_t i = 0; i < cols; i++) {
		double x[saip::LINK_OBJECT_STATE_ROWS];
		for (int r = 0; r < saip::LINK_OBJECT_STATE_ROWS; r++) x[r] = per_instance ? state[(size_t)r * cols + i] : state[r];
		const double n = std::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
		if (!(n > 0) || !std::isfinite(n)) {
			if (per_instance) snprintf(msg, len, "instance %zu: the quaternion is zero or not finite", i);
			else snprintf(msg, len, "the quaternion is zero or not finite");
			return false;
		}
		for (int r = 3; r < 7; r++) x[r] /= n;
		for (int r = 0; r < saip::LINK_OBJECT_STATE_ROWS; r++) out[(size_t)r * cols + i] = x[r];
	}
	return true;
}
extern "C" saip_status saip_batch_link_object_attach(saip_batch* b, int n_spheres, const double* centres, const double* radii, const double* material,
													 const double* inertial, int per_instance) {
	const char* fn = "saip_batch_link_object_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	const int P = n_spheres;
	if (P < 1 || P > saip::LINK_OBJECT_MAX_SPHERES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d spheres required (got %d)", fn, saip::LINK_OBJECT_MAX_SPHERES, P);
	if (!centres || !radii) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null centres or radii", fn);
	if (!material) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null material", fn);
	if (!inertial) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null inertial words", fn);
	per_instance = per_instance ? 1 : 0;
	for (int s = 0; s < P; s++) {
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(centres[3 * s + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the centre is not finite", fn, s);
		if (!std::isfinite(radii[s])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the radius is not finite", fn, s);
		if (radii[s] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: radius %g below 0", fn, s, radii[s]);
	}
	char msg[200];
	if (!link_contact_check_materials(material, 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (!link_object_check_inertial(inertial, per_instance ? (size_t)b->B : 1, per_instance, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// (the arguments first: a configuration-only batch, which can hold no link contact, still reports them)
	if (!b->link_contact.attached) return fail(SAIP_ERR_ORDER, "%s: no link contact is attached (saip_batch_link_contact_attach first: the object is its second stage)", fn);
	if (b->link_object.attached) return fail(SAIP_ERR_ORDER, "%s: a link object is already attached (saip_batch_link_object_detach first)", fn);
	if ((st = need_ready(b, fn))) return st;
	auto& J = b->link_object;
	J = saip_batch::LinkObject();
	saip::LinkObjectGeom& G = J.geom;
	memset(&G, 0, sizeof(G));
	G.P = P;
	for (int s = 0; s < P; s++) {
		for (int e = 0; e < 3; e++) G.r[s][e] = centres[3 * s + e];
		G.radius[s] = radii[s];
	}
	for (int k = 0; k < saip::LINK_CONTACT_MATERIAL_WORDS; k++) G.mat[k] = material[k];
	auto upload_geom = [&]() -> saip_status {
		HIP_TRY(hipMalloc((void**)&J.geom_dev, sizeof(G)));
		HIP_TRY(hipMemcpyAsync(J.geom_dev, &G, sizeof(G), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
		return SAIP_OK;
	};
	// the state at attach: the body frame on the world frame, at rest
	std::vector<double> x0((size_t)saip::LINK_OBJECT_STATE_ROWS * b->B, 0.0);
	for (int i = 0; i < b->B; i++) x0[(size_t)3 * b->B + i] = 1.0;
	const size_t ld = b->ld;
	if ((st = upload_geom()) || (st = alloc_zero(b, &J.inertial, (size_t)saip::LINK_OBJECT_INERTIAL_WORDS * (per_instance ? ld : 1))) ||
		(st = alloc_zero(b, &J.state, (size_t)saip::LINK_OBJECT_STATE_ROWS * ld)) || (st = alloc_zero(b, &J.readout, (size_t)saip::LINK_OBJECT_READOUT_ROWS * ld)) ||
		(st = alloc_zero(b, &J.summary, (size_t)saip::LINK_OBJECT_SUMMARY_ROWS * ld)) ||
		(st = upload_table(b, J.inertial, inertial, saip::LINK_OBJECT_INERTIAL_WORDS, per_instance, "inertial", fn)) ||
		(st = upload_table(b, J.state, x0.data(), saip::LINK_OBJECT_STATE_ROWS, 1, "state", fn))) {
		link_object_free(b);
		return st;
	}
	J.attached = true;
	J.per_instance = per_instance;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_object_detach(saip_batch* b) {
	const char* fn = "saip_batch_link_object_detach";
	saip_status st = need_link_object(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a substep may still be in flight
	link_object_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_object_info(saip_batch* b, int* n_spheres, int* per_instance) {
	saip_status st = need_link_object(b, "saip_batch_link_object_info");
	if (st) return st;
	if (n_spheres) *n_spheres = b->link_object.geom.P;
	if (per_instance) *per_instance = b->link_object.per_instance;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_object_set_state_host(saip_batch* b, const double* state, int per_instance) {
	const char* fn = "saip_batch_link_object_set_state_host";
	saip_status st = need_link_object(b, fn);
	if (st) return st;
	if (!state) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null state", fn);
	char msg[200];
	std::vector<double> x;
	if (!link_object_prepare_state(state, per_instance ? (size_t)b->B : 1, per_instance != 0, x, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	if (!per_instance) {  // one column for all
		std::vector<double> all((size_t)saip::LINK_OBJECT_STATE_ROWS * b->B);
		for (int r = 0; r < saip::LINK_OBJECT_STATE_ROWS; r++)
			for (int i = 0; i < b->B; i++) all[(size_t)r * b->B + i] = x[r];
		x.swap(all);
	}
	return upload_table(b, b->link_object.state, x.data(), saip::LINK_OBJECT_STATE_ROWS, 1, "state", fn);
}
extern "C" saip_status saip_batch_link_object_set_inertial_host(saip_batch* b, const double* inertial) {
	const char* fn = "saip_batch_link_object_set_inertial_host";
	saip_status st = need_link_object(b, fn);
	if (st) return st;
	const auto& J = b->link_object;
	if (!inertial) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null inertial words", fn);
	char msg[200];
	if (!link_object_check_inertial(inertial, J.per_instance ? (size_t)b->B : 1, J.per_instance, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return upload_table(b, J.inertial, inertial, saip::LINK_OBJECT_INERTIAL_WORDS, J.per_instance, "inertial", fn);
}
extern "C" double* saip_batch_link_object_state_device(saip_batch* b) { return b ? b->link_object.state : nullptr; }
extern "C" double* saip_batch_link_object_readout_device(saip_batch* b) { return b ? b->link_object.readout : nullptr; }
extern "C" double* saip_batch_link_object_summary_device(saip_batch* b) { return b ? b->link_object.summary : nullptr; }
extern "C" saip_status saip_batch_link_object_state_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_link_object_state_host";
	const saip_status st = need_link_object(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->link_object.state, saip::LINK_OBJECT_STATE_ROWS, fn);
}
extern "C" saip_status saip_batch_link_object_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_link_object_readout_host";
	const saip_status st = need_link_object(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->link_object.readout, saip::LINK_OBJECT_READOUT_ROWS, fn);
}
extern "C" saip_status saip_batch_link_object_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_link_object_summary_host";
	const saip_status st = need_link_object(b, fn);
	return rows_to_host(b, st, out, st ? nullptr : b->link_object.summary, saip::LINK_OBJECT_SUMMARY_ROWS, fn);
}
static_assert(saip::LINK_OBJECT_SUMMARY_ROWS == saip::LINK_CONTACT_SUMMARY_ROWS, "the reset kernel of link contact zeroes the object's summaries too");
extern "C" saip_status saip_batch_link_object_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_link_object_summary_reset";
	saip_status st = need_link_object(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_link_contact_summary_reset(b->B, b->ld, b->link_object.summary, b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_link_object_add_cost(saip_batch* b, const double* target_p, double w_pos, const double* target_quat, double w_ori) {
	const char* fn = "saip_batch_link_object_add_cost";
	saip_status st = need_link_object(b, fn);
	if (st) return st;
	if (b->n_samp == 0) return fail(SAIP_ERR_ORDER, "%s: no sampler is attached (saip_batch_sampler_attach): there is no cost to add to", fn);
	if (!target_p) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null target position", fn);
	for (int e = 0; e < 3; e++)
		if (!std::isfinite(target_p[e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the target position is not finite", fn);
	if (w_pos != w_pos || w_ori != w_ori) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a weight is NaN", fn);
	double tq[4];
	if (target_quat) {
		const double n = std::sqrt(target_quat[0] * target_quat[0] + target_quat[1] * target_quat[1] + target_quat[2] * target_quat[2] + target_quat[3] * target_quat[3]);
		if (!(n > 0) || !std::isfinite(n)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the target quaternion is zero or not finite", fn);
		for (int i = 0; i < 4; i++) tq[i] = target_quat[i] / n;
	}
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_link_object_add_cost(b->B, b->ld, b->link_object.state, b->samp_cost, target_p, w_pos, target_quat ? tq : nullptr, w_ori, b->stream));
	return SAIP_OK;
}
