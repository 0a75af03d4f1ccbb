// Link contact of the resident simulator: up to 16 world-fixed obstacles push back on up to 32 link spheres, at the resident state q, dq, in
// front of an integration substep (arithmetic: saip_link_contact.h).
//   EVALUATE  writes the readout [8][ld] (and, when kept, centres, velocities and F_s [9 S][ld])
//   APPLY     also writes tau_sim = tau_cmd (NaN -> 0) + sum_s J_v(c_s)^T F_s and advances the running summaries [4][ld]
// Nothing else is touched: no state, torque, status, goal or recorder array; columns B..ld-1 are never written.
//   saip_link_contact_add_cost adds the summaries to the sampler's cost, saip_link_contact_summary_reset zeroes them, one lane per instance.
//
// As in saip_clearance.hip an instance gets eight lanes and a block of 64 threads serves eight instances (thread t is lane t & 7 of group
// t >> 3).  This kernel runs once per SUBSTEP, so nothing inside its serial loops waits for global memory: the geometry, the eight
// instances' q and dq columns, their obstacle rows and the materials are staged in the LDS first, by loads that do not depend on one
// another.  What the loops still read from global memory are the model's per-joint constants, batch-uniform.
//   phase 1   every lane walks (SAIP_FK_JOINT_STEP + SAIP_FK_TWIST_STEP) and stores centre and velocity of its share of the sorted spheres,
//             and the world axis and origin of the joints it is responsible for: on a chain lane l stores joints l, l + 8, ... as the walk
//             passes them, on a tree the walk of sorted position owner[j] stores joint j.  No per-joint array lives in registers.
//   phase 2   lc_lane: the lane's spheres x obstacles; F_s and the flag go to the LDS, the readout partials fold by cross-lane moves
//   phase 3   lane l takes joints l, l + 8, ... over the sorted spheres and writes tau_sim
#include <hip/hip_runtime.h>

#include "saip_fk.h"
#include "saip_link_contact.h"
#include "saip_link_object.h"

namespace saip {

static_assert(LINK_CONTACT_MAX_JOINTS == SAIP_MAXN, "the joint vectors of the LDS are sized for SAIP_MAXN joints");
static_assert(sizeof(LinkContactGeom) % sizeof(double) == 0, "the geometry is staged by doubles");

namespace {

enum { LC_G = LINK_CONTACT_GROUPS, LC_L = LINK_CONTACT_LANES, LC_GEOM_DOUBLES = sizeof(LinkContactGeom) / sizeof(double) };

// what a block keeps in the LDS: 5 vectors x 6 KB, q and dq 4 KB, obstacles 8 KB, flags 1 KB, materials 0.5 KB, geometry 1.5 KB: 46 096 bytes
struct LinkContactShared {
	double C[LINK_CONTACT_VEC_WORDS], V[LINK_CONTACT_VEC_WORDS], F[LINK_CONTACT_VEC_WORDS];  // per sorted sphere: centre, velocity, F_s
	double JA[LINK_CONTACT_VEC_WORDS], JO[LINK_CONTACT_VEC_WORDS];                            // per joint: world axis, origin
	double Q[SAIP_MAXN * LC_G], DQ[SAIP_MAXN * LC_G];                                         // [n][8]
	double OB[LINK_CONTACT_MAX_OBSTACLES * LINK_CONTACT_OBSTACLE_WORDS * LC_G];               // [O][8][8], or [O][8] when batch-uniform
	double MAT[LINK_CONTACT_MAX_OBSTACLES * LINK_CONTACT_MATERIAL_WORDS];
	int A[LINK_CONTACT_FLAG_WORDS];
	union {
		LinkContactGeom G;
		double words[LC_GEOM_DOUBLES];
	} geom;
};

// Sphere i of the sorted list, carried by the body whose rotation, origin and twist accumulators are R, o, tv, tw, tc
__device__ __forceinline__ void lc_emit(const LinkContactParams& P, LinkContactShared& sh, const int g, const int col, const int i, const double* R, const double* o,
										const double* tv, const double* tw, const double* tc) {
	const LinkContactGeom& G = sh.geom.G;
	double c[3], v[3];
	cl_centre(o, R, G.r[i], c);
	ct_velocity(tv, tw, tc, c, v);
	const int s = G.slot[i];
	for (int e = 0; e < 3; e++) {
		sh.C[cl_centre_index(i, e, g)] = c[e];
		sh.V[cl_centre_index(i, e, g)] = v[e];
		if (P.keep) {
			P.keep[(size_t)(3 * s + e) * P.ld + col] = c[e];
			P.keep[(size_t)(3 * (G.S + s) + e) * P.ld + col] = v[e];
		}
	}
}

// statement of SAIP_FK_JOINT_STEP: the twist accumulators, and the joint's world axis and origin to the LDS when `store_`
#define SAIP_LC_JOINT(store_)                          \
	{                                                  \
		SAIP_FK_TWIST_STEP(dq)                         \
		if (store_)                                    \
			for (int e = 0; e < 3; e++) {              \
				sh.JA[cl_centre_index(j, e, b)] = aw[e]; \
				sh.JO[cl_centre_index(j, e, b)] = o[e];  \
			}                                          \
	}

// phase 1 for one lane.  q, dq, ld, b are the names the walk macros read the state by: here the staged columns [n][8] and the group.
template <bool TREE>
__device__ __forceinline__ void lc_walk(const LinkContactParams& P, LinkContactShared& sh, const ModelDev& md, const int lane, const int b, const int col) {
	const LinkContactGeom& G = sh.geom.G;
	const double *q = sh.Q, *dq = sh.DQ;
	constexpr int ld = LC_G;
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0}, tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
	if constexpr (TREE) {
		// as saip_clearance.hip: a lane takes a run of neighbours of the sorted list and continues a walk where the body it stands on is an
		// ancestor of the next one.  Joint j is stored by the walk to its lowest sorted position owner[j]: that walk passes j, because no
		// earlier sphere of the run is moved by j, so a continued walk stands in front of it.
		const int run = (G.S + LC_L - 1) / LC_L;
		int at = -1;  // the body R, o and the accumulators belong to
		for (int i = lane * run; i < (lane + 1) * run && i < G.S; i++) {
			const int body = G.body[i];
			if (body != at) {
				const uint32_t anc = G.anc[i];
				if (at >= 0 && !((anc >> at) & 1u)) {
					for (int e = 0; e < 9; e++) R[e] = (e & 3) ? 0.0 : 1.0;
					for (int e = 0; e < 3; e++) o[e] = tv[e] = tw[e] = tc[e] = 0.0;
					at = -1;
				}
				for (int j = at + 1; j <= body; j++) {
					if (!((anc >> j) & 1u)) continue;
					SAIP_FK_JOINT_STEP(SAIP_LC_JOINT(G.owner[j] == i))
				}
				at = body;
			}
			lc_emit(P, sh, b, col, i, R, o, tv, tw, tc);
		}
	} else {
		// every lane walks the chain up to the last body that carries a sphere, stores spheres lane, lane + 8, ... of the sorted list as the
		// walk passes their body, and joints lane, lane + 8, ...
		int i = lane;
		for (; i < G.S && G.body[i] < 0; i += LC_L) lc_emit(P, sh, b, col, i, R, o, tv, tw, tc);  // links welded to the fixed base
		for (int j = 0; j <= G.jmax; j++) {
			SAIP_FK_JOINT_STEP(SAIP_LC_JOINT((j & (LC_L - 1)) == lane))
			for (; i < G.S && G.body[i] == j; i += LC_L) lc_emit(P, sh, b, col, i, R, o, tv, tw, tc);
		}
	}
}

// ---- what saip_link_contact_apply and saip_link_object_apply share besides the walk: each written once
// staging: independent loads, eight consecutive doubles of a row per instance array (thread t: column t & 7, rows t >> 3, + 8, ...); and
// the commanded torques of this lane's joints lane, lane + 8, ... (APPLY: requested now, used in phase 3)
__device__ __forceinline__ void lc_stage(const LinkContactParams& P, LinkContactShared& sh, const int t, const int lane, const int g, const int b0, const bool live,
										 double* u0) {
	const int ld = P.ld, n = P.n, O = P.O, b = b0 + g;
	for (int w = t; w < LC_GEOM_DOUBLES; w += 64) sh.geom.words[w] = ((const double*)P.geom)[w];
	{
		const bool in = b0 + lane < P.B;
		for (int r = g; r < n; r += LC_G) {
			sh.Q[r * LC_G + lane] = in ? P.q[(size_t)r * ld + b0 + lane] : 0.0;
			sh.DQ[r * LC_G + lane] = in ? P.dq[(size_t)r * ld + b0 + lane] : 0.0;
		}
	}
	if (P.per_instance) {
		const bool in = b0 + lane < P.B;
		for (int r = g; r < O * LINK_CONTACT_OBSTACLE_WORDS; r += LC_G) sh.OB[r * LC_G + lane] = in ? P.obst[(size_t)r * ld + b0 + lane] : 0.0;
	} else {
		for (int w = t; w < O * LINK_CONTACT_OBSTACLE_WORDS; w += 64) sh.OB[w] = P.obst[w];
	}
	if (t < O * LINK_CONTACT_MATERIAL_WORDS) sh.MAT[t] = P.mat[t];
#pragma unroll
	for (int r = 0; r < SAIP_MAXN / LC_L; r++) {
		const int j = lane + LC_L * r;
		u0[r] = (P.mode == LINK_CONTACT_APPLY && live && j < n) ? lc_u0(P.tau_cmd[(size_t)j * ld + b]) : 0.0;
	}
}
// what the lanes of group g read in phase 2: the staged tables
__device__ __forceinline__ LinkContactView lc_view(const LinkContactParams& P, const LinkContactShared& sh, const int g) {
	LinkContactView W;
	W.S = P.S;
	W.O = P.O;
	W.slot = sh.geom.G.slot;
	W.radius = sh.geom.G.radius;
	W.obst = sh.OB;
	W.stride = P.per_instance ? LC_G : 1;
	W.col = P.per_instance ? g : 0;
	W.mat = sh.MAT;
	return W;
}
// the fold over the group: cross-lane moves, no LDS traffic and no atomics (lanes off.. of the group fold with themselves: their values
// are not used again)
__device__ __forceinline__ void lc_fold_group(LinkContactPartial& v) {
	for (int off = LC_L / 2; off >= 1; off >>= 1) {
		LinkContactPartial w;
		for (int e = 0; e < 3; e++) w.f[e] = __shfl_down(v.f[e], off, LC_L);
		w.dmin = __shfl_down(v.dmin, off, LC_L);
		w.fn_sum = __shfl_down(v.fn_sum, off, LC_L);
		w.fmax = __shfl_down(v.fmax, off, LC_L);
		w.k = __shfl_down(v.k, off, LC_L);
		w.active = __shfl_down(v.active, off, LC_L);
		w.bad = __shfl_down(v.bad, off, LC_L);
		lc_fold(&v, w);
	}
}
// F_s of this lane's spheres to the kept array
__device__ __forceinline__ void lc_keep_forces(const LinkContactParams& P, const LinkContactShared& sh, const int lane, const int g, const int b) {
	const int S = P.S;
	if (P.keep)
		for (int i = lane; i < S; i += LC_L)
			for (int e = 0; e < 3; e++) P.keep[(size_t)(3 * (2 * S + sh.geom.G.slot[i]) + e) * P.ld + b] = sh.F[cl_centre_index(i, e, g)];
}
// phase 3: the torques of joints lane, lane + 8, ...; run: the group's verdict "valid and something active"
__device__ __forceinline__ void lc_torques(const LinkContactParams& P, const LinkContactShared& sh, const int lane, const int g, const int b, const int run,
										   const double* u0) {
	const LinkContactGeom& G = sh.geom.G;
	const int n = P.n, S = P.S;
#pragma unroll
	for (int r = 0; r < SAIP_MAXN / LC_L; r++) {
		const int j = lane + LC_L * r;
		if (j >= n) continue;
		double tau = u0[r];
		if (run) {
			double x = 0.0;
			if (G.owner[j] >= 0) {
				const double aw[3] = {sh.JA[cl_centre_index(j, 0, g)], sh.JA[cl_centre_index(j, 1, g)], sh.JA[cl_centre_index(j, 2, g)]};
				const double oj[3] = {sh.JO[cl_centre_index(j, 0, g)], sh.JO[cl_centre_index(j, 1, g)], sh.JO[cl_centre_index(j, 2, g)]};
				x = lc_joint_sum(S, G.anc, j, P.model->jtype[j], aw, oj, sh.C, sh.F, sh.A, g);
			}
			tau = lc_tau(tau, x);
		}
		P.tau_sim[(size_t)j * P.ld + b] = tau;
	}
}

}  // namespace

template <bool TREE>
__global__ void __launch_bounds__(64) saip_link_contact_apply(const LinkContactParams P) {
	__shared__ LinkContactShared sh;
	const int t = threadIdx.x, lane = t & (LC_L - 1), g = t >> 3;
	const int b0 = blockIdx.x * LC_G, b = b0 + g;
	const bool live = b < P.B;  // (a lane of a group past the batch still has to reach the barriers)
	const int ld = P.ld;
	double u0[SAIP_MAXN / LC_L];
	lc_stage(P, sh, t, lane, g, b0, live, u0);
	__syncthreads();
	// ---- phase 1: centres, velocities, joint axes and origins
	if (live) lc_walk<TREE>(P, sh, *P.model, lane, g, b);
	__syncthreads();
	// ---- phase 2: the items of this lane, then the fold over the group
	LinkContactPartial v = {{0.0, 0.0, 0.0}, INFINITY, 0.0, 0.0, -1, 0, 0};
	if (live) lc_lane(lc_view(P, sh, g), sh.C, sh.V, sh.F, sh.A, g, lane, &v);
	lc_fold_group(v);
	const int run = __shfl((!v.bad && v.active > 0) ? 1 : 0, 0, LC_L);  // lane 0's verdict for the whole group: does the torque loop run?
	__syncthreads();
	if (!live) return;
	lc_keep_forces(P, sh, lane, g, b);
	if (lane == 0) {
		double ro[LINK_CONTACT_READOUT_ROWS];
		lc_readout(v, ro);
		for (int r = 0; r < LINK_CONTACT_READOUT_ROWS; r++) P.readout[(size_t)r * ld + b] = ro[r];
		if (P.mode == LINK_CONTACT_APPLY) lc_summary_advance(P.summary + b, ld, P.dt, ro);
	}
	if (P.mode != LINK_CONTACT_APPLY) return;
	lc_torques(P, sh, lane, g, b, run, u0);
}

// ---- the pushed object (saip_link_object.h): the launch that replaces the one above while an object is attached.  The same walk, lanes,
// blocks and staging; on top of them the object's 13 state words, its inertial words and its shape are staged with the other independent
// loads, lane p < P forms c_p and v_p of object sphere p in phase 1 (they live in the LDS beside C and V), phase 2 is lo_lane (the robot
// spheres of the lane against the obstacles, then against the object spheres) and, on lane p < P, lo_world (object sphere p against the
// obstacles); both partials fold by cross-lane moves and lane 0 integrates the body and writes its new state, rows of [ld].  No atomics,
// and nothing inside the item loops reads global memory.
namespace {
enum { LO_GEOM_DOUBLES = sizeof(LinkObjectGeom) / sizeof(double) };
static_assert(sizeof(LinkObjectGeom) % sizeof(double) == 0, "the shape is staged by doubles");
// 46 096 bytes of link contact + 2 x 1.5 KB object sphere vectors, 832 B state, 256 B inertial words, 296 B shape: 50 552 bytes
struct LinkObjectShared {
	LinkContactShared lc;
	double OC[LINK_OBJECT_VEC_WORDS], OV[LINK_OBJECT_VEC_WORDS];  // per object sphere: centre, velocity
	double X[LINK_OBJECT_STATE_ROWS * LC_G];                      // [13][8]
	double IN[LINK_OBJECT_INERTIAL_WORDS * LC_G];                 // [4][8]
	union {
		LinkObjectGeom G;
		double words[LO_GEOM_DOUBLES];
	} og;
};
}  // namespace

template <bool TREE>
__global__ void __launch_bounds__(64) saip_link_object_apply(const LinkObjectParams Q) {
	__shared__ LinkObjectShared so;
	LinkContactShared& sh = so.lc;
	const LinkContactParams& P = Q.lc;
	const int t = threadIdx.x, lane = t & (LC_L - 1), g = t >> 3;
	const int b0 = blockIdx.x * LC_G, b = b0 + g;
	const bool live = b < P.B;
	const int ld = P.ld;
	// ---- staging: link contact's, and the object's words
	double u0[SAIP_MAXN / LC_L];
	lc_stage(P, sh, t, lane, g, b0, live, u0);
	if (t < LO_GEOM_DOUBLES) so.og.words[t] = ((const double*)Q.geom)[t];
	{
		const bool in = b0 + lane < P.B;
		for (int r = g; r < LINK_OBJECT_STATE_ROWS; r += LC_G) so.X[r * LC_G + lane] = in ? Q.state[(size_t)r * ld + b0 + lane] : 0.0;
		if (g < LINK_OBJECT_INERTIAL_WORDS) so.IN[g * LC_G + lane] = Q.inertial_per_instance ? (in ? Q.inertial[(size_t)g * ld + b0 + lane] : 1.0) : Q.inertial[g];
	}
	__syncthreads();
	const LinkObjectGeom& OG = so.og.G;
	// ---- phase 1: the robot's walk, and the object spheres
	double x[LINK_OBJECT_STATE_ROWS];
	for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) x[r] = so.X[r * LC_G + g];
	if (live) {
		lc_walk<TREE>(P, sh, *P.model, lane, g, b);
		if (lane < OG.P) {
			double R[9], c[3], v[3];
			lo_rotation(x + 3, R);
			lo_sphere(x, R, OG.r[lane], c, v);
			for (int e = 0; e < 3; e++) {
				so.OC[lo_index(lane, e, g)] = c[e];
				so.OV[lo_index(lane, e, g)] = v[e];
			}
		}
	}
	__syncthreads();
	// ---- phase 2: the items of this lane, then the two folds over the group
	LinkContactPartial v = {{0.0, 0.0, 0.0}, INFINITY, 0.0, 0.0, -1, 0, 0};
	LinkObjectPartial q;
	lo_partial_clear(&q);
	if (live) {
		const LinkContactView W = lc_view(P, sh, g);
		lo_lane(W, OG, sh.C, sh.V, so.OC, so.OV, x, sh.F, sh.A, g, lane, &v, &q);
		if (lane < OG.P) lo_world(W, OG, so.OC, so.OV, x, g, lane, &q);
	}
	lc_fold_group(v);
	for (int off = LC_L / 2; off >= 1; off >>= 1) {
		LinkObjectPartial y;
		for (int e = 0; e < 3; e++) {
			y.rf[e] = __shfl_down(q.rf[e], off, LC_L);
			y.rm[e] = __shfl_down(q.rm[e], off, LC_L);
			y.wf[e] = __shfl_down(q.wf[e], off, LC_L);
			y.wm[e] = __shfl_down(q.wm[e], off, LC_L);
		}
		y.dmin = __shfl_down(q.dmin, off, LC_L);
		y.fn_sum = __shfl_down(q.fn_sum, off, LC_L);
		y.wpen = __shfl_down(q.wpen, off, LC_L);
		y.k = __shfl_down(q.k, off, LC_L);
		y.active = __shfl_down(q.active, off, LC_L);
		lo_fold(&q, y);
	}
	const bool bad = v.bad || !lo_state_finite(x);  // (lane 0's word counts)
	const int run = __shfl((!bad && v.active + q.active > 0) ? 1 : 0, 0, LC_L);
	__syncthreads();
	if (!live) return;
	lc_keep_forces(P, sh, lane, g, b);
	if (lane == 0) {
		double ro[LINK_CONTACT_READOUT_ROWS], rq[LINK_OBJECT_READOUT_ROWS];
		lc_readout(v, ro);
		for (int r = 0; r < LINK_CONTACT_READOUT_ROWS; r++) P.readout[(size_t)r * ld + b] = ro[r];
		lo_readout(q, bad, rq);
		for (int r = 0; r < LINK_OBJECT_READOUT_ROWS; r++) Q.readout[(size_t)r * ld + b] = rq[r];
		if (P.mode == LINK_CONTACT_APPLY) {
			lc_summary_advance(P.summary + b, ld, P.dt, ro);
			lo_summary_advance(Q.summary + b, ld, P.dt, q, bad);
			if (!bad) {
				double in[LINK_OBJECT_INERTIAL_WORDS], xn[LINK_OBJECT_STATE_ROWS];
				for (int r = 0; r < LINK_OBJECT_INERTIAL_WORDS; r++) in[r] = so.IN[r * LC_G + g];
				lo_integrate(x, in, Q.gravity, P.dt, q, xn);
				for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) Q.state[(size_t)r * ld + b] = xn[r];
			}
		}
	}
	if (P.mode != LINK_CONTACT_APPLY) return;
	lc_torques(P, sh, lane, g, b, run, u0);
}

// cost[i] += w_pos |p - target|^2 + w_ori (1 - (q . q_t)^2) on the sampler's cost, one lane per instance
__global__ void __launch_bounds__(64) saip_link_object_add_cost(const int B, const int ld, const double* state, double* cost, const double tx, const double ty,
																 const double tz, const double w_pos, const int has_quat, const double q0, const double q1, const double q2,
																 const double q3, const double w_ori) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	double x[LINK_OBJECT_STATE_ROWS];
	for (int r = 0; r < LINK_OBJECT_STATE_ROWS; r++) x[r] = state[(size_t)r * ld + b];
	const double tp[3] = {tx, ty, tz}, tq[4] = {q0, q1, q2, q3};
	cost[b] = lo_add_cost(cost[b], x, tp, w_pos, tq, has_quat != 0, w_ori);
}

__global__ void __launch_bounds__(64) saip_link_contact_add_cost(const int B, const int ld, const double* summary, double* cost, const double w_impulse,
																 const double w_peak) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	cost[b] = lc_add_cost(cost[b], summary[b], summary[(size_t)ld + b], w_impulse, w_peak);
}

// the summaries of an attachment that has integrated no substep: zeros (columns B..ld-1 stay as they are, which a memset would not leave)
__global__ void __launch_bounds__(64) saip_link_contact_summary_reset(const int B, const int ld, double* summary) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	for (int r = 0; r < LINK_CONTACT_SUMMARY_ROWS; r++) summary[(size_t)r * ld + b] = 0.0;
}

hipError_t launch_link_contact_apply(const LinkContactParams& P, bool tree, hipStream_t stream) {
	const dim3 grid((P.B + LC_G - 1) / LC_G);
	if (tree) hipLaunchKernelGGL(saip_link_contact_apply<true>, grid, dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_link_contact_apply<false>, grid, dim3(64), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_link_object_apply(const LinkObjectParams& Q, bool tree, hipStream_t stream) {
	const dim3 grid((Q.lc.B + LC_G - 1) / LC_G);
	if (tree) hipLaunchKernelGGL(saip_link_object_apply<true>, grid, dim3(64), 0, stream, Q);
	else hipLaunchKernelGGL(saip_link_object_apply<false>, grid, dim3(64), 0, stream, Q);
	return hipGetLastError();
}

hipError_t launch_link_object_add_cost(int B, int ld, const double* state, double* cost, const double* tp, double w_pos, const double* tq, double w_ori, hipStream_t stream) {
	hipLaunchKernelGGL(saip_link_object_add_cost, dim3((B + 63) / 64), dim3(64), 0, stream, B, ld, state, cost, tp[0], tp[1], tp[2], w_pos, tq ? 1 : 0, tq ? tq[0] : 0.0,
					   tq ? tq[1] : 0.0, tq ? tq[2] : 0.0, tq ? tq[3] : 0.0, w_ori);
	return hipGetLastError();
}

hipError_t launch_link_contact_add_cost(int B, int ld, const double* summary, double* cost, double w_impulse, double w_peak, hipStream_t stream) {
	hipLaunchKernelGGL(saip_link_contact_add_cost, dim3((B + 63) / 64), dim3(64), 0, stream, B, ld, summary, cost, w_impulse, w_peak);
	return hipGetLastError();
}

hipError_t launch_link_contact_summary_reset(int B, int ld, double* summary, hipStream_t stream) {
	hipLaunchKernelGGL(saip_link_contact_summary_reset, dim3((B + 63) / 64), dim3(64), 0, stream, B, ld, summary);
	return hipGetLastError();
}

}  // namespace saip
