// The clearance monitor of the resident simulator: signed distances of up to 32 link spheres to up to 16 world-fixed obstacles and over up
// to 64 self pairs, at the resident state q (arithmetic: saip_clearance.h).
//   EVALUATE  writes the readout [8][ld] (and, when kept, the centres [3 S][ld])
//   MONITOR   also advances the running summaries [4][ld] by one period
// Nothing else is touched: no state, torque, status, goal or recorder array; columns B..ld-1 are never written.
//   saip_clearance_add_cost adds the summaries to the sampler's cost, one lane per instance.
//
// The work of an instance is S x O + P items, not a fixed handful of terms, so an instance gets eight lanes: a block of 64 threads serves
// eight instances (groups of eight consecutive lanes; thread t is lane t & 7 of group t >> 3).  Per row of q, of a per-instance obstacle
// table and of every output a block touches eight consecutive doubles (a 64-byte run); the batch-uniform tables are the same words for
// every group.
#include <hip/hip_runtime.h>

#include "saip_clearance.h"
#include "saip_fk.h"

namespace saip {

namespace {

// Sphere i of the sorted list, carried by the body whose rotation and origin are R, o: its centre goes to the LDS (and to the kept centres).
__device__ __forceinline__ void clearance_emit(const ClearanceParams& P, const ClearanceGeom& G, double* C, const int g, const int b, const int i,
											   const double* R, const double* o) {
	double c[3];
	cl_centre(o, R, G.r[i], c);
	const int s = G.slot[i];
	for (int e = 0; e < 3; e++) {
		C[cl_centre_index(s, e, g)] = c[e];
		if (P.centres) P.centres[(size_t)(3 * s + e) * P.ld + b] = c[e];
	}
}

}  // namespace

template <bool TREE>
__global__ void __launch_bounds__(64) saip_clearance_eval(const ClearanceParams P) {
	// The centres of the block's eight instances: 3 planes x 256 doubles = 6 KB.  Component e of sphere s of group g sits at double
	//   e * 256 + (s / 8) * 64 + (g / 4) * 32 + (g % 4) * 8 + (s % 8)                                       (cl_centre_index)
	// A 64-bit LDS read is served one 32-lane half at a time, over 32 banks of eight bytes: bank = double index mod 32 = (g % 4) * 8 + (s % 8).
	// A half holds four groups (g / 4 is the half), so the groups of a half own disjoint octets of banks, and within a group the eight
	// lanes of a sphere x obstacle step read the spheres of eight consecutive items k: either one sphere (the same address: a broadcast)
	// or up to eight CONSECUTIVE spheres, which differ in s % 8.  Those reads are conflict-free for every S and O.  The two reads of a
	// self-pair item go where the caller's pair list sends them and may collide within a group; there are at most 64 / 8 such steps.
	__shared__ double C[CLEARANCE_CENTRE_WORDS];
	const int lane = threadIdx.x & (CLEARANCE_LANES - 1), g = threadIdx.x >> 3;
	const int b = blockIdx.x * CLEARANCE_GROUPS + g;
	const bool live = b < P.B;  // (a lane of a group past the batch still has to reach the barrier)
	const ClearanceGeom& G = *P.geom;
	const ModelDev& md = *P.model;
	const double* q = P.q;
	const int ld = P.ld;
	// ---- phase 1: the world centres.  The walk is serial; the eight lanes of a group would idle while one walked, so each walks for itself
	if (live) {
		double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
		if constexpr (TREE) {
			// a lane takes a run of neighbours of the sorted list (they share bodies, hence walks): per sphere the walk over the ancestors of
			// its body, continued from where it stands when the body it stands on is one of them, restarted at the base otherwise
			const int run = (G.S + CLEARANCE_LANES - 1) / CLEARANCE_LANES;
			int at = -1;  // the body R, o belong to
			for (int i = lane * run; i < (lane + 1) * run && i < G.S; i++) {
				const int body = G.body[i];
				if (body != at) {
					const uint32_t anc = body >= 0 ? md.anc[body] : 0u;
					if (at >= 0 && !((anc >> at) & 1u)) {
						for (int e = 0; e < 9; e++) R[e] = (e & 3) ? 0.0 : 1.0;
						for (int e = 0; e < 3; e++) o[e] = 0.0;
						at = -1;
					}
					for (int j = at + 1; j <= body; j++) {
						if (!((anc >> j) & 1u)) continue;
						SAIP_FK_JOINT_STEP()
					}
					at = body;
				}
				clearance_emit(P, G, C, g, b, i, R, o);
			}
		} else {
			// every lane walks the chain once and stores spheres lane, lane + 8, ... of the sorted list as the walk passes their body
			int i = lane;
			for (; i < G.S && G.body[i] < 0; i += CLEARANCE_LANES) clearance_emit(P, G, C, g, b, i, R, o);  // links welded to the fixed base
			for (int j = 0; i < G.S; j++) {
				SAIP_FK_JOINT_STEP()
				for (; i < G.S && G.body[i] == j; i += CLEARANCE_LANES) clearance_emit(P, G, C, g, b, i, R, o);
			}
		}
	}
	__syncthreads();
	if (!live) return;
	// ---- phase 2: the items of this lane, then the fold over the group: cross-lane moves, no LDS traffic and no atomics
	ClearancePartial v;
	cl_lane(G, P.obst, P.per_instance ? (long long)ld : 1, P.per_instance ? (long long)b : 0, P.margin, C, g, lane, &v);
	for (int off = CLEARANCE_LANES / 2; off >= 1; off >>= 1) {
		ClearancePartial w;
		w.pen = __shfl_down(v.pen, off, CLEARANCE_LANES);
		w.dmin = __shfl_down(v.dmin, off, CLEARANCE_LANES);
		w.pmin = __shfl_down(v.pmin, off, CLEARANCE_LANES);
		w.k = __shfl_down(v.k, off, CLEARANCE_LANES);
		w.under = __shfl_down(v.under, off, CLEARANCE_LANES);
		w.bad = __shfl_down(v.bad, off, CLEARANCE_LANES);
		cl_fold(&v, w);  // (lanes off.. of the group fold with themselves: their values are not used again)
	}
	if (lane != 0) return;
	double ro[CLEARANCE_READOUT_ROWS];
	cl_readout(G, v, C, g, ro);
	for (int r = 0; r < CLEARANCE_READOUT_ROWS; r++) P.readout[(size_t)r * ld + b] = ro[r];
	if (P.mode == CLEARANCE_MONITOR) cl_summary_advance(P.summary + b, ld, P.dt, ro[0], ro[2], P.period);
}

__global__ void __launch_bounds__(64) saip_clearance_add_cost(const int B, const int ld, const double* summary, double* cost, const double w_penalty,
															  const double w_collision, const double d_safe) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	cost[b] = cl_add_cost(cost[b], summary[b], summary[(size_t)ld + b], w_penalty, w_collision, d_safe);
}

// the summaries of a monitor that has seen no period: +inf, 0, 0, -1 (columns B..ld-1 stay as they are)
__global__ void __launch_bounds__(64) saip_clearance_summary_reset(const int B, const int ld, double* summary) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	summary[b] = INFINITY;
	summary[(size_t)ld + b] = 0.0;
	summary[(size_t)2 * ld + b] = 0.0;
	summary[(size_t)3 * ld + b] = -1.0;
}

hipError_t launch_clearance_eval(const ClearanceParams& P, bool tree, hipStream_t stream) {
	const dim3 grid((P.B + CLEARANCE_GROUPS - 1) / CLEARANCE_GROUPS);
	if (tree) hipLaunchKernelGGL(saip_clearance_eval<true>, grid, dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_clearance_eval<false>, grid, dim3(64), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_clearance_add_cost(int B, int ld, const double* summary, double* cost, double w_penalty, double w_collision, double d_safe,
									 hipStream_t stream) {
	hipLaunchKernelGGL(saip_clearance_add_cost, dim3((B + 63) / 64), dim3(64), 0, stream, B, ld, summary, cost, w_penalty, w_collision, d_safe);
	return hipGetLastError();
}

hipError_t launch_clearance_summary_reset(int B, int ld, double* summary, hipStream_t stream) {
	hipLaunchKernelGGL(saip_clearance_summary_reset, dim3((B + 63) / 64), dim3(64), 0, stream, B, ld, summary);
	return hipGetLastError();
}

}  // namespace saip
