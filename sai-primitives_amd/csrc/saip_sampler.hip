// Resident rollout sampler: the three device steps of a sampling-MPC round that used to go through the host (saip.h).
//   saip_sampler_perturb  one lane per instance: the keyframes of every sampled task's schedule rewritten in place around the nominal
//                         plan, noise from a counter-based generator (nothing depends on B, ld or the launch shape)
//   saip_sampler_cost     one lane per instance: one cost per instance from the recorder's summaries and pose log
//   saip_sampler_weights  one workgroup of 256 lanes: minimum, lowest index that attains it, softmin weights, their sums; writes the
//                         weights [B], the result record and the best map [B]
//   saip_sampler_update   one workgroup of 256 lanes per (sampled task, keyframe): the weighted mean of the keyframe's rows (rotations
//                         in the tangent space of the old nominal) becomes the new nominal.  A workgroup reads and writes the nominal
//                         rows of its own keyframe only.
//   saip_sampler_shift    the receding-horizon warm start of the nominal plan
// Scenario groups (B = C M instances: M scenario blocks of C candidates, instance i = s C + c):
//   saip_sampler_group_cost       one lane per candidate: the M scenario costs of a candidate folded into its group cost
//   saip_sampler_weights_grouped  saip_sampler_weights over the C group costs, and the best map over all B instances
// perturb keys the noise by the candidate; update runs unchanged on columns 0 .. C - 1.  With M = 1 neither of the two is launched.
// No atomics, no device-side counter: weights -> update is ordered by the stream, and every sum has the fixed shape stated in
// saip_sampler.h (lane l takes instances l, l + 256, ...; a fixed tree over the lanes), so two runs give the same bits.  Every array row
// is a [ld] run: a wavefront's loads and stores are contiguous; columns B .. ld - 1 are never written.
#include <hip/hip_runtime.h>

#include "saip_sampler.h"

namespace saip {

__global__ void __launch_bounds__(64) saip_sampler_perturb(const SamplerParams P) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.B) return;
	const int c = P.C == P.B ? i : i % P.C;  // (uniform) the candidate this instance rolls out
	for (int t = 0; t < P.n; t++) samp_perturb_candidate(P.e[t], P.ld, i, c, P.seed_lo, P.seed_hi, P.round);
}

// cost [M][C] as rows of the cost array: lane c reads cost[s C + c], contiguous across the wavefront for every s
__global__ void __launch_bounds__(64) saip_sampler_group_cost(const double* __restrict__ cost, int C, int M, int risk, int tail, double* __restrict__ group) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= C) return;
	group[c] = samp_group_cost(cost, C, M, c, risk, tail);
}

__global__ void __launch_bounds__(64) saip_sampler_cost(const SamplerCostParams P) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.B) return;
	P.cost[i] = samp_cost_instance(P, i);
}

// the fold inside a wavefront: after it lane 0 holds the group result of the shape in saip_sampler.h (a lane whose partner lies outside
// the wavefront gets its own value back from the shuffle; such lanes never reach lane 0)
__device__ __forceinline__ double samp_wave_sum(double v) {
	for (int off = SAMP_WAVE / 2; off >= 1; off /= 2) v = v + __shfl_down(v, off, SAMP_WAVE);
	return v;
}
// the sum over the workgroup of one value per lane, returned to every lane; `part` is [4] doubles of LDS
__device__ __forceinline__ double samp_block_sum(double v, double* part) {
	v = samp_wave_sum(v);
	__syncthreads();  // the previous use of `part` has been read
	if (threadIdx.x % SAMP_WAVE == 0) part[threadIdx.x / SAMP_WAVE] = v;
	__syncthreads();
	return (part[0] + part[1]) + (part[2] + part[3]);
}

// GROUPED: B is the number of candidates and the map covers n_map >= B instances in scenario blocks of B
template <bool GROUPED>
__device__ __forceinline__ void samp_weights_body(const double* __restrict__ cost, int B, double temperature, double* __restrict__ w,
												  SamplerResult* __restrict__ res, int* __restrict__ best_map, int n_map) {
	__shared__ double part[4], pm[4];
	__shared__ int pi[4], pn[4];
	const int lane = threadIdx.x;
	double m;
	int im, nv;
	samp_lane_minimum(cost, B, lane, m, im, nv);
	for (int off = SAMP_WAVE / 2; off >= 1; off /= 2) {
		const double om = __shfl_down(m, off, SAMP_WAVE);
		const int oi = __shfl_down(im, off, SAMP_WAVE), on = __shfl_down(nv, off, SAMP_WAVE);
		if (lane % SAMP_WAVE + off < SAMP_WAVE) {
			samp_min_combine(m, im, om, oi);
			nv += on;
		}
	}
	if (lane % SAMP_WAVE == 0) {
		pm[lane / SAMP_WAVE] = m;
		pi[lane / SAMP_WAVE] = im;
		pn[lane / SAMP_WAVE] = nv;
	}
	__syncthreads();
	m = pm[0];
	im = pi[0];
	nv = pn[0];
	for (int g = 1; g < 4; g++) {
		samp_min_combine(m, im, pm[g], pi[g]);
		nv += pn[g];
	}
	double sw = 0.0, sw2 = 0.0;
	if (nv > 0) samp_lane_weights(cost, B, lane, m, temperature, w, sw, sw2);
	else
		for (int i = lane; i < B; i += SAMP_LANES) w[i] = 0.0;
	sw = samp_block_sum(sw, part);
	sw2 = samp_block_sum(sw2, part);
	for (int i = lane; i < B; i += SAMP_LANES) best_map[i] = im;
	if (GROUPED)
		for (int i = B + lane; i < n_map; i += SAMP_LANES) best_map[i] = samp_group_map(i, B, im);
	if (lane == 0) {  // one vector store per field
		res->best = im;
		res->n_valid = nv;
		res->min_cost = nv ? m : 0.0;
		res->sum_w = nv ? sw : 0.0;
		res->ess = nv ? (sw * sw) / sw2 : 0.0;
	}
}

__global__ void __launch_bounds__(SAMP_LANES) saip_sampler_weights(const double* __restrict__ cost, int B, double temperature, double* __restrict__ w,
																	SamplerResult* __restrict__ res, int* __restrict__ best_map) {
	samp_weights_body<false>(cost, B, temperature, w, res, best_map, B);
}
__global__ void __launch_bounds__(SAMP_LANES) saip_sampler_weights_grouped(const double* __restrict__ group, int C, double temperature, double* __restrict__ w,
																			SamplerResult* __restrict__ res, int* __restrict__ best_map, int B) {
	samp_weights_body<true>(group, C, temperature, w, res, best_map, B);
}

__global__ void __launch_bounds__(SAMP_LANES) saip_sampler_update(const SamplerParams P, const double* __restrict__ w, const SamplerResult* __restrict__ res) {
	__shared__ double part[4], tot[4][SAMP_MAX_ROWS];
	if (res->n_valid == 0) return;  // (uniform over the grid) no finite cost: the nominal stays
	const SamplerEntry& E = P.e[blockIdx.y];
	const int k = blockIdx.x, lane = threadIdx.x;
	if (k >= E.K) return;
	double sw = 0.0, sw2 = 0.0;
	{
#pragma clang fp contract(off)
		for (int i = lane; i < P.B; i += SAMP_LANES) {
			sw = sw + w[i];
			sw2 = sw2 + w[i] * w[i];
		}
	}
	sw = samp_block_sum(sw, part);
	sw2 = samp_block_sum(sw2, part);
	double acc[SAMP_MAX_ROWS];
	samp_lane_accumulate(E, k, P.ld, P.B, w, lane, acc);
	for (int j = 0; j < E.d; j++) {
		const double v = samp_wave_sum(acc[j]);
		if (lane % SAMP_WAVE == 0) tot[lane / SAMP_WAVE][j] = v;
	}
	__syncthreads();  // every lane has read the old nominal rows of this keyframe, and the wavefront sums are in LDS
	if (lane == 0) {
		double t[SAMP_MAX_ROWS];
		for (int j = 0; j < E.d; j++) t[j] = (tot[0][j] + tot[1][j]) + (tot[2][j] + tot[3][j]);
		samp_finish_keyframe(E, k, P.ld, t, sw, sw2, res->best);
	}
}

__global__ void __launch_bounds__(64) saip_sampler_shift(const SamplerParams P, int n) {
	for (int t = 0; t < P.n; t++)
		for (int c = threadIdx.x; c < P.e[t].count; c += blockDim.x) samp_shift_column(P.e[t].nominal, P.e[t].K, P.e[t].count, n, c);
}

hipError_t launch_sampler_perturb(const SamplerParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sampler_perturb, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_sampler_cost(const SamplerCostParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sampler_cost, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_sampler_update(const SamplerParams& P, const double* cost, double temperature, double* w, SamplerResult* res, int* best_map, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sampler_weights, dim3(1), dim3(SAMP_LANES), 0, stream, cost, P.B, temperature, w, res, best_map);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	int Kmax = 0;
	for (int t = 0; t < P.n; t++) Kmax = P.e[t].K > Kmax ? P.e[t].K : Kmax;
	hipLaunchKernelGGL(saip_sampler_update, dim3(Kmax, P.n), dim3(SAMP_LANES), 0, stream, P, w, res);
	return hipGetLastError();
}
// P.B = C M with M > 1: group cost, weights over the C group costs with the map over B, update over columns 0 .. C - 1
hipError_t launch_sampler_update_grouped(const SamplerParams& P, const double* cost, int risk, int tail, double* group, double temperature, double* w, SamplerResult* res,
										 int* best_map, hipStream_t stream) {
	const int C = P.C, M = P.B / P.C;
	hipLaunchKernelGGL(saip_sampler_group_cost, dim3((C + 63) / 64), dim3(64), 0, stream, cost, C, M, risk, tail, group);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(saip_sampler_weights_grouped, dim3(1), dim3(SAMP_LANES), 0, stream, (const double*)group, C, temperature, w, res, best_map, P.B);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	SamplerParams Pc = P;  // the update kernel sees a batch of C
	Pc.B = C;
	int Kmax = 0;
	for (int t = 0; t < P.n; t++) Kmax = P.e[t].K > Kmax ? P.e[t].K : Kmax;
	hipLaunchKernelGGL(saip_sampler_update, dim3(Kmax, P.n), dim3(SAMP_LANES), 0, stream, Pc, (const double*)w, (const SamplerResult*)res);
	return hipGetLastError();
}
// Scenario sharing: in `rows` rows of [ld], column i takes the bits of column (i / C) C; source columns and columns B .. ld - 1 stay
__global__ void __launch_bounds__(64) saip_sampler_share_columns(double* __restrict__ a, int rows, int B, int ld, int C) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= B || i % C == 0) return;
	double* row = a + (size_t)blockIdx.y * ld;
	for (int r = blockIdx.y; r < rows; r += gridDim.y, row += (size_t)gridDim.y * ld) row[i] = row[i - i % C];
}
hipError_t launch_sampler_share_columns(double* a, int rows, int B, int ld, int C, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sampler_share_columns, dim3((B + 63) / 64, rows < 1024 ? rows : 1024), dim3(64), 0, stream, a, rows, B, ld, C);
	return hipGetLastError();
}
hipError_t launch_sampler_shift(const SamplerParams& P, int n, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sampler_shift, dim3(1), dim3(64), 0, stream, P, n);
	return hipGetLastError();
}

}  // namespace saip
