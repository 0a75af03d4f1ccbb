// The sensing chain of the resident simulator (arithmetic: saip_sense_chain.h), the stateful second stage of the sensing model.
//   saip_sense_chain_apply      the launch shape of saip_sense_apply.  Rows 0 .. n-1 (SENSE_MODE_JOINTS): se_joint of the true q, dq, then
//                               one sample of the joint's chain; q_meas, dq_meas and the chain state of the (joint, instance) are stored.
//                               Rows n .. (SENSE_MODE_WRENCH): the wrench rows of saip_sense_apply, unchanged.
//   saip_sense_chain_randomize  fills the per-instance chain table with draws between two batch-uniform tables
// The true state is never written, and columns B..ld-1 of no array are written.  Every array is [rows][ld] and a wavefront is 64
// consecutive instances of one row, so each of its loads and stores (the taps included: tap k of the wavefront's joint is one row) is one
// contiguous run.  The taps are copied into locals indexed by unrolled constants only (registers): no scratch.
#include <hip/hip_runtime.h>

#include "saip_sense_chain.h"

namespace saip {

__global__ void __launch_bounds__(64) saip_sense_chain_apply(const SenseChainParams C) {
	const SenseParams& P = C.S;
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const int row = blockIdx.y + ((P.mode & SENSE_MODE_JOINTS) ? 0 : P.n);
	const size_t ld = P.ld;
	if (row >= P.n) {
		se_wrench_rows(P, row, b);
		return;
	}
	const long long js = P.per_instance_joints ? (long long)ld : 1, jc = P.per_instance_joints ? (long long)b : 0;
	const long long cs = C.per_instance ? (long long)ld : 1, cc = C.per_instance ? (long long)b : 0;
	const size_t k = (size_t)row * ld + b;
	double qm, dqm;
	se_joint(P.joints + (long long)row * SENSE_JOINT_WORDS * js + jc, js, P.seed_lo, P.seed_hi, P.period, b, row, P.q[k], P.dq[k], &qm, &dqm);
	double* tq = C.taps + (size_t)(2 * row) * C.depth * ld + b;  // (never dereferenced at depth 0, where taps is null)
	sc_step(C.table + (long long)row * SENSE_CHAIN_WORDS * cs + cc, cs, C.depth, C.sample_time, tq, tq + (size_t)C.depth * ld,
			C.filt + (size_t)row * SENSE_CHAIN_FILT_ROWS * ld + b, C.primed + k, (long long)ld, qm, dqm, &qm, &dqm);
	P.q_meas[k] = qm;
	P.dq_meas[k] = dqm;
}

// One lane per instance, looping over the words: every store of a wavefront is one contiguous run of a row.
__global__ void __launch_bounds__(64) saip_sense_chain_randomize(const SenseChainRandomParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const size_t ld = P.ld;
	for (int w = 0; w < P.n * SENSE_CHAIN_WORDS; w++) P.table[(size_t)w * ld + b] = sc_draw(P.seed_lo, P.seed_hi, P.round, b, w, P.lo[w], P.hi[w], P.depth);
}

hipError_t launch_sense_chain_apply(const SenseChainParams& C, hipStream_t stream) {
	const SenseParams& P = C.S;
	const int rows = ((P.mode & SENSE_MODE_JOINTS) ? P.n : 0) + ((P.mode & SENSE_MODE_WRENCH) ? 3 * P.n_slots : 0);
	if (rows == 0) return hipSuccess;
	hipLaunchKernelGGL(saip_sense_chain_apply, dim3((P.B + 63) / 64, rows), dim3(64), 0, stream, C);
	return hipGetLastError();
}

hipError_t launch_sense_chain_randomize(const SenseChainRandomParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sense_chain_randomize, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
