// The sensing model of the resident simulator (arithmetic: saip_sense.h).
//   saip_sense_apply      elementwise over (row, instance).  Rows 0 .. n-1 (SENSE_MODE_JOINTS): q_meas, dq_meas of one joint from the true
//                         q, dq.  Rows n .. n + 3 slots - 1 (SENSE_MODE_WRENCH): one axis pair of the sensed wrench of one slot's task,
//                         goal rows 30..35 in place, behind the simulated-sensor launch that has just written them.
//   saip_sense_randomize  fills the per-instance joint and wrench tables with uniform draws between two batch-uniform tables
// saip_sense_apply never writes the true state, and columns B..ld-1 of no array are written.  Every array is [rows][ld] and a wavefront
// is 64 consecutive instances of one row, so each of its loads and stores is one contiguous run.
#include <hip/hip_runtime.h>

#include "saip_sense.h"

namespace saip {

__global__ void __launch_bounds__(64) saip_sense_apply(const SenseParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const int row = blockIdx.y + ((P.mode & SENSE_MODE_JOINTS) ? 0 : P.n);
	const size_t ld = P.ld;
	if (row < P.n) {
		const long long js = P.per_instance_joints ? (long long)ld : 1, jc = P.per_instance_joints ? (long long)b : 0;
		const size_t k = (size_t)row * ld + b;
		double qm, dqm;
		se_joint(P.joints + (long long)row * SENSE_JOINT_WORDS * js + jc, js, P.seed_lo, P.seed_hi, P.period, b, row, P.q[k], P.dq[k], &qm, &dqm);
		P.q_meas[k] = qm;
		P.dq_meas[k] = dqm;
		return;
	}
	se_wrench_rows(P, row, b);
}

// One lane per instance, looping over the words: every store of a wavefront is one contiguous run of a row.
__global__ void __launch_bounds__(64) saip_sense_randomize(const SenseRandomParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const size_t ld = P.ld;
	if (P.joints)
		for (int w = 0; w < P.n * SENSE_JOINT_WORDS; w++)
			P.joints[(size_t)w * ld + b] = se_draw(P.seed_lo, P.seed_hi, P.round, SENSE_TABLE_JOINTS, b, w, P.joint_lo[w], P.joint_hi[w]);
	if (P.wrenches)
		for (int w = 0; w < P.n_slots * SENSE_WRENCH_WORDS; w++)
			P.wrenches[(size_t)w * ld + b] = se_draw(P.seed_lo, P.seed_hi, P.round, SENSE_TABLE_WRENCHES, b, w, P.wrench_lo[w], P.wrench_hi[w]);
}

hipError_t launch_sense_apply(const SenseParams& P, hipStream_t stream) {
	const int rows = ((P.mode & SENSE_MODE_JOINTS) ? P.n : 0) + ((P.mode & SENSE_MODE_WRENCH) ? 3 * P.n_slots : 0);
	if (rows == 0) return hipSuccess;
	hipLaunchKernelGGL(saip_sense_apply, dim3((P.B + 63) / 64, rows), dim3(64), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_sense_randomize(const SenseRandomParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_sense_randomize, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
