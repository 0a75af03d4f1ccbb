// Environment schedules: the obstacle and plane tables of ONE closed-loop period of saip_batch_rollout_async, written at the head of the
// period from keyframes that stay resident on the device (arithmetic: saip_env_schedule.h).  One launch serves every schedule of the batch.
// The keyframe index, the fraction of the period and the length of a keyframe interval are computed on the host at enqueue time and arrive
// as launch arguments: no device-side counter, no atomic.  The launch reads no state.
//
// A per-instance table gets one lane per instance: every load and store is a contiguous [ld] run, columns B..ld-1 are never touched.  A
// batch-uniform table is written by the first lanes of the grid, one item per lane.  Items outside [first, first + n_items) are never written.
#include <hip/hip_runtime.h>

#include "saip_env_schedule.h"

namespace saip {

__global__ void __launch_bounds__(64) saip_env_schedule_apply(const EnvScheduleParams P) {
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	for (int t = 0; t < P.n; t++) {
		const EnvEntry& E = P.e[t];
		if (E.per_instance) {
			if (g >= P.B) continue;
			for (int item = 0; item < E.n_items; item++) env_entry_item(E, item, P.ld, g);
		} else if (g < E.n_items) {
			env_entry_item(E, g, 1, 0);
		}
	}
}

hipError_t launch_env_schedule(const EnvScheduleParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_env_schedule_apply, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
