// Goal schedules: the user goals of ONE closed-loop period of saip_batch_rollout_async, written in front of the period's OTG step and
// control cycle from keyframes that stay resident on the device (one lane per instance).  One launch serves every scheduled task.  The
// keyframe index i and the fraction s of the period are computed on the host at enqueue time and arrive as launch arguments: no device-side
// counter, no atomic.  It writes rows [first, first + count) of the scheduled tasks' goal blocks in columns 0..B-1 and nothing else.
#include <hip/hip_runtime.h>

#include "saip_device.h"

namespace saip {

// a + s (b - a), the difference, the product and the sum each rounded on its own (no contraction into an FMA): a host restatement in
// double precision reproduces the goal rows bit for bit
__device__ __forceinline__ double sched_lerp(double a, double b, double s) {
#pragma clang fp contract(off)
	return a + s * (b - a);
}

// R(s) = R0 Exp(s Log(R0^T R1)), row-major 3 x 3.  Log through the antisymmetric part and atan2 (well conditioned up to the angle the host
// accepts, pi - 1e-3), Exp through Rodrigues' formula as cos I + sin [k]x + (1 - cos) k k^T.  Sums of three terms run left to right and
// nothing is contracted, so a host restatement differs only by what its atan2 / sin / cos / sqrt differ.
__device__ __forceinline__ void sched_slerp(const double* R0, const double* R1, double s, double* out) {
#pragma clang fp contract(off)
	double M[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) M[3 * i + j] = (R0[i] * R1[j] + R0[3 + i] * R1[3 + j]) + R0[6 + i] * R1[6 + j];
	const double w0 = 0.5 * (M[7] - M[5]), w1 = 0.5 * (M[2] - M[6]), w2 = 0.5 * (M[3] - M[1]);
	const double sn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
	const double cs = 0.5 * (((M[0] + M[4]) + M[8]) - 1.0);
	if (sn == 0.0) {  // the same orientation twice (angle pi is refused at attach)
		for (int e = 0; e < 9; e++) out[e] = R0[e];
		return;
	}
	const double ang = s * atan2(sn, cs);
	const double k[3] = {w0 / sn, w1 / sn, w2 / sn};
	const double sa = sin(ang), ca = cos(ang), v = 1.0 - ca;
	double E[9];
	E[0] = (v * k[0]) * k[0] + ca;
	E[1] = (v * k[0]) * k[1] - sa * k[2];
	E[2] = (v * k[0]) * k[2] + sa * k[1];
	E[3] = (v * k[1]) * k[0] + sa * k[2];
	E[4] = (v * k[1]) * k[1] + ca;
	E[5] = (v * k[1]) * k[2] - sa * k[0];
	E[6] = (v * k[2]) * k[0] - sa * k[1];
	E[7] = (v * k[2]) * k[1] + sa * k[0];
	E[8] = (v * k[2]) * k[2] + ca;
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) out[3 * i + j] = (R0[3 * i] * E[j] + R0[3 * i + 1] * E[3 + j]) + R0[3 * i + 2] * E[6 + j];
}

// Row r of keyframe i: a [ld] array per row for per-instance keyframes (a wavefront's loads are contiguous), one batch-uniform value
// otherwise (index and pointer are wave-uniform: a uniform load).
__device__ __forceinline__ double sched_key(const ScheduleEntry& E, int i, int r, int ld, int b) {
	const size_t row = (size_t)i * E.count + r;
	return E.per_instance ? E.key[row * ld + b] : E.key[row];
}

__global__ void __launch_bounds__(64) saip_goal_schedule_apply(const ScheduleParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const int ld = P.ld;
	for (int t = 0; t < P.n; t++) {
		const ScheduleEntry& E = P.e[t];
		double* goal = E.goal + (size_t)E.first * ld + b;
		if (E.mode == SCHED_HOLD || E.s == 0.0) {  // on a keyframe (and past the last one): the keyframe's rows exactly
			for (int r = 0; r < E.count; r++) goal[(size_t)r * ld] = sched_key(E, E.i, r, ld, b);
			continue;
		}
		const int r_rot = E.rot ? 3 - E.first : E.count;  // first of the nine rotation rows inside the range
		for (int r = 0; r < E.count; r++) {
			if (r >= r_rot && r < r_rot + 9) continue;
			goal[(size_t)r * ld] = sched_lerp(sched_key(E, E.i, r, ld, b), sched_key(E, E.i + 1, r, ld, b), E.s);
		}
		if (E.rot) {
			double R0[9], R1[9], R[9];
			for (int e = 0; e < 9; e++) {
				R0[e] = sched_key(E, E.i, r_rot + e, ld, b);
				R1[e] = sched_key(E, E.i + 1, r_rot + e, ld, b);
			}
			sched_slerp(R0, R1, E.s, R);
			for (int e = 0; e < 9; e++) goal[(size_t)(r_rot + e) * ld] = R[e];
		}
	}
}

hipError_t launch_goal_schedule(const ScheduleParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_goal_schedule_apply, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
