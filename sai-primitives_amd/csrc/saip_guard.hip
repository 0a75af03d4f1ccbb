// Resident guards (arithmetic: saip_guard.h): one evaluation of every instance's guards, in a rollout period behind the goal schedules,
// the simulated-sensor launches and the sensing launch and in front of the period's OTG step and cycle.
//   saip_guard_apply<TREE>  one lane per instance.  It gathers the inputs of the signals the tables need (the sensed wrench rows of the
//                           goal block, max |dq|, and -- only when a guard or a phase needs it -- the pose of the task's control frame by
//                           SAIP_FK_WALK and the selection-projected errors in the recorder's arithmetic), writes them to the readout,
//                           then runs gd_step: the transition on the instance's column of the state arrays, and goal rows 0..23 of a
//                           HOLD or OFFSET phase.
//   saip_guard_reset        the state of _attach and _reset: everything 0 but entry[p > 0] = -1
//   saip_guard_add_cost     gd_cost on the sampler's per-instance cost
// It reads what the controller reads (q, dq: the measured copy while a sensing model is attached) and writes the guard state, the readout
// and goal rows 0..23 of one task; columns B..ld-1 of no array are written.  Every array is [rows][ld], so each load and store of a
// wavefront is one contiguous run.  run[] and fires[] are addressed in their rows by unrolled constants: no scratch.
#include "saip_law.h"
#include "saip_fk.h"
#include "saip_guard.h"

namespace saip {

template <bool TREE>
__global__ void __launch_bounds__(64) saip_guard_apply(const GuardParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const int ld = P.ld;
	const double nan = __builtin_nan("");
	GuardSignals S;
	for (int e = 0; e < 3; e++) S.f[e] = S.m[e] = S.pos[e] = nan;
	S.ep = S.eo = S.speed = nan;
	double rd[GUARD_READOUT_ROWS];
	for (int e = 0; e < GUARD_READOUT_ROWS; e++) rd[e] = nan;
	const double* goal = P.goal;
	if (P.need & GUARD_NEED_FORCE) {
		for (int e = 0; e < 3; e++) S.f[e] = goal[(size_t)(30 + e) * ld + b];
		rd[GUARD_READ_FORCE] = gd_norm3(S.f);
	}
	if (P.need & GUARD_NEED_MOMENT) {
		for (int e = 0; e < 3; e++) S.m[e] = goal[(size_t)(33 + e) * ld + b];
		rd[GUARD_READ_MOMENT] = gd_norm3(S.m);
	}
	if (P.need & GUARD_NEED_SPEED) {
		double vmax = 0.0;
		for (int j = 0; j < P.n; j++) vmax = fmax(vmax, fabs(P.dq[(size_t)j * ld + b]));
		S.speed = rd[GUARD_READ_JOINT_SPEED] = vmax;
	}
	double pose[GUARD_LATCH_ROWS];
	for (int e = 0; e < GUARD_LATCH_ROWS; e++) pose[e] = nan;
	const bool fk = (P.need & GUARD_NEED_FK) != 0;
	if (fk) {
		const ModelDev& md = *P.model;
		const TaskDev& task_ref = P.tasks[P.task];
		const double* q = P.q;
		double pos[3], Rc[9];
		{
			const TaskDev& tk = task_ref;  // (the walk names the task `tk`, by reference)
			SAIP_FK_WALK(TREE)
		}
		for (int e = 0; e < 3; e++) pose[e] = S.pos[e] = rd[GUARD_READ_POSITION + e] = pos[e];
		for (int e = 0; e < 9; e++) pose[3 + e] = Rc[e];
		if (P.need & GUARD_NEED_ERROR) {
			// sigma_pos (x_goal - x) and sigma_ori orientationError(R_goal, Rc), as the recorder and the task diagnostics form them, against the
			// goal rows as they stand now
			const TaskDev* const tk = &task_ref;  // (the law's macros take the task by pointer)
			const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
			const double* rot = tk->param_in_compliant_frame ? Rc : I3;
			double sig_f[9], sig_m[9], sig_p[9], sig_o[9], T[9], ImS[9];
			LAW_MOTION_SIGMAS
			double r[6], e3[3], oe[3] = {0, 0, 0};
			for (int i = 0; i < 3; i++) e3[i] = goal[(size_t)i * ld + b] - pos[i];
			law_mat3_vec(sig_p, e3, r);
			for (int c = 0; c < 3; c++) {
				const double a0 = Rc[c], a1 = Rc[3 + c], a2 = Rc[6 + c];
				const double b0 = goal[(size_t)(3 + c) * ld + b], b1 = goal[(size_t)(6 + c) * ld + b], b2 = goal[(size_t)(9 + c) * ld + b];
				oe[0] -= 0.5 * (a1 * b2 - a2 * b1);
				oe[1] -= 0.5 * (a2 * b0 - a0 * b2);
				oe[2] -= 0.5 * (a0 * b1 - a1 * b0);
			}
			law_mat3_vec(sig_o, oe, r + 3);
			S.ep = rd[GUARD_READ_POS_ERROR] = gd_norm3(r);
			S.eo = rd[GUARD_READ_ORI_ERROR] = gd_norm3(r + 3);
		}
	}
	for (int e = 0; e < GUARD_READOUT_ROWS; e++) P.readout[(size_t)e * ld + b] = rd[e];
	const long long gstride = P.per_instance ? (long long)ld : 1;
	gd_step(P.guards + (P.per_instance ? b : 0), gstride, P.G, P.phases, P.P, S, pose, fk, P.phase + b, P.since + b, P.clock + b, P.run + b, P.entry + b,
			P.fires + b, P.latch + b, (long long)ld, P.goal + b, (long long)ld);
}

__global__ void __launch_bounds__(64) saip_guard_reset(const GuardParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const size_t ld = P.ld;
	P.phase[b] = P.since[b] = P.clock[b] = 0;
	for (int g = 0; g < P.G; g++) P.run[g * ld + b] = P.fires[g * ld + b] = 0;
	for (int p = 0; p < P.P; p++) P.entry[p * ld + b] = p ? -1 : 0;
	for (int e = 0; e < GUARD_LATCH_ROWS; e++) P.latch[e * ld + b] = 0.0;
}

__global__ void __launch_bounds__(64) saip_guard_add_cost(const int B, const int* __restrict__ entry, double* __restrict__ cost, const double w_time, const double w_miss) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= B) return;
	cost[b] = gd_cost(cost[b], entry[b], w_time, w_miss);
}

hipError_t launch_guard_apply(const GuardParams& P, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL(saip_guard_apply<true>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_guard_apply<false>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_guard_reset(const GuardParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_guard_reset, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_guard_add_cost(int B, const int* entry_row, double* cost, double w_time, double w_miss, hipStream_t stream) {
	hipLaunchKernelGGL(saip_guard_add_cost, dim3((B + 63) / 64), dim3(64), 0, stream, B, entry_row, cost, w_time, w_miss);
	return hipGetLastError();
}

}  // namespace saip
