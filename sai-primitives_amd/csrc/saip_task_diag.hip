// Task-space diagnostics of one motion-force task (one lane per instance), for the state last pushed:
//   MotionForceTask::getPositionError / getOrientationError          src/tasks/MotionForceTask.cpp:540-546, 291
//   getCurrentLinearVelocity / getCurrentAngularVelocity              :293-298 (_jacobian = P Jw: the partial-task projection included)
//   getSensedForceControlWorldFrame / getSensedMomentControlWorldFrame :805-828
//   getUnitMassForce                                                   MotionForceTask.h:266, MotionForceTask.cpp:478
// A readback path, off the control cycle: it reads the task's goal, desired state, integrators and constants and writes `out` only.
#include "saip_law.h"
#include "saip_fk.h"

namespace saip {

// out = [24][ld]: 0..2 position error, 3..5 orientation error, 6..8 / 9..11 current linear / angular velocity, 12..14 / 15..17 sensed force /
// moment at the control point in the world frame, 18..23 unit-mass force.  goal: the user goal block ([gcomps][ld]); desired: what the law
// tracks (the OTG output of the last cycle, or the goal when the OTG is off).  TREE: kinematic trees -- the walk over the ancestors of the
// task's body only.
template <bool TREE>
__global__ void __launch_bounds__(64) saip_task_diag_kernel(const CycleParams P, const int task, const double* __restrict__ goal,
															 const double* __restrict__ desired, const int gcomps, double* __restrict__ out) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const ModelDev& md = *P.model;
	const TaskDev& task_ref = P.tasks[task];
	const double* q = P.q;
	const double* dq = P.dq;
	const int ld = P.ld;
	// pose (the arithmetic of fk_control_frame, hence bit-identical to the pose readback) and the unprojected world twist vw = Jw dq,
	// accumulated in the same walk (SAIP_FK_TWIST_STEP); at the end v += w x p - c, since sum_j dq_j a_j x (p - o_j) = w x p - c
	double pos[3], Rc[9], tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
	{
		const TaskDev& tk = task_ref;  // (the walk names the task `tk`, by reference)
		SAIP_FK_WALK(TREE, { SAIP_FK_TWIST_STEP(dq) })
	}
	const TaskDev* const tk = &task_ref;  // (the law and its macros take the task by pointer)
	double vw[6];
	vw[0] = tv[0] + (tw[1] * pos[2] - tw[2] * pos[1]) - tc[0];
	vw[1] = tv[1] + (tw[2] * pos[0] - tw[0] * pos[2]) - tc[1];
	vw[2] = tv[2] + (tw[0] * pos[1] - tw[1] * pos[0]) - tc[2];
	for (int e = 0; e < 3; e++) vw[3 + e] = tw[e];

	// selection projectors, as the control law builds them
	const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	const double* rot = tk->param_in_compliant_frame ? Rc : I3;
	double sig_f[9], sig_m[9], sig_p[9], sig_o[9], T[9], ImS[9];
	LAW_MOTION_SIGMAS
	double r[24];
	// position error sigma_pos (x_goal - x), orientation error sigma_ori orientationError(R_goal, Rc) = -1/2 sum_c Rc[:,c] x Rg[:,c]
	double e3[3], oe[3] = {0, 0, 0};
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
	// current twist J dq with J = P Jw; P is block-diagonal (MotionForceTask.cpp:143-168 only ever fills its two 3x3 diagonal blocks)
	law_mat3_vec(tk->Ppos, vw, r + 6);
	law_mat3_vec(tk->Pori, vw + 3, r + 9);
	// sensed force / moment: goal entries 30..35 (sensor frame) exist when closed-loop force or moment control is on, else they are zero
	if (gcomps >= 36) {
		double fms[6], fc[3], mc[3], fsw[3], msw[3], Rl[9];
		for (int e = 0; e < 6; e++) fms[e] = goal[(size_t)(30 + e) * ld + b];
		for (int i = 0; i < 9; i++) Rl[i] = tk->Rcs[i];
		LAW_SENSED_WRENCH(fms, fms + 3)
		for (int e = 0; e < 3; e++) {
			r[12 + e] = fsw[e];
			r[15 + e] = msw[e];
		}
	} else {
		for (int e = 12; e < 18; e++) r[e] = 0.0;
	}
	// unit-mass force: the control law on copies of the state -- integrators read, never written back; the passivity controller is left
	// out (it scales the force feedback F_f only, not F_um), so its state is not touched either
	double G[36], ip[3], io[3], ifm[6], Ff[6];
	for (int e = 0; e < 36; e++) G[e] = e < gcomps ? desired[(size_t)e * ld + b] : 0.0;
	for (int e = 0; e < 3; e++) {
		ip[e] = tk->integ[(size_t)e * ld + b];
		io[e] = tk->integ[(size_t)(3 + e) * ld + b];
	}
	for (int e = 0; e < 6; e++) ifm[e] = tk->integ[(size_t)(6 + e) * ld + b];
	law_motion_force_general<true>(tk, vw, pos, Rc, G, ip, io, ifm, r + 18, Ff);
	for (int e = 0; e < 24; e++) out[(size_t)e * ld + b] = r[e];
}

hipError_t launch_task_diag(const CycleParams& P, int task, const double* goal, const double* desired, int gcomps, double* out, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL(saip_task_diag_kernel<true>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P, task, goal, desired, gcomps, out);
	else hipLaunchKernelGGL(saip_task_diag_kernel<false>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P, task, goal, desired, gcomps, out);
	return hipGetLastError();
}

}  // namespace saip
