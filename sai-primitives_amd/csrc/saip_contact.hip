// Contact planes and the simulated force sensor of the resident simulator (one lane per instance): the force of up to four world-fixed
// half-spaces on one contact point carried by the body of a motion-force task, at the resident state q, dq (arithmetic: saip_contact.h).
//   SENSE  writes the wrench a force sensor would report into rows 30..35 of the task's goal block (the inverse of LAW_SENSED_WRENCH)
//   APPLY  writes tau_sim = tau_cmd (NaN -> 0) + J_v^T f for the integrator, and advances the running summaries
// Both write the readout.  Nothing else is touched: no state, torque, status, integrator or OTG array; columns B..ld-1 are never written.
// J_v^T f needs f, which needs the finished walk (pose and twist of the point), so APPLY walks the chain twice: the second walk has the
// joint's world axis and origin at hand again and nothing per joint is kept in between (no per-lane arrays, no scratch).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "saip_contact.h"
#include "saip_fk.h"

namespace saip {

// Every array is [rows][ld], so a wavefront's loads and stores are contiguous.  TREE: kinematic trees -- the walk over the ancestors of the
// task's body only; the other joints get no contact torque.  MOVING: the planes have an environment schedule -- the force is taken against
// the surface velocities it writes (ct_plane_forces_moving); everything else is the same text.
template <bool TREE, bool MOVING = false>
__global__ void __launch_bounds__(64) saip_contact_apply(const std::conditional_t<MOVING, ContactMovingParams, ContactParams> P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const ModelDev& md = *P.model;
	const TaskDev& tk = P.tasks[P.task];
	const double* q = P.q;
	const int ld = P.ld;
	// pose of the control frame (the arithmetic of fk_control_frame) and the twist accumulators, in one walk
	double pos[3], Rc[9], tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
	{
		SAIP_FK_WALK(TREE, { SAIP_FK_TWIST_STEP(P.dq) })
	}
	double pc[3], vc[3];
	ct_point(pos, Rc, P.rc, pc);
	ct_velocity(tv, tw, tc, pc, vc);
	ContactForce c;
	if constexpr (MOVING) ct_plane_forces_moving(P.planes, P.vel, P.n_planes, P.per_instance ? (long long)ld : 1, P.per_instance ? (long long)b : 0, pc, vc, &c);
	else ct_plane_forces(P.planes, P.n_planes, P.per_instance ? (long long)ld : 1, P.per_instance ? (long long)b : 0, pc, vc, &c);
	double* ro = P.readout + b;
	for (int e = 0; e < 3; e++) {
		ro[(size_t)e * ld] = c.f[e];
		ro[(size_t)(3 + e) * ld] = pc[e];
	}
	ro[(size_t)6 * ld] = c.dmin;
	ro[(size_t)7 * ld] = (double)c.active;
	if (P.mode == CONTACT_SENSE) {
		double FS[3], MS[3];
		ct_sensor(c.f, pc, pos, Rc, tk.Rcs, tk.tcs, FS, MS);
		for (int e = 0; e < 3; e++) {
			P.goal[(size_t)(30 + e) * ld + b] = FS[e];
			P.goal[(size_t)(33 + e) * ld + b] = MS[e];
		}
		return;
	}
	// APPLY.  A NaN torque is no torque (the integrator coasts): a flagged instance still gets pushed by the wall.  Joints the walk below
	// does not visit (behind the body; off its branch in a tree) carry the commanded torque alone.
	const uint32_t anc = TREE && tk.body >= 0 ? md.anc[tk.body] : 0u;
	for (int j = 0; j < P.n; j++) {
		if (j <= tk.body && (!TREE || ((anc >> j) & 1u))) continue;
		const double t = P.tau_cmd[(size_t)j * ld + b];
		P.tau_sim[(size_t)j * ld + b] = t == t ? t : 0.0;
	}
	if (c.active) {
		SAIP_FK_WALK(TREE, {
			const double aj[3] = {ax, ay, az};
			double aw[3];
			fk_mat3_vec(Rt, aj, aw);
			const double t = P.tau_cmd[(size_t)j * ld + b];
			P.tau_sim[(size_t)j * ld + b] = (t == t ? t : 0.0) + ct_joint_torque(md.jtype[j] == 1, aw, o, pc, c.f);
		})
	} else {
		// no plane acts: f = 0 exactly, and the torques pass through
		for (int j = 0; j <= tk.body; j++) {
			if (TREE && !((anc >> j) & 1u)) continue;
			const double t = P.tau_cmd[(size_t)j * ld + b];
			P.tau_sim[(size_t)j * ld + b] = t == t ? t : 0.0;
		}
	}
	if (P.summary) ct_summary_advance(P.summary + b, ld, P.dt, c);
}

hipError_t launch_contact_apply(const ContactParams& P, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL(saip_contact_apply<true>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_contact_apply<false>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_contact_apply_moving(const ContactMovingParams& P, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL((saip_contact_apply<true, true>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL((saip_contact_apply<false, true>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
