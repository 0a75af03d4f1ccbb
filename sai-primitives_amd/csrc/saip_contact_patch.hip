// Contact patches of the resident simulator: up to eight contact points on the body of a motion-force task against the patch's own planes,
// the net force and net moment fed to the integrator and to the simulated sensor; up to two patches per launch (arithmetic:
// saip_contact_patch.h).  The modes of saip_contact.hip:
//   SENSE  writes the wrench a force sensor would report into rows 30..35 of the task's goal block, for the patches that have the sensor
//   APPLY  writes tau_sim = ((tau_cmd, NaN -> 0) + patch 0) + patch 1 for the integrator, and advances the running summaries
// Both write the readout of the patches they evaluate.  Nothing else is touched; columns B..ld-1 are never written.
//
// Eight instances x eight lanes per 64-thread block: lane l of a group is point slot l.  Every lane of a group walks the chain (or the
// ancestors of the body) with the same arguments -- redundant, but the walk is serial -- and then evaluates its own point.  The sums over
// the slots are width-8 cross-lane folds (off = 4, 2, 1; no LDS, no atomics).  APPLY walks a second time, every lane forming its own point's
// torque on the joint at hand, and only for the groups in which a point touches.  Nothing per joint or per point is kept in an array.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "saip_contact_patch.h"
#include "saip_fk.h"

namespace saip {

// lane 0 of every aligned group of eight ends with v[0] + ... + v[7] in the order of cp_fold_sum
__device__ __forceinline__ double cp_lane_sum(double v) {
	v = v + __shfl_down(v, 4, 8);
	v = v + __shfl_down(v, 2, 8);
	v = v + __shfl_down(v, 1, 8);
	return v;
}
__device__ __forceinline__ int cp_lane_sum(int v) {
	v += __shfl_down(v, 4, 8);
	v += __shfl_down(v, 2, 8);
	v += __shfl_down(v, 1, 8);
	return v;
}

// MOVING: the planes of a patch may have an environment schedule -- such a patch is evaluated against the surface velocities it writes
// (cp_slot_eval_moving); everything else is the same text.
template <bool TREE, bool MOVING = false>
__global__ void __launch_bounds__(64) saip_contact_patch_apply(const std::conditional_t<MOVING, ContactPatchMovingParams, ContactPatchParams> P) {
	const int lane = threadIdx.x & 7;
	const int inst = blockIdx.x * 8 + (threadIdx.x >> 3);
	// a group beyond B evaluates instance B - 1 again and stores nothing: every lane of the wavefront takes every shuffle
	const bool live = inst < P.B;
	const int b = live ? inst : P.B - 1;
	const bool writer = live && lane == 0;
	const ModelDev& md = *P.model;
	const double* q = P.q;
	const int ld = P.ld;
	for (int ip = 0; ip < P.n_patches; ip++) {
		const PatchDev& pd = P.patch[ip];
		if (P.mode == CONTACT_SENSE && !pd.sensor) continue;
		const TaskDev& tk = P.tasks[pd.task];
		double pos[3], Rc[9], tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
		{
			SAIP_FK_WALK(TREE, { SAIP_FK_TWIST_STEP(P.dq) })
		}
		PatchSlot s;
		if (lane < pd.n_points) {
			const double rl[3] = {pd.r[lane][0], pd.r[lane][1], pd.r[lane][2]};
			bool moved = false;
			if constexpr (MOVING) {
				if (P.vel[ip]) {
					cp_slot_eval_moving(pd.planes, P.vel[ip], pd.n_planes, pd.per_instance ? (long long)ld : 1, pd.per_instance ? (long long)b : 0, pos, Rc, rl, tv, tw, tc, &s);
					moved = true;
				}
			}
			if (!moved) cp_slot_eval(pd.planes, pd.n_planes, pd.per_instance ? (long long)ld : 1, pd.per_instance ? (long long)b : 0, pos, Rc, rl, tv, tw, tc, &s);
		} else {
			cp_slot_unused(&s);
		}
		double F[3], M[3];
		for (int e = 0; e < 3; e++) {
			F[e] = cp_lane_sum(s.c.f[e]);
			M[e] = cp_lane_sum(s.m[e]);
		}
		const double fn_total = cp_lane_sum(s.c.fn_sum);
		const int n_touch = __shfl(cp_lane_sum(s.c.active > 0 ? 1 : 0), 0, 8);  // the whole group needs it
		double dmin = s.dcand;
		int i_deep = lane;
		for (int off = 4; off > 0; off >>= 1) {
			const double db = __shfl_down(dmin, off, 8);
			const int ib = __shfl_down(i_deep, off, 8);
			if (cp_deeper(db, ib, dmin, i_deep)) {
				dmin = db;
				i_deep = ib;
			}
		}
		if (live) pd.readout[(size_t)(12 + lane) * ld + b] = s.c.fn_sum;  // every lane its own slot's row; rows 0..11 by lane 0
		if (writer) {
			double* ro = pd.readout + b;
			for (int e = 0; e < 3; e++) {
				ro[(size_t)e * ld] = F[e];
				ro[(size_t)(3 + e) * ld] = M[e];
				ro[(size_t)(9 + e) * ld] = pos[e];
			}
			ro[(size_t)6 * ld] = dmin;
			ro[(size_t)7 * ld] = (double)n_touch;
			ro[(size_t)8 * ld] = (double)i_deep;
		}
		if (P.mode == CONTACT_SENSE) {
			if (writer) {
				double FS[3], MS[3];
				cp_sensor(F, M, Rc, tk.Rcs, tk.tcs, FS, MS);
				for (int e = 0; e < 3; e++) {
					pd.goal[(size_t)(30 + e) * ld + b] = FS[e];
					pd.goal[(size_t)(33 + e) * ld + b] = MS[e];
				}
			}
			continue;
		}
		// APPLY.  A NaN torque is no torque (the integrator coasts).  The first patch seeds every joint its second walk does not reach with
		// the commanded torque; a later patch adds to what stands there and skips (does not add zero to) every other joint.
		const bool touch = n_touch > 0;
		if (ip == 0 && writer) {
			const uint32_t anc = TREE && tk.body >= 0 ? md.anc[tk.body] : 0u;
			for (int j = 0; j < P.n; j++) {
				if (touch && j <= tk.body && (!TREE || ((anc >> j) & 1u))) continue;
				const double t = P.tau_cmd[(size_t)j * ld + b];
				P.tau_sim[(size_t)j * ld + b] = t == t ? t : 0.0;
			}
		}
		if (touch) {
			SAIP_FK_WALK(TREE, {
				const double aj[3] = {ax, ay, az};
				double aw[3];
				fk_mat3_vec(Rt, aj, aw);
				const double ext = cp_lane_sum(s.c.active ? ct_joint_torque(md.jtype[j] == 1, aw, o, s.p, s.c.f) : 0.0);
				if (writer) {
					double base;
					if (ip == 0) {
						const double t = P.tau_cmd[(size_t)j * ld + b];
						base = t == t ? t : 0.0;
					} else {
						base = P.tau_sim[(size_t)j * ld + b];
					}
					P.tau_sim[(size_t)j * ld + b] = base + ext;
				}
			})
		}
		if (writer) cp_summary_advance(pd.summary + b, ld, P.dt, F, M, fn_total, dmin, n_touch, pd.n_points);
	}
}

hipError_t launch_contact_patch_apply(const ContactPatchParams& P, bool tree, hipStream_t stream) {
	const unsigned blocks = (unsigned)(((long long)P.B + 7) / 8);
	if (tree) hipLaunchKernelGGL(saip_contact_patch_apply<true>, dim3(blocks), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_contact_patch_apply<false>, dim3(blocks), dim3(64), 0, stream, P);
	return hipGetLastError();
}
hipError_t launch_contact_patch_apply_moving(const ContactPatchMovingParams& P, bool tree, hipStream_t stream) {
	const unsigned blocks = (unsigned)(((long long)P.B + 7) / 8);
	if (tree) hipLaunchKernelGGL((saip_contact_patch_apply<true, true>), dim3(blocks), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL((saip_contact_patch_apply<false, true>), dim3(blocks), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
