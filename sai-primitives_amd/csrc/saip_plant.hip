// The plant model of the resident simulator (one lane per instance; arithmetic: saip_plant.h).
//   saip_plant_apply      tau_act = actuator(tau_cmd) - friction + joint stops + J^T of the acting external wrenches, at the resident state
//                         q, dq, in front of an integration substep; advances the running summaries
//   saip_plant_randomize  fills the per-instance joint and wrench tables with uniform draws between two batch-uniform tables
//   saip_plant_chain_randomize  the same for the actuation chain's table (saip_plant_chain.h)
// saip_plant_apply<*, true> runs the actuation chain in front of the joint rows and writes the chain's state arrays besides.
// saip_plant_apply reads q, dq and tau_cmd and writes tau_act and the summaries: no state, torque, status, integrator or OTG array is
// touched, and columns B..ld-1 are never written.  The joint part keeps nothing per joint: every joint's torque goes straight to tau_act.
// A wrench needs the finished walk to its link (the application point, the link's rotation) before any joint's share of it is known, so
// every acting wrench walks its chain twice, as saip_contact.hip does: the second walk has the joint's world axis and origin at hand again
// and adds the joint's share to tau_act in place (no per-lane arrays, no scratch).  Wrenches are handled in table order, so a joint
// receives its shares in table order.
#include <hip/hip_runtime.h>

#include "saip_fk.h"
#include "saip_plant.h"
#include "saip_plant_chain.h"

namespace saip {

// the launch of either instantiation and the plant's part of it
template <bool CHAIN>
struct PlantArgs {
	typedef PlantParams type;
};
template <>
struct PlantArgs<true> {
	typedef PlantChainParams type;
};
__device__ inline const PlantParams& pl_params(const PlantParams& A) { return A; }
__device__ inline const PlantParams& pl_params(const PlantChainParams& A) { return A.P; }
// the chain's arrays of joint j, instance b
__device__ inline double* pc_chain_taps(const PlantChainParams& A, int j, int b) { return A.depth > 0 ? A.taps + (size_t)j * A.depth * A.P.ld + b : nullptr; }
__device__ inline void pc_chain_load(const PlantChainParams& A, int j, int b, PlantChainLoaded* L) {
	const size_t ld = A.P.ld;
	const long long cs = A.per_instance ? (long long)ld : 1, cc = A.per_instance ? (long long)b : 0;
	pc_load(A.table + (long long)j * PLANT_CHAIN_WORDS * cs + cc, cs, A.depth, pc_chain_taps(A, j, b), A.filt + (size_t)j * PLANT_CHAIN_FILT_ROWS * ld + b, A.primed + (size_t)j * ld + b,
			(long long)ld, A.advance != 0, L);
}

// Every array is [rows][ld], so a wavefront's loads and stores are contiguous.  TREE: kinematic trees -- the walks cover the ancestors of
// the wrench's body only; the other joints get nothing from it.  CHAIN: the actuation chain (saip_plant_chain.h) stands between tau_cmd and
// pl_joint -- one pc_step per joint (as pc_load and pc_finish), on the chain's own state arrays; everything behind it is the same code.
template <bool TREE, bool CHAIN>
__global__ void __launch_bounds__(64) saip_plant_apply(const typename PlantArgs<CHAIN>::type A) {
	const PlantParams& P = pl_params(A);
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const ModelDev& md = *P.model;
	const double* q = P.q;
	const int ld = P.ld;
	const long long js = P.per_instance_joints ? (long long)ld : 1, jc = P.per_instance_joints ? (long long)b : 0;
	PlantFold f;
	pl_fold_init(&f);
	PlantChainLoaded nxt;
	if constexpr (CHAIN) pc_chain_load(A, 0, b, &nxt);
	for (int j = 0; j < P.n; j++) {
		const size_t k = (size_t)j * ld + b;
		const double dqj = P.dq[k];
		PlantJointOut o;
		double t = P.tau_cmd[k];
		if constexpr (CHAIN) {
			// the next joint's words and state are requested before this joint's stores: the compiler cannot tell the rows of one column
			// apart and would make every load wait for the stores before it, one memory round trip per joint
			const PlantChainLoaded cur = nxt;
			if (j + 1 < P.n) pc_chain_load(A, j + 1, b, &nxt);
			t = pc_finish(cur, A.depth, pc_chain_taps(A, j, b), A.filt + (size_t)j * PLANT_CHAIN_FILT_ROWS * ld + b, A.primed + k, ld, t, P.dt, A.advance != 0);
		}
		pl_joint(P.joints + (long long)j * PLANT_JOINT_WORDS * js + jc, js, t, q[k], dqj, &o);
		P.tau_act[k] = o.tau;
		pl_fold_joint(&f, o, dqj);
	}
	double work_ext = 0.0;
	const long long ws = P.per_instance_wrenches ? (long long)ld : 1, wc = P.per_instance_wrenches ? (long long)b : 0;
	for (int w = 0; w < P.n_wrenches; w++) {
		const double* ww = P.wrenches + (long long)w * PLANT_WRENCH_WORDS * ws + wc;
		const PlantSite& tk = P.site[w];
		if (tk.body < 0 || !pl_wrench_acts(ww, ws, P.period)) continue;
		// the application point and the link's rotation in the world (the arithmetic of fk_control_frame)
		double pos[3], Rc[9];
		{
			SAIP_FK_WALK(TREE)
		}
		double F[3], M[3];
		pl_wrench_world(ww, ws, tk.frame, Rc, F, M);
		const double pw[3] = {pos[0], pos[1], pos[2]};
		{
			SAIP_FK_WALK(TREE, {
				const double aj[3] = {ax, ay, az};
				double aw[3];
				fk_mat3_vec(Rt, aj, aw);
				const double x = pl_wrench_torque(md.jtype[j] == 1, aw, o, pw, F, M);
				const size_t k = (size_t)j * ld + b;
				P.tau_act[k] = P.tau_act[k] + x;
				work_ext = pl_work_add(work_ext, x, P.dq[k]);
			})
		}
	}
	pl_summary_advance(P.summary + b, ld, P.dt, f, work_ext);
}

// One lane per instance, looping over the words: every store of a wavefront is one contiguous run of a row.
__global__ void __launch_bounds__(64) saip_plant_randomize(const PlantRandomParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const size_t ld = P.ld;
	if (P.joints)
		for (int w = 0; w < P.n * PLANT_JOINT_WORDS; w++)
			P.joints[(size_t)w * ld + b] = pl_draw(P.seed_lo, P.seed_hi, P.round, PLANT_TABLE_JOINTS, b, w, P.joint_lo[w], P.joint_hi[w], false);
	if (P.wrenches)
		for (int w = 0; w < P.n_wrenches * PLANT_WRENCH_WORDS; w++)
			P.wrenches[(size_t)w * ld + b] =
				pl_draw(P.seed_lo, P.seed_hi, P.round, PLANT_TABLE_WRENCHES, b, w, P.wrench_lo[w], P.wrench_hi[w], w % PLANT_WRENCH_WORDS >= 6);
}

// One lane per instance over the chain table's words, as saip_plant_randomize.
__global__ void __launch_bounds__(64) saip_plant_chain_randomize(const PlantChainRandomParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const size_t ld = P.ld;
	for (int w = 0; w < P.n * PLANT_CHAIN_WORDS; w++) P.table[(size_t)w * ld + b] = pc_draw(P.seed_lo, P.seed_hi, P.round, b, w, P.lo[w], P.hi[w], P.depth);
}

hipError_t launch_plant_apply(const PlantParams& P, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL((saip_plant_apply<true, false>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL((saip_plant_apply<false, false>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_plant_chain_apply(const PlantChainParams& C, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL((saip_plant_apply<true, true>), dim3((C.P.B + 63) / 64), dim3(64), 0, stream, C);
	else hipLaunchKernelGGL((saip_plant_apply<false, true>), dim3((C.P.B + 63) / 64), dim3(64), 0, stream, C);
	return hipGetLastError();
}

hipError_t launch_plant_chain_randomize(const PlantChainRandomParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_plant_chain_randomize, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_plant_randomize(const PlantRandomParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_plant_randomize, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
