// Batched forward dynamics + semi-implicit Euler step: the "step after the path" of SURVEY.md 8(f) f4, so that closed-loop
// rollouts (OTG -> control cycle -> dynamics) stay on the device.  It stands in for what the reference's examples do with the
// external physics engine: sim->setJointTorques(...); sim->integrate()   (/root/reference/examples/05-using_robot_controller/
// 05-using_robot_controller.cpp:225-231; sai-simulation is not part of the reference tree, so there is no reference arithmetic to
// match -- the oracle is the Lagrangian restatement in oracle/restatement.forward_dynamics, see tests/test_gpu_dynamics.py).
//
//   M(q) qdd + b(q, dq) + g(q) = tau        b: Coriolis / centrifugal, g: gravity
//   dq <- dq + dt qdd ;  q <- q + dt dq     (semi-implicit Euler, `substeps` times per call with the torque held)
//
// One lane per instance (7-dof chains run saip_dynamics_oct.hip instead: eight lanes per instance).  Bias forces by one recursive Newton-Euler pass in world coordinates, M(q) from composite rigid bodies
// (spatial inertias about the joint origins, suffix sums along the chain), Cholesky solve.  Per-body arrays are lane-private
// (scratch for NMAX = 32, mostly registers for NMAX = 8); the kernel is FP64-latency bound like the cycle kernels and is not on the
// benchmarked path.
#include <hip/hip_runtime.h>
#include <math.h>

#include "saip_device.h"
#include "saip_rbd.h"

namespace saip {

// TREE: kinematic trees (ModelDev::is_tree) -- the same step with the tree traversals of saip_rbd.h; every integrate path of the engine lands
// here for them, whatever the dof
// INERTIA: mass, centre of mass and inertia of every body from the lane's column of the resident table SimParams::inertia instead of the model
template <int NMAX, bool TREE, bool INERTIA>
__global__ void __launch_bounds__(64) saip_integrate_kernel(const SimParams S) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= S.B) return;
	const ModelDev& md = *S.model;
	using IN = typename InertialSource<INERTIA>::type;
	IN in;
	if constexpr (INERTIA) {
		in.w = S.inertia + (S.inertia_stride == 1 ? 0 : (long long)b);
		in.stride = S.inertia_stride;
	}
	const int n = S.n;
	double q[NMAX], dq[NMAX], tau[NMAX], h[NMAX], ddq[NMAX], e[NMAX];
	double M[NMAX][NMAX];
#pragma unroll
	for (int j = 0; j < n; j++) {
		q[j] = S.q[(size_t)j * S.ld + b];
		dq[j] = S.dq[(size_t)j * S.ld + b];
		tau[j] = S.tau[(size_t)j * S.ld + b];
		if (!(tau[j] == tau[j])) tau[j] = 0.0;  // flagged instances (NaN torques) coast
		e[j] = 0.0;
		ddq[j] = 0.0;
	}
	const V3 a0 = v3(-S.gravity[0], -S.gravity[1], -S.gravity[2]);
	Chain<NMAX> K;
	for (int step = 0; step < S.substeps; step++) {
		if constexpr (TREE) chain_fk_tree<NMAX>(md, n, q, K, in);
		else chain_fk<NMAX>(md, n, q, K, in);
		if constexpr (TREE) rnea_tree<NMAX>(md, n, K, dq, e, a0, true, h, in);  // b(q, dq) + g(q)
		else rnea<NMAX>(md, n, K, dq, e, a0, true, h, in);
		if constexpr (TREE) mass_matrix_crb_tree<NMAX>(md, n, K, M, in);
		else mass_matrix_crb<NMAX>(md, n, K, M, in);
		// Cholesky M = L L^T (lower, in place), then two triangular solves
#pragma unroll
		for (int k = 0; k < n; k++) {
			double d = M[k][k];
#pragma unroll
			for (int l = 0; l < n; l++)
				if (l < k) d -= M[k][l] * M[k][l];
			d = sqrt(d);
			M[k][k] = d;
			const double rd = 1.0 / d;
#pragma unroll
			for (int i = 0; i < n; i++) {
				if (i <= k) continue;
				double s = M[i][k];
#pragma unroll
				for (int l = 0; l < n; l++)
					if (l < k) s -= M[i][l] * M[k][l];
				M[i][k] = s * rd;
			}
		}
#pragma unroll
		for (int i = 0; i < n; i++) {
			double s = tau[i] - h[i] - S.damping * dq[i];
#pragma unroll
			for (int l = 0; l < n; l++)
				if (l < i) s -= M[i][l] * ddq[l];
			ddq[i] = s / M[i][i];
		}
#pragma unroll
		for (int ii = 0; ii < n; ii++) {
			const int i = n - 1 - ii;
			double s = ddq[i];
#pragma unroll
			for (int l = 0; l < n; l++)
				if (l > i) s -= M[l][i] * ddq[l];
			ddq[i] = s / M[i][i];
		}
#pragma unroll
		for (int j = 0; j < n; j++) {
			dq[j] += S.dt * ddq[j];
			q[j] += S.dt * dq[j];
		}
	}
#pragma unroll
	for (int j = 0; j < n; j++) {
		S.q[(size_t)j * S.ld + b] = q[j];
		S.dq[(size_t)j * S.ld + b] = dq[j];
		if (S.ddq) S.ddq[(size_t)j * S.ld + b] = ddq[j];
	}
}

hipError_t launch_integrate_oct(const SimParams& S, hipStream_t stream);  // saip_dynamics_oct.hip: eight lanes per instance, 7-dof chains

template <bool INERTIA>
static hipError_t launch_integrate_lanes(const SimParams& S, bool tree, hipStream_t stream) {
	const int grid = (S.B + 63) / 64;
	if (tree) {
		if (S.n <= 8) hipLaunchKernelGGL((saip_integrate_kernel<8, true, INERTIA>), dim3(grid), dim3(64), 0, stream, S);
		else hipLaunchKernelGGL((saip_integrate_kernel<32, true, INERTIA>), dim3(grid), dim3(64), 0, stream, S);
	} else {
		if (S.n <= 8) hipLaunchKernelGGL((saip_integrate_kernel<8, false, INERTIA>), dim3(grid), dim3(64), 0, stream, S);
		else hipLaunchKernelGGL((saip_integrate_kernel<32, false, INERTIA>), dim3(grid), dim3(64), 0, stream, S);
	}
	return hipGetLastError();
}

// S.inertia (the resident inertia table) selects the INERTIA instantiation of whichever kernel the model takes
hipError_t launch_integrate(const SimParams& S, bool tree, hipStream_t stream) {
	// 7-dof chains: the eight-lanes-per-instance kernel is faster at every batch size measured (8.7 vs 33.4 us at 4096, 46.8 vs 81.1 us at
	// 65 536, 166 vs 218 us at 262 144 per two substeps)
	if (!tree && S.n == 7) return launch_integrate_oct(S, stream);
	return S.inertia ? launch_integrate_lanes<true>(S, tree, stream) : launch_integrate_lanes<false>(S, tree, stream);
}

}  // namespace saip
