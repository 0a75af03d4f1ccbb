// Robot-model queries at the resident state, one lane per instance (the batched SaiModel accessors of include/saip.h):
//   saip_model_frames_kernel      position / rotation / linearVelocity / angularVelocity / J of up to SAIP_MAXQF frames in one walk
//   saip_model_dynamics_kernel    M, M^-1, jointGravityVector, coriolisForce
// Readback paths, off the control cycle: they read q, dq and the model constants and write their outputs only.
#include <hip/hip_runtime.h>
#include <math.h>

#include "saip_device.h"
#include "saip_fk.h"
#include "saip_rbd.h"

namespace saip {

namespace {

__device__ __forceinline__ void mq_cross(const double* a, const double* b, double* c) {
	c[0] = a[1] * b[2] - a[2] * b[1];
	c[1] = a[2] * b[0] - a[0] * b[2];
	c[2] = a[0] * b[1] - a[1] * b[0];
}

// rows of frame f once the walk has reached its body: R, o = rotation and origin of that body, tv / tw / tc = the twist accumulators of
// saip_task_diag_kernel (v = tv + tw x p - tc, w = tw).  The Jacobian columns of the joints up to the body already hold Jw = z_j and the
// partial Jv = o_j x z_j (revolute) or z_j (prismatic); here Jv gets its z_j x p, and the columns behind the body are zeroed.
// TREE: the columns of the joints that are not ancestors of the body are zeroed (on a chain those are the ones behind it)
template <bool TREE = false>
__device__ __forceinline__ void frame_emit(const FrameQuery& Q, const ModelDev& md, const int f, const int b, const double* R, const double* o,
										   const double* tv, const double* tw, const double* tc) {
	const size_t ld = Q.ld;
	const int n = Q.n;
	double* out = Q.out + (size_t)Q.slot[f] * Q.rows * ld + b;
	// the tail of SAIP_FK_WALK, with the frame in place of the task's control frame: the same arithmetic, hence the same bits
	double p[3], pos[3], Rc[9];
	fk_mat3_vec(R, Q.pos[f], p);
	for (int e = 0; e < 3; e++) pos[e] = o[e] + p[e];
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++) Rc[3 * r + c] = R[3 * r] * Q.rot[f][c] + R[3 * r + 1] * Q.rot[f][3 + c] + R[3 * r + 2] * Q.rot[f][6 + c];
	double v[3], w[3];
	v[0] = tv[0] + (tw[1] * pos[2] - tw[2] * pos[1]) - tc[0];
	v[1] = tv[1] + (tw[2] * pos[0] - tw[0] * pos[2]) - tc[1];
	v[2] = tv[2] + (tw[0] * pos[1] - tw[1] * pos[0]) - tc[2];
	for (int e = 0; e < 3; e++) w[e] = tw[e];
	double ps[3];  // the point rotated into the output frame (Jacobian columns)
	if (Q.world) {
		double t[3], Rw[9], vw[3], ww[3];
		fk_mat3_vec(Q.Rwb, pos, t);
		for (int e = 0; e < 3; e++) {
			ps[e] = t[e];
			pos[e] = t[e] + Q.pwb[e];
		}
		for (int r = 0; r < 3; r++)
			for (int c = 0; c < 3; c++) Rw[3 * r + c] = Q.Rwb[3 * r] * Rc[c] + Q.Rwb[3 * r + 1] * Rc[3 + c] + Q.Rwb[3 * r + 2] * Rc[6 + c];
		fk_mat3_vec(Q.Rwb, v, vw);
		fk_mat3_vec(Q.Rwb, w, ww);
		for (int e = 0; e < 9; e++) Rc[e] = Rw[e];
		for (int e = 0; e < 3; e++) {
			v[e] = vw[e];
			w[e] = ww[e];
		}
	} else {
		for (int e = 0; e < 3; e++) ps[e] = pos[e];
	}
	for (int e = 0; e < 3; e++) out[e * ld] = pos[e];
	for (int e = 0; e < 9; e++) out[(3 + e) * ld] = Rc[e];
	for (int e = 0; e < 3; e++) {
		out[(12 + e) * ld] = v[e];
		out[(15 + e) * ld] = w[e];
	}
	if (!Q.jac) return;
	const int body = Q.body[f];
	const size_t rs = (size_t)n * ld;  // one Jacobian row
	const uint32_t anc = TREE && body >= 0 ? md.anc[body] : 0u;
	for (int c = 0; c < n; c++) {
		double* J = out + (size_t)(18 + c) * ld;
		bool off_path;
		if constexpr (TREE) off_path = !((anc >> c) & 1u);
		else off_path = c > body;
		if (off_path) {
			for (int r = 0; r < 6; r++) J[r * rs] = 0.0;
		} else if (md.jtype[c] == 1) {
			const double z[3] = {J[3 * rs], J[4 * rs], J[5 * rs]};
			double zp[3];
			mq_cross(z, ps, zp);
			for (int r = 0; r < 3; r++) J[r * rs] += zp[r];
		}
	}
}

}  // namespace

// One joint j of a frames walk, expanded in place: SAIP_FK_JOINT_STEP with the twist accumulators and, with Q.jac, column j of the Jacobian
// -- Jw = z_j and the partial Jv of frame_emit -- stored to frame g, where FRAMES_ declares g: a loop header or one frame.
#define MQ_FRAME_JOINT_STEP(FRAMES_)                                                                                    \
	SAIP_FK_JOINT_STEP({                                                                                                \
		SAIP_FK_TWIST_STEP(Q.dq)                                                                                        \
		if (Q.jac) {                                                                                                    \
			double zs[3], os[3], jv[3], jw[3];                                                                          \
			if (Q.world) {                                                                                              \
				fk_mat3_vec(Q.Rwb, aw, zs);                                                                             \
				fk_mat3_vec(Q.Rwb, o, os);                                                                              \
			} else {                                                                                                    \
				for (int e = 0; e < 3; e++) {                                                                           \
					zs[e] = aw[e];                                                                                      \
					os[e] = o[e];                                                                                       \
				}                                                                                                       \
			}                                                                                                           \
			if (rev) {                                                                                                  \
				mq_cross(os, zs, jv);                                                                                   \
				for (int e = 0; e < 3; e++) jw[e] = zs[e];                                                              \
			} else {                                                                                                    \
				for (int e = 0; e < 3; e++) {                                                                           \
					jv[e] = zs[e];                                                                                      \
					jw[e] = 0.0;                                                                                        \
				}                                                                                                       \
			}                                                                                                           \
			FRAMES_ {                                                                                                   \
				double* J = Q.out + (size_t)Q.slot[g] * Q.rows * ld + (size_t)(18 + j) * ld + b;                        \
				const size_t rs = (size_t)n * ld;                                                                       \
				for (int e = 0; e < 3; e++) {                                                                           \
					J[e * rs] = jv[e];                                                                                  \
					J[(3 + e) * rs] = jw[e];                                                                            \
				}                                                                                                       \
			}                                                                                                           \
		}                                                                                                               \
	})

// out = [nf][rows][ld]: rows 0..2 position, 3..11 rotation (row-major), 12..14 linear velocity, 15..17 angular velocity, 18.. the 6 x n
// Jacobian [Jv; Jw] row-major.  Chain: one walk for all frames (sorted by body on the host): each frame is emitted as the walk passes its
// body.  TREE: one walk per frame over the ancestors of its body (the bodies of two frames need not lie on one path).  The pose is the
// arithmetic of fk_control_frame (SAIP_FK_JOINT_STEP): a frame equal to a task's control frame is bit-identical to the pose readback, of a
// tree as well.  The joint axes and origins of the Jacobian are not kept in a per-lane array (runtime-indexed: it would live in scratch):
// they go straight to the output columns, coalesced across the instances, and are read back once p is known.
template <bool TREE>
__global__ void __launch_bounds__(64) saip_model_frames_kernel(const FrameQuery Q) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= Q.B) return;
	const ModelDev& md = *Q.model;
	const double* q = Q.q;
	const size_t ld = Q.ld;
	const int n = Q.n;
	if constexpr (TREE) {
		for (int f = 0; f < Q.nf; f++) {
			const int body = Q.body[f];
			const uint32_t anc = body >= 0 ? md.anc[body] : 0u;
			double tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
			double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
			for (int j = 0; j <= body; j++) {
				if (!((anc >> j) & 1u)) continue;
				MQ_FRAME_JOINT_STEP(const int g = f;)
			}
			frame_emit<true>(Q, md, f, b, R, o, tv, tw, tc);
		}
	} else {
		double tv[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, tc[3] = {0, 0, 0};
		double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
		int f = 0;
		for (; f < Q.nf && Q.body[f] < 0; f++) frame_emit(Q, md, f, b, R, o, tv, tw, tc);  // links welded to the fixed base
		for (int j = 0; f < Q.nf; j++) {
			MQ_FRAME_JOINT_STEP(for (int g = f; g < Q.nf; g++))  // every frame not emitted yet lies on body j or beyond
			for (; f < Q.nf && Q.body[f] == j; f++) frame_emit(Q, md, f, b, R, o, tv, tw, tc);
		}
	}
}

// M (composite rigid bodies), M^-1 (Cholesky), g = RNEA(dq = ddq = 0, base acceleration -gravity) and h = C(q, dq) dq = RNEA(dq, ddq = 0,
// no gravity): the routines of the forward-dynamics step (saip_rbd.h), so M qdd + h + g = tau is the model saip_batch_integrate steps.
// NMAX = 8 walks a chain padded to eight joints: the padding joints of ModelDev are all zero (no mass, no inertia, a zero rotation), add
// exact zeros, and every loop runs to the compile-time bound -- every per-lane array is statically indexed and stays in registers.
// TREE: kinematic trees -- the same queries with the tree traversals of saip_rbd.h.
template <int NMAX, bool TREE>
__global__ void __launch_bounds__(64) saip_model_dynamics_kernel(const DynQuery Q) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= Q.B) return;
	const ModelDev& md = *Q.model;
	const int nn = Q.n;
	const int n = TREE ? nn : (NMAX <= 8 ? NMAX : nn);  // (trees are not padded: padding bodies would hang off body 0)
	const size_t ld = Q.ld;
	constexpr int U = NMAX <= 8 ? NMAX : 1;  // the 32 instantiation keeps its loops rolled (its arrays live in scratch either way)
	double q[NMAX], dq[NMAX], zero[NMAX], t[NMAX];
#pragma unroll
	for (int j = 0; j < NMAX; j++) {
		q[j] = j < nn ? Q.q[(size_t)j * ld + b] : 0.0;
		dq[j] = j < nn ? Q.dq[(size_t)j * ld + b] : 0.0;
		zero[j] = 0.0;
	}
	Chain<NMAX> K;
	if constexpr (TREE) chain_fk_tree<NMAX>(md, n, q, K);
	else chain_fk<NMAX>(md, n, q, K);
	if (Q.g) {
		if constexpr (TREE) rnea_tree<NMAX>(md, n, K, zero, zero, v3(-md.gravity[0], -md.gravity[1], -md.gravity[2]), false, t);
		else rnea<NMAX>(md, n, K, zero, zero, v3(-md.gravity[0], -md.gravity[1], -md.gravity[2]), false, t);
#pragma unroll U
		for (int j = 0; j < NMAX; j++)
			if (j < nn) Q.g[(size_t)j * ld + b] = t[j];
	}
	if (Q.h) {
		if constexpr (TREE) rnea_tree<NMAX>(md, n, K, dq, zero, v3(0, 0, 0), true, t);
		else rnea<NMAX>(md, n, K, dq, zero, v3(0, 0, 0), true, t);
#pragma unroll U
		for (int j = 0; j < NMAX; j++)
			if (j < nn) Q.h[(size_t)j * ld + b] = t[j];
	}
	if (!Q.M && !Q.Minv) return;
	double M[NMAX][NMAX];
	if constexpr (TREE) mass_matrix_crb_tree<NMAX>(md, n, K, M);
	else mass_matrix_crb<NMAX>(md, n, K, M);
	if (Q.M) {
#pragma unroll U
		for (int i = 0; i < NMAX; i++)
#pragma unroll U
			for (int j = 0; j < NMAX; j++)
				if (i < nn && j < nn) Q.M[(size_t)(i * nn + j) * ld + b] = M[i][j];
	}
	if (!Q.Minv) return;
	// Cholesky M = L L^T (lower, in place), then M^-1 column by column: L y = e_c, L^T x = y
#pragma unroll U
	for (int k = 0; k < NMAX; k++) {
		if (k >= nn) break;
		double d = M[k][k];
#pragma unroll U
		for (int l = 0; l < k; l++) d -= M[k][l] * M[k][l];
		d = sqrt(d);
		M[k][k] = d;
		const double rd = 1.0 / d;
#pragma unroll U
		for (int i = k + 1; i < NMAX; i++) {
			if (i >= nn) break;
			double s = M[i][k];
#pragma unroll U
			for (int l = 0; l < k; l++) s -= M[i][l] * M[k][l];
			M[i][k] = s * rd;
		}
	}
#pragma unroll U
	for (int c = 0; c < NMAX; c++) {
		if (c >= nn) break;
		double y[NMAX];
#pragma unroll U
		for (int i = 0; i < NMAX; i++) {
			if (i >= nn) break;
			double s = i == c ? 1.0 : 0.0;
#pragma unroll U
			for (int l = c; l < i; l++) s -= M[i][l] * y[l];
			y[i] = i < c ? 0.0 : s / M[i][i];
		}
#pragma unroll U
		for (int ii = 0; ii < NMAX; ii++) {
			const int i = NMAX - 1 - ii;
			if (i >= nn) continue;
			double s = y[i];
#pragma unroll U
			for (int l = i + 1; l < NMAX; l++)
				if (l < nn) s -= M[l][i] * y[l];
			y[i] = s / M[i][i];
			Q.Minv[(size_t)(i * nn + c) * ld + b] = y[i];
		}
	}
}

hipError_t launch_model_frames(const FrameQuery& Q, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL(saip_model_frames_kernel<true>, dim3((Q.B + 63) / 64), dim3(64), 0, stream, Q);
	else hipLaunchKernelGGL(saip_model_frames_kernel<false>, dim3((Q.B + 63) / 64), dim3(64), 0, stream, Q);
	return hipGetLastError();
}

hipError_t launch_model_dynamics(const DynQuery& Q, bool tree, hipStream_t stream) {
	const int grid = (Q.B + 63) / 64;
	if (tree) {
		if (Q.n <= 8) hipLaunchKernelGGL((saip_model_dynamics_kernel<8, true>), dim3(grid), dim3(64), 0, stream, Q);
		else hipLaunchKernelGGL((saip_model_dynamics_kernel<32, true>), dim3(grid), dim3(64), 0, stream, Q);
		return hipGetLastError();
	}
	if (Q.n <= 8) hipLaunchKernelGGL((saip_model_dynamics_kernel<8, false>), dim3(grid), dim3(64), 0, stream, Q);
	else hipLaunchKernelGGL((saip_model_dynamics_kernel<32, false>), dim3(grid), dim3(64), 0, stream, Q);
	return hipGetLastError();
}

}  // namespace saip
