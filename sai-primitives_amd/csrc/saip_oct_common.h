// Building blocks shared by the eight-lanes-per-instance kernels (saip_kernel_oct.hip, saip_dynamics_oct.hip): lane r of an 8-lane group
// owns joint r / row r of its instance; two instances share a 16-lane DPP row.
#pragma once
#include <hip/hip_runtime.h>

namespace saip {

#define UNR _Pragma("unroll")

// a load through a pointer that was itself read from memory (TaskDev::goal, ::integ): the compiler only knows it as a generic address and emits
// flat_load, which may complete out of order with the global loads around it -- every wait behind it then becomes a wait for EVERYTHING in
// flight (vmcnt(0)).  The arrays are in HBM: say so, and the waits stay counted.
__device__ __forceinline__ double saip_ldg(const double* p, const size_t i) {
	typedef const double __attribute__((address_space(1))) * gptr_t;
	return ((gptr_t)(unsigned long long)p)[i];
}

// 1/x and 1/sqrt(x) from the hardware estimates plus two Newton steps: full double accuracy for the normal-range, positive arguments met
// here (pivots of SPD factorisations), without the scaling / fix-up sequences of the IEEE division and the library rsqrt
__device__ __forceinline__ double oct_rcp(const double x) {
	double y = __builtin_amdgcn_rcp(x);
	y = fma(fma(-x, y, 1.0), y, y);
	return fma(fma(-x, y, 1.0), y, y);
}
__device__ __forceinline__ double oct_rsqrt(const double x) {
	double y = __builtin_amdgcn_rsq(x);
	const double h = 0.5 * x;
	y = fma(y, fma(-h * y, y, 0.5), y);
	return fma(y, fma(-h * y, y, 0.5), y);
}

// value of the lane `n` positions up (row_shl) / down (row_shr) inside the 16-lane DPP row, 0 beyond it: a VALU move, no LDS round trip.
// Callers mask the lanes whose source sits in the neighbouring instance (two instances share a row).
template <int CTRL>
__device__ __forceinline__ double oct_dpp(const double x) {
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
enum { DPP_ROW_SHL = 0x100, DPP_ROW_SHR = 0x110, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_ROR = 0x120 };

// Which block of instances a workgroup takes.  The dispatcher is observed to deal workgroups round-robin over the 8 XCDs (workgroups w and w + 8
// share one; MI355X_MICROARCH.md "Workgroup dispatch, XCD placement"), each with a private L2.  With block = blockIdx, neighbouring blocks -- which
// share cache lines of every [row][ld] input array (8 instances x 8 B = half a 128-B line per row for the eight-lane kernels, ONE double per row for
// the wavefront-per-instance kernel) -- sit on different XCDs, and every line is fetched from HBM once per XCD that touches it (measured, round 3 / 4:
// 2.15 x the algorithmic bytes on config 2, 8 x on config 5).  This bijective remap gives the workgroups of one XCD a contiguous range of blocks.
// A speed choice only: any other placement reads the same values.
// Used by the wavefront-per-instance kernel only (config 5, same session: 172.7 -> 170.2 us per launch, HBM traffic 65 -> 11 MB against 7.5 MB
// algorithmic).  The eight-lane kernels were measured with it as well and run on plain blockIdx: their traffic fell as expected (config 2: 4.6 ->
// 2.7 MB per launch against 2.2 algorithmic) but every launch got SLOWER (config 2 6.67 -> 6.92 us, config 3 13.53 -> 13.85, config 4's shard 9.61 ->
// 10.02) -- at 4 % of the HBM peak the bytes are not what these kernels wait for, and neighbouring workgroups that miss on the
// same line at the same moment queue behind one another in one L2 instead of missing in parallel in two.
__device__ __forceinline__ int saip_xcd_block(const unsigned orig, const unsigned nwg) {
	const unsigned q = nwg >> 3, r = nwg & 7u, x = orig & 7u;
	return (int)((x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (orig >> 3));
}

// ---------------------------------------------------------------- lane layout
// Eight lanes per instance, eight instances per wavefront, two instances per 16-lane DPP row, INTERLEAVED: the two instances of a row take its
// even and its odd lanes (joint r of instance 2 row + parity sits in lane 16 row + 2 r + parity).  Every boundary of a scan along the chain is
// then a ROW boundary, which DPP handles by itself (bound_ctrl zero fill, or the untouched `old` operand for an identity) -- with the two
// instances side by side (lanes 0-7 / 8-15) every scan step needed a select per moved register: a third of the instructions of the
// wavefront's longest phase (doubling them cost 4.5 % of the launch, measured).
__device__ __forceinline__ int octl_r(const int lane) { return (lane >> 1) & 7; }
__device__ __forceinline__ int octl_grp(const int lane) { return ((lane >> 4) << 1) | (lane & 1); }
// the lane that holds joint j of this lane's instance
__device__ __forceinline__ int octl_src(const int lane, const int j) { return (lane & 0x31) | (j << 1); }
// the votes of the eight lanes of this lane's instance, bit r = joint r
__device__ __forceinline__ unsigned octl_votes(const unsigned long long ballot, const int lane) {
	unsigned x = (unsigned)((ballot >> (16 * (lane >> 4))) & 0xffffull) >> (lane & 1);  // the row's votes, this instance's on the even bits
	x &= 0x5555u;
	x = (x | (x >> 1)) & 0x3333u;
	x = (x | (x >> 2)) & 0x0f0fu;
	x = (x | (x >> 4)) & 0x00ffu;
	return x;
}
// sum / maximum over the eight lanes of an instance, every lane gets the result (rotations by 4 and 8 inside the row keep the parity)
__device__ __forceinline__ double octl_sum(double x) {
	x += oct_dpp<DPP_QUAD_XOR2>(x);
	x += oct_dpp<DPP_ROW_ROR + 4>(x);
	return x + oct_dpp<DPP_ROW_ROR + 8>(x);
}
__device__ __forceinline__ double octl_max(double x) {
	x = fmax(x, oct_dpp<DPP_QUAD_XOR2>(x));
	x = fmax(x, oct_dpp<DPP_ROW_ROR + 4>(x));
	return fmax(x, oct_dpp<DPP_ROW_ROR + 8>(x));
}
// the three exchange steps of a butterfly over the eight lanes of an instance (arg-max with its index, ...)
constexpr int OCT_BFLY0 = DPP_QUAD_XOR2, OCT_BFLY1 = DPP_ROW_ROR + 4, OCT_BFLY2 = DPP_ROW_ROR + 8;
// arg-max over the eight lanes of an instance: every lane ends with the largest `best` and the joint index `idx` that came with it (ties: the
// lowest index).  A macro, not a function: as a function taking references the kernels built under max-ilp scheduling came out different
// (more instructions, scratch or registers in 14 of 16 instantiations of saip_cycle_oct).
#define OCT_ARGMAX_STEP(CTRL, best, idx)                                                                        \
	{                                                                                                           \
		const double ob = oct_dpp<CTRL>(best);                                                                  \
		const int oj = __builtin_amdgcn_update_dpp(0, idx, CTRL, 0xF, 0xF, true);                               \
		const bool take = ob > best || (ob == best && oj < idx);                                                \
		best = take ? ob : best;                                                                                \
		idx = take ? oj : idx;                                                                                  \
	}
#define OCT_ARGMAX(best, idx)            \
	OCT_ARGMAX_STEP(OCT_BFLY0, best, idx) \
	OCT_ARGMAX_STEP(OCT_BFLY1, best, idx) \
	OCT_ARGMAX_STEP(OCT_BFLY2, best, idx)
// value of joint r - D (shr) / r + D (shl) of the same instance; lanes without such a joint get `fill` (0 or 1: the identity's diagonal)
template <int D, bool ONE>
__device__ __forceinline__ double octl_shr(const double x) {
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), DPP_ROW_SHR + 2 * D, 0xF, 0xF, true);
	const int hi = ONE ? __builtin_amdgcn_update_dpp(0x3FF00000, __double2hiint(x), DPP_ROW_SHR + 2 * D, 0xF, 0xF, false)
					   : __builtin_amdgcn_update_dpp(0, __double2hiint(x), DPP_ROW_SHR + 2 * D, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
template <int D>
__device__ __forceinline__ double octl_shl(const double x) {
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), DPP_ROW_SHL + 2 * D, 0xF, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), DPP_ROW_SHL + 2 * D, 0xF, 0xF, true);
	return __hiloint2double(hi, lo);
}
// one step of the prefix product of the frames along the chain: T_r <- T_{r-D} o T_r, (Ra,oa) o (Rb,ob) = (Ra Rb, oa + Ra ob); lanes without
// a predecessor compose with the identity
#define OCT_FRAME_STEP(D, Tw)                                                                                                        \
	{                                                                                                                                \
		double Xa[12], Tn[12];                                                                                                       \
		UNR for (int e = 0; e < 12; e++) Xa[e] = (e == 0 || e == 4 || e == 8) ? octl_shr<D, true>(Tw[e]) : octl_shr<D, false>(Tw[e]); \
		UNR for (int i = 0; i < 3; i++) {                                                                                            \
			UNR for (int j = 0; j < 3; j++) Tn[3 * i + j] = Xa[3 * i] * Tw[j] + Xa[3 * i + 1] * Tw[3 + j] + Xa[3 * i + 2] * Tw[6 + j];  \
			Tn[9 + i] = Xa[9 + i] + Xa[3 * i] * Tw[9] + Xa[3 * i + 1] * Tw[10] + Xa[3 * i + 2] * Tw[11];                            \
		}                                                                                                                            \
		UNR for (int e = 0; e < 12; e++) Tw[e] = Tn[e];                                                                              \
	}


__device__ __forceinline__ void oct_mat3_vec(const double* R, const double* v, double* out) {
	UNR for (int i = 0; i < 3; i++) out[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

// Cholesky factor of an SPD R x R matrix given by its lower triangle; L overwrites A's lower triangle, dinv = 1 / L_kk
template <int R>
__device__ __forceinline__ void oct_cholesky(double (&L)[R][R], double (&dinv)[R]) {
	UNR for (int k = 0; k < R; k++) {
		const double rs = oct_rsqrt(L[k][k]);
		dinv[k] = rs;
		UNR for (int i = k + 1; i < R; i++) L[i][k] *= rs;
		UNR for (int j = k + 1; j < R; j++)
			UNR for (int i = j; i < R; i++) L[i][j] = fma(-L[i][k], L[j][k], L[i][j]);
	}
}
// x = (L L^T)^-1 e_col, i.e. column (= row) `col` of the inverse; col is a lane variable
template <int R>
__device__ __forceinline__ void oct_solve_unit(const double (&L)[R][R], const double (&dinv)[R], const int col, double (&x)[R]) {
	double y[R];
	UNR for (int i = 0; i < R; i++) {
		double s = (i == col) ? 1.0 : 0.0;
		UNR for (int k = 0; k < i; k++) s = fma(-L[i][k], y[k], s);
		y[i] = s * dinv[i];
	}
	UNR for (int i = R - 1; i >= 0; i--) {
		double s = y[i];
		UNR for (int k = i + 1; k < R; k++) s = fma(-L[k][i], x[k], s);
		x[i] = s * dinv[i];
	}
}

// x = (L L^T)^-1 b for any right-hand side held by the lane
template <int R>
__device__ __forceinline__ void oct_solve(const double (&L)[R][R], const double (&dinv)[R], const double (&b)[R], double (&x)[R]) {
	double y[R];
	UNR for (int i = 0; i < R; i++) {
		double s = b[i];
		UNR for (int k = 0; k < i; k++) s = fma(-L[i][k], y[k], s);
		y[i] = s * dinv[i];
	}
	UNR for (int i = R - 1; i >= 0; i--) {
		double s = y[i];
		UNR for (int k = i + 1; k < R; k++) s = fma(-L[k][i], x[k], s);
		x[i] = s * dinv[i];
	}
}

// inverse of an SPD R x R matrix given by its lower triangle
template <int R>
__device__ __forceinline__ void oct_spd_inverse_n(const double (&A)[R][R], double (&Ainv)[R][R]) {
	double L[R][R], dinv[R], x[R];
	UNR for (int i = 0; i < R; i++)
		UNR for (int j = 0; j <= i; j++) L[i][j] = A[i][j];
	oct_cholesky<R>(L, dinv);
	UNR for (int col = 0; col < R; col++) {
		oct_solve_unit<R>(L, dinv, col, x);
		UNR for (int i = 0; i < R; i++) Ainv[i][col] = x[i];
	}
}

// eigen-decomposition of a symmetric R x R matrix (R = 4, 6) held, identically, by all eight lanes of an instance: round-robin Jacobi.
// The R/2 rotations of a round touch disjoint index pairs, so they are computed at the same time in different lanes (lane m of each
// quad takes pair m; the reciprocal / rsqrt chains are most of a rotation's cost), broadcast inside the quad by DPP quad_perm and applied
// by every lane to its copy of A; the eigenvector matrix is distributed (lane i < R keeps row i: 4 instead of 4 R operations per
// rotation) and gathered at the end.  Wave-uniform convergence test per sweep.  Eigenvalues on the diagonal of A, eigenvectors in the
// columns of V (all lanes alike).  (The row-cyclic form this replaces computed every rotation in every lane: 92 instructions per pair
// against ~49 now; config 14: 37 k clocks of the blended block's 100 k.)
template <int R>
__device__ __forceinline__ void oct_jacobi_n(double (&A)[R][R], double (&V)[R][R], const int lane) {
	static_assert(R == 4 || R == 6, "even sizes with at most three pairs per round");
	constexpr int NP = R / 2, RM = R - 1;
	// which pair of a round this lane computes.  A quad holds joints 2 q, 2 q + 1 of two instances -- even joints take pair 0, odd joints pair 1
	// (quad_perm [0,1,0,1] / [2,3,2,3] hands them to the quad's lanes of the same instance), and the third pair of a 6 x 6 round is computed by
	// every lane itself (fetching all three by ds_bpermute from joints 0, 1, 2 measured the same or slower: config 12 27.4 vs 26.7 us).
	const int r = octl_r(lane), m = r & 1;
	// t = tan of the rotation angle: sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (aqq - app) / (2 apq), written without the
	// division by apq; hardware reciprocal / rsqrt estimates + Newton steps (arguments are positive and in range)
	auto rotation = [](const double apq, const double app, const double aqq, double& cs, double& sn, double& tn) {
		const double d = aqq - app, b2 = 2.0 * apq;
		const double x = fma(d, d, b2 * b2);
		const bool rot = x > 1e-300;
		const double h = rot ? x * oct_rsqrt(x) : 1.0;
		const double tm = fabs(b2) * oct_rcp(fabs(d) + h);
		tn = rot ? (((d >= 0.0) == (b2 >= 0.0)) ? tm : -tm) : 0.0;
		cs = oct_rsqrt(fma(tn, tn, 1.0));
		sn = tn * cs;
	};
	double vrow[R];
	UNR for (int j = 0; j < R; j++) vrow[j] = (j == r) ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 12; sweep++) {
		double off = 0.0, dg = 0.0;
		UNR for (int p = 0; p < R; p++) {
			dg = fma(A[p][p], A[p][p], dg);
			UNR for (int q = p + 1; q < R; q++) off = fma(A[p][q], A[p][q], off);
		}
		if (!__any(off > 1e-32 * dg)) break;  // every instance of the wavefront has converged (quadratic convergence: 3 - 6 sweeps)
		UNR for (int t = 0; t < RM; t++) {
			// tournament round t: (t, R-1) and ((t + j) mod (R-1), (t - j) mod (R-1)), j = 1 .. R/2 - 1
			double apq = 0.0, app = 0.0, aqq = 0.0;
			UNR for (int j = 0; j < NP; j++) {
				const int a_ = j == 0 ? t : (t + j) % RM, b_ = j == 0 ? RM : (t + RM - j) % RM;
				const int p = a_ < b_ ? a_ : b_, q = a_ < b_ ? b_ : a_;
				const bool mine = m == j;
				apq = mine ? A[p][q] : apq;
				app = mine ? A[p][p] : app;
				aqq = mine ? A[q][q] : aqq;
			}
			double cs, sn, tn, cs2 = 1.0, sn2 = 0.0, tn2 = 0.0;
			rotation(apq, app, aqq, cs, sn, tn);
			if (NP == 3) {  // the third pair of the round, in every lane
				const int a_ = (t + 2) % RM, b_ = (t + RM - 2) % RM;
				const int p = a_ < b_ ? a_ : b_, q = a_ < b_ ? b_ : a_;
				rotation(A[p][q], A[p][p], A[q][q], cs2, sn2, tn2);
			}
			UNR for (int j = 0; j < NP; j++) {
				const int a_ = j == 0 ? t : (t + j) % RM, b_ = j == 0 ? RM : (t + RM - j) % RM;
				const int p = a_ < b_ ? a_ : b_, q = a_ < b_ ? b_ : a_;
				double c, s_, tj;
				if (j == 0) { c = oct_dpp<0x44>(cs); s_ = oct_dpp<0x44>(sn); tj = oct_dpp<0x44>(tn); }
				else if (j == 1) { c = oct_dpp<0xEE>(cs); s_ = oct_dpp<0xEE>(sn); tj = oct_dpp<0xEE>(tn); }
				else { c = cs2; s_ = sn2; tj = tn2; }
				const double apq_j = A[p][q];
				UNR for (int k = 0; k < R; k++) {
					if (k != p && k != q) {
						const double akp = A[k][p], akq = A[k][q];
						const double np_ = c * akp - s_ * akq, nq_ = s_ * akp + c * akq;
						A[k][p] = np_;
						A[p][k] = np_;
						A[k][q] = nq_;
						A[q][k] = nq_;
					}
				}
				A[p][p] = fma(-tj, apq_j, A[p][p]);
				A[q][q] = fma(tj, apq_j, A[q][q]);
				A[p][q] = 0.0;
				A[q][p] = 0.0;
				const double vp = vrow[p], vq = vrow[q];
				vrow[p] = c * vp - s_ * vq;
				vrow[q] = s_ * vp + c * vq;
			}
		}
	}
	UNR for (int i = 0; i < R; i++)
		UNR for (int c = 0; c < R; c++) V[i][c] = __shfl(vrow[c], octl_src(lane, i));
}
__device__ __forceinline__ void oct_jacobi4(double (&A)[4][4], double (&V)[4][4], const int lane) { oct_jacobi_n<4>(A, V, lane); }
__device__ __forceinline__ void oct_spd_inverse4(const double (&A)[4][4], double (&Ainv)[4][4]) { oct_spd_inverse_n<4>(A, Ainv); }

// cyclic Jacobi eigen-solve of a symmetric n x n matrix in LDS by ONE lane (rare exact path): eigenvalues on the diagonal of A,
// eigenvectors in the columns of V (optional)
__device__ inline void oct_serial_jacobi(double* A, double* V, const int n, const int ld) {
	if (V)
		for (int i = 0; i < n; i++)
			for (int j = 0; j < n; j++) V[i * ld + j] = (i == j) ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 14; sweep++) {
		double off = 0.0, dg = 0.0;
		for (int p = 0; p < n; p++) {
			dg = fma(A[p * ld + p], A[p * ld + p], dg);
			for (int q = p + 1; q < n; q++) off = fma(A[p * ld + q], A[p * ld + q], off);
		}
		if (!(off > 1e-36 * dg)) break;
		for (int p = 0; p < n - 1; p++)
			for (int q = p + 1; q < n; q++) {
				const double apq = A[p * ld + q];
				if (apq == 0.0) continue;
				const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
				const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
				const double c = rsqrt(fma(t, t, 1.0)), s = t * c;
				for (int k = 0; k < n; k++) {  // A <- A R (columns p, q)
					const double akp = A[k * ld + p], akq = A[k * ld + q];
					A[k * ld + p] = c * akp - s * akq;
					A[k * ld + q] = s * akp + c * akq;
				}
				for (int k = 0; k < n; k++) {  // A <- R^T A (rows p, q)
					const double apk = A[p * ld + k], aqk = A[q * ld + k];
					A[p * ld + k] = c * apk - s * aqk;
					A[q * ld + k] = s * apk + c * aqk;
				}
				if (V)
					for (int k = 0; k < n; k++) {
						const double vkp = V[k * ld + p], vkq = V[k * ld + q];
						V[k * ld + p] = c * vkp - s * vkq;
						V[k * ld + q] = s * vkp + c * vkq;
					}
			}
	}
}

}  // namespace saip
