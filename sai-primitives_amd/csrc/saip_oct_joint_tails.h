// The rarely-run ends of the eight-lane cycle (saip_kernel_oct.hip: oct_cycle_body), compiled into the general (FULL) instantiations only:
// the joint task behind a motion-force task that leaves it more than one direction -- any selection matrix with <= 4 rows (GJ == 1), a full
// joint task in a nullspace of rank 2..5 (GJ == 2) -- and the joint-limit-avoidance wrap.  Lane r of an instance owns joint r / column r.
// With them what they share with the body: the instance's LDS block and the synchronisation inside it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "saip_device.h"
#include "saip_law.h"
#include "saip_oct_common.h"

namespace saip {

// the cycle's LDS block per instance
struct OctInst {
	union {  // the kinematics scratch is dead before the task matrices are written
		double X[8][12];     // world frame per joint: R (9, row-major) + o (3)
		struct {
			double T1[6][8], A[8][8], Am[8][8], Lam[8][8];  // Lam also carries J M_BIE^-1 until Lambda exists; rows 6, 7: padding lanes' scratch
			double N1[8][8];
		};
	};
	double M[8][8];      // lower triangle of M(q), row r by lane r; kept to the end (the blended singularity strategies want M z)
	double zo[8][6];     // joint motion vector about the world origin S_r = (w, v): revolute (z, o x z), prismatic (0, z)
	double J[6][8];
	double vec[13][8];   // 0 dq, 1 tau, 2 g, 3 / 4 row and scalar exchanges, 5 goal force + moment (general laws), 7 u, 8 d, 9 flags, 10..12 motion-force goal (24)
	double ist[10];      // integrator state, fetched with the inputs: 0..5 motion-force task (position, orientation), 6..9 the rows of a Gram-path joint
	                     // task; the control law leaves the advanced motion-force values here for the epilogue.  (Also the padding that makes the
	                     // instance stride = 2 (mod 32) doubles: the eight instances of a wavefront hit different LDS banks.)
};
static_assert(sizeof(OctInst) % 256 == 16, "instance stride must be 2 (mod 32) doubles");
static_assert(sizeof(OctInst) * 8 * 4 <= 160 * 1024, "four wavefronts per CU (one LDS block each, also with two wavefronts per instance group)");

// synchronisation inside a wavefront's instance blocks: wavefront-local in the two-wavefront form (DUO, see oct_cycle_body), a workgroup
// barrier of the one wavefront otherwise
template <bool DUO>
__device__ __forceinline__ void oct_sync() {
	if (DUO) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	} else {
		__syncthreads();
	}
}

// Lambda = (Jh M^-1 Jh^T)^-1 and Lambda_mod of a joint task reduced to R range directions (JointTask.cpp:241-267), every lane alike.  Jh: the
// R x N reduced Jacobian in full, jh: this lane's column of it; mi / mb: this lane's column of M^-1 / M_BIE^-1, mcol: column e of M^-1 for the
// rank-one bounded-inertia form (at most one clamped entry e, beta = c / (1 + c (M^-1)_ee)); dropped directions are padded with a unit diagonal.
template <int R, int N>
__device__ __forceinline__ void oct_lambda_mod(double (&Lam)[R][R], double (&Lmod)[R][R], const double (&Jh)[R][N], const double (&jh)[R], const double (&mi)[N],
                                               const double (&mb)[N], const double (&mcol)[N], const double beta, const int jt_dec, const bool general_bie,
                                               const bool (&dropped)[R], const bool act) {
	double t1v[R], AR[R][R];
	UNR for (int c = 0; c < R; c++) {
		double st = 0.0;
		UNR for (int l = 0; l < N; l++) st = fma(Jh[c][l], mi[l], st);  // (Jh M^-1)[c][rr]: M^-1 symmetric
		t1v[c] = act ? st : 0.0;
	}
	UNR for (int c = 0; c < R; c++)
		UNR for (int k = 0; k <= c; k++) {
			const double gs = octl_sum(t1v[c] * jh[k]);
			AR[c][k] = (c == k && dropped[c]) ? 1.0 : gs;
		}
	oct_spd_inverse_n<R>(AR, Lam);
	if (jt_dec == DEC_FULL) {
		UNR for (int c = 0; c < R; c++)
			UNR for (int k = 0; k < R; k++) Lmod[c][k] = Lam[c][k];
	} else if (jt_dec == DEC_IMPEDANCE) {
		UNR for (int c = 0; c < R; c++)
			UNR for (int k = 0; k < R; k++) Lmod[c][k] = (c == k) ? 1.0 : 0.0;
	} else if (general_bie) {
		double tbv[R];
		UNR for (int c = 0; c < R; c++) {
			double st = 0.0;
			UNR for (int l = 0; l < N; l++) st = fma(Jh[c][l], mb[l], st);
			tbv[c] = act ? st : 0.0;
		}
		UNR for (int c = 0; c < R; c++)
			UNR for (int k = 0; k <= c; k++) {
				const double gs = octl_sum(tbv[c] * jh[k]);
				AR[c][k] = (c == k && dropped[c]) ? 1.0 : gs;
			}
		oct_spd_inverse_n<R>(AR, Lmod);
	} else {  // rank-one bounded-inertia form: Lambda_mod = Lambda + gamma (Lambda t)(Lambda t)^T, t = Jh m
		double t[R], lt[R], qq = 0.0;
		UNR for (int c = 0; c < R; c++) {
			double st = 0.0;
			UNR for (int l = 0; l < N; l++) st = fma(Jh[c][l], mcol[l], st);
			t[c] = st;
		}
		UNR for (int c = 0; c < R; c++) {
			double sl = 0.0;
			UNR for (int k = 0; k < R; k++) sl = fma(Lam[c][k], t[k], sl);
			lt[c] = sl;
			qq = fma(t[c], sl, qq);
		}
		const double gamma = beta * oct_rcp(fma(-beta, qq, 1.0));
		UNR for (int c = 0; c < R; c++)
			UNR for (int k = 0; k < R; k++) Lmod[c][k] = fma(gamma * lt[c], lt[k], Lam[c][k]);
	}
}

// ---------------------------------------------------------------- JointTask, general path (GJ == 1): any selection matrix with m <= 4 rows behind any
// motion-force task.  Lane j holds column j of Jp = S N_1 (m x 7): cj is column rr of N_1.  Left singular vectors / squared singular values of
// Jp = eigen-pairs of its 4 x 4 Gram matrix (sums over the lanes by DPP), by an unrolled Jacobi solve in registers; matrixRangeBasis keeps the
// directions with sigma_i / sigma_0 >= 1e-3 (JointTask.cpp:233); the rest of the task algebra is r x r with dropped directions padded.
// jg: this lane's goal row (position, velocity, acceleration); tau_r: the torque of the task in front; returns the torque behind this one and
// leaves the advanced integrator of task row r in jt_ie_new.
template <bool DUO, int N>
__device__ __forceinline__ double oct_joint_tail_gram(const CycleParams& P, OctInst& sm, const int lane, const double (&cj)[N], const double (&mi)[N], const double (&mb)[N],
                                                      const double (&mcol)[N], const double beta, const bool general_bie, const int jt_dec, const double q_r,
                                                      const double (&jg)[3], const double tau_r, double& jt_ie_new) {
	const TaskDev& jt = P.tasks[1];
	const int r = octl_r(lane), mj = jt.m;
	const bool act = r < N;
	double cp[4];
	UNR for (int i = 0; i < 4; i++) {
		double sc = 0.0;
		UNR for (int l = 0; l < N; l++) sc = fma(jt.S[i * N + l], cj[l], sc);  // rows >= m of the stored S are zero
		cp[i] = act ? sc : 0.0;
	}
	double Gp[4][4], V4[4][4], trp = 0.0;
	UNR for (int i = 0; i < 4; i++)
		UNR for (int k = 0; k <= i; k++) {
			const double gs = octl_sum(cp[i] * cp[k]);
			Gp[i][k] = gs;
			Gp[k][i] = gs;
			if (i == k) trp += gs;
		}
	// Usual case: Jp has full row rank, matrixRangeBasis returns the identity (sai-model: task_dof == rows) and no eigen-solve is needed.
	// Certificate (the one of the motion-force branch predicate): lambda_max <= trace, so a positive definite  Gp - 1e-6 trace I  on
	// the m task rows proves sigma_min / sigma_max > 1e-3; trace / m >= 1e-6 proves sigma_max >= 1e-3.  Only wavefronts that hold an
	// instance it cannot decide run the register Jacobi solve (measured, config 3: 19 k of 40 k clocks per wavefront were this solve).
	bool full_rank = trp * 0.25 >= 1e-6;
	{
		double Gs[4][4];
		const double sh = 1e-6 * trp;
		UNR for (int i = 0; i < 4; i++)
			UNR for (int k = 0; k <= i; k++) Gs[i][k] = Gp[i][k];
		UNR for (int i = 0; i < 4; i++) Gs[i][i] = (i < mj) ? Gs[i][i] - sh : 1.0;
		UNR for (int kk = 0; kk < 4; kk++) {
			const double d = Gs[kk][kk];
			full_rank = full_rank && (d > 1e-13 * trp);
			const double id = oct_rcp(d);
			UNR for (int i = kk + 1; i < 4; i++) {
				const double lik = Gs[i][kk] * id;
				UNR for (int k = kk + 1; k <= i; k++) Gs[i][k] = fma(-lik, Gs[k][kk], Gs[i][k]);
			}
		}
	}
#if defined(SAIP_OCT_FORCE_EXACT)
	full_rank = false;
#endif
	bool keep[4];
	double jh[4];
	UNR for (int i = 0; i < 4; i++)
		UNR for (int k = 0; k < 4; k++) V4[i][k] = (i == k) ? 1.0 : 0.0;
	UNR for (int c = 0; c < 4; c++) {
		keep[c] = c < mj;
		jh[c] = keep[c] ? cp[c] : 0.0;
	}
	if (__any(!full_rank)) {
		double Ve[4][4];
		oct_jacobi4(Gp, Ve, lane);
		double lmaxp = 0.0;
		UNR for (int c = 0; c < 4; c++) lmaxp = fmax(lmaxp, Gp[c][c]);
		const bool any_range = (sqrt(fmax(trp, 0.0)) >= 1e-3) && (sqrt(lmaxp) >= 1e-3);
		UNR for (int c = 0; c < 4; c++) {
			const bool kc = any_range && (sqrt(fmax(Gp[c][c], 0.0) / lmaxp) >= 1e-3);
			double sj = 0.0;
			UNR for (int i = 0; i < 4; i++) sj = fma(Ve[i][c], cp[i], sj);
			if (!full_rank) {
				keep[c] = kc;
				jh[c] = kc ? sj : 0.0;  // own column of Jh = U^T Jp
				UNR for (int i = 0; i < 4; i++) V4[i][c] = Ve[i][c];
			}
		}
	}
	// gather Jh, q, the joint-task goal rows and w = M^-1 tau_prec for the whole instance
	double tauv[N];
	UNR for (int j = 0; j < N; j++) tauv[j] = sm.vec[1][j];
	double wr = 0.0;
	UNR for (int l = 0; l < N; l++) wr = fma(mi[l], tauv[l], wr);
	UNR for (int c = 0; c < 4; c++) sm.T1[c][r] = jh[c];
	sm.vec[4][r] = wr;
	sm.vec[6][r] = q_r;
	sm.vec[7][r] = jg[0];
	sm.vec[8][r] = jg[1];
	sm.vec[3][r] = jg[2];
	oct_sync<DUO>();
	double Jh[4][N];
	UNR for (int c = 0; c < 4; c++)
		UNR for (int j = 0; j < N; j++) Jh[c][j] = sm.T1[c][j];
	double Lam4[4][4], Lmod4[4][4];
	bool dropped[4];
	UNR for (int c = 0; c < 4; c++) dropped[c] = !keep[c];
	oct_lambda_mod<4, N>(Lam4, Lmod4, Jh, jh, mi, mb, mcol, beta, jt_dec, general_bie, dropped, act);
	// control law of the (at most four) task rows, every lane alike (JointTask.cpp:285-356)
	double qa[N], dqa[N], wa[N];
	UNR for (int j = 0; j < N; j++) {
		qa[j] = sm.vec[6][j];
		dqa[j] = sm.vec[0][j];
		wa[j] = sm.vec[4][j];
	}
	const bool track = (jt.has_ki || P.integ_always);
	double a1[4] = {0, 0, 0, 0}, b1[4] = {0, 0, 0, 0};
	UNR for (int i = 0; i < 4; i++) {
		double cur = 0.0, vel = 0.0, sw = 0.0;
		UNR for (int l = 0; l < N; l++) {
			const double sil = jt.S[i * N + l];
			cur = fma(sil, qa[l], cur);
			vel = fma(sil, dqa[l], vel);
			sw = fma(sil, wa[l], sw);
		}
		const bool row = i < mj;
		const double gq = row ? sm.vec[7][i] : 0.0, gdq = row ? sm.vec[8][i] : 0.0, gddq = row ? sm.vec[3][i] : 0.0;
		const double e = cur - gq;
		double ie = (track && row) ? sm.ist[6 + i] : 0.0;
		ie += e * jt.dt;  // :323-324
		jt_ie_new = (r == i) ? ie : jt_ie_new;  // lane i keeps row i for the epilogue
		double fi;
		if (jt.vel_sat) {  // :327-341
			double vdes = -jt.kp[i] * jt.kvinv[i] * e - jt.ki[i] * jt.kvinv[i] * ie;
			vdes = fmin(fmax(vdes, -jt.sat[i]), jt.sat[i]);
			fi = -jt.kv[i] * (vel - vdes);
		} else {
			fi = -jt.kp[i] * e - jt.kv[i] * (vel - gdq) - jt.ki[i] * ie;  // :342-345
		}
		const double ai = gddq - sw;
		UNR for (int c = 0; c < 4; c++) {
			a1[c] = fma(V4[i][c], row ? ai : 0.0, a1[c]);
			b1[c] = fma(V4[i][c], row ? fi : 0.0, b1[c]);
		}
	}
	double tj = tau_r;
	UNR for (int c = 0; c < 4; c++) {
		double gc = 0.0;
		UNR for (int k = 0; k < 4; k++) gc = fma(Lam4[c][k], a1[k], fma(Lmod4[c][k], b1[k], gc));  // :348-351
		tj = fma(jh[c], keep[c] ? gc : 0.0, tj);  // tau += Jh^T g
	}
	return tj;
}

// ---------------------------------------------------------------- full joint task (S = I, GJ == 2) behind a motion-force task of rank k < 6: Jp = N_1 has
// rank 7 - k (2..5).  Column-pivoted Gram-Schmidt over the instance's lanes (lane j owns column j, cj): arg-max of the column norms by
// a DPP butterfly carrying the index, the pivot column travels by ds_bpermute, the deflation coefficients are the rows of
// Jh = U^T Jp (the same clean-gap rule as the lane kernel; an ambiguous gap is reported in `bad` -- status 1 -- never silently truncated).
// rmax: wave-uniform bound on the rank; fi / ddq_d: this joint's PD(I) force and goal acceleration; returns the torque behind this task.
template <bool DUO, int N>
__device__ __forceinline__ double oct_joint_tail_pivoted(OctInst& sm, const int lane, const double (&cj)[N], const double (&mi)[N], const double (&mb)[N], const double (&mcol)[N],
                                                         const double beta, const bool general_bie, const int jt_dec, const int rmax, const double fi, const double ddq_d,
                                                         const double tau_r, bool& bad) {
	const int r = octl_r(lane), rr = r < N ? r : N - 1;
	const bool act = r < N;
	double Wc[N], jh[5], uown[5];
	UNR for (int i = 0; i < N; i++) Wc[i] = act ? cj[i] : 0.0;
	UNR for (int s5 = 0; s5 < 5; s5++) jh[s5] = uown[s5] = 0.0;
	double c0 = 1.0;
	bool going = true;
	int rank = 0;
	bad = false;
	UNR for (int s5 = 0; s5 <= 5; s5++) {
		if (s5 <= rmax) {
			double cnw = 0.0;
			UNR for (int i = 0; i < N; i++) cnw = fma(Wc[i], Wc[i], cnw);
			double bestw = act ? cnw : -1.0;
			int jbw = r;
			OCT_ARGMAX(bestw, jbw)
			if (s5 == 0) {
				const double frob2 = octl_sum(act ? cnw : 0.0);
				c0 = bestw;
				if (frob2 < 1e-6) going = false;  // ||Jp||_F < 1e-3: empty range
				else if (bestw < 1e-5) { going = false; bad = true; }
			} else if (going) {
				const double ratio = bestw / c0;
				if (ratio < 1e-20) going = false;                         // numerically exact rank below the bound
				else if (ratio < 1e-4 || s5 == rmax) { going = false; bad = true; }  // ambiguous gap, or more directions than 7 - k
			}
			if (s5 < rmax && s5 < 5) {
				const int src = octl_src(lane, jbw);
				const double inv = going ? oct_rsqrt(bestw) : 0.0;
				double u[N], dd = 0.0;
				UNR for (int i = 0; i < N; i++) {
					u[i] = __shfl(Wc[i], src) * inv;
					dd = fma(u[i], Wc[i], dd);
				}
				UNR for (int i = 0; i < N; i++) Wc[i] = fma(-u[i], dd, Wc[i]);
				double uo = 0.0;
				UNR for (int i = 0; i < N; i++) uo = (i == rr) ? u[i] : uo;
				jh[s5 < 5 ? s5 : 0] = act ? dd : 0.0;
				uown[s5 < 5 ? s5 : 0] = act ? uo : 0.0;
				if (going) rank = s5 + 1;
			}
		}
	}
	// Lambda = (Jh M^-1 Jh^T)^-1 (rank x rank, padded to 5): gather Jh, own column of T1, sums over the lanes
	double tauv[N];
	UNR for (int j = 0; j < N; j++) tauv[j] = sm.vec[1][j];
	UNR for (int c = 0; c < 5; c++) sm.T1[c][r] = jh[c];
	oct_sync<DUO>();
	double Jh[5][N];
	UNR for (int c = 0; c < 5; c++)
		UNR for (int j = 0; j < N; j++) Jh[c][j] = sm.T1[c][j];
	double wr = 0.0, Lam5[5][5], Lmod5[5][5];
	UNR for (int l = 0; l < N; l++) wr = fma(mi[l], tauv[l], wr);  // (M^-1 tau_prec)_rr
	bool dropped[5];
	UNR for (int c = 0; c < 5; c++) dropped[c] = c >= rank;
	oct_lambda_mod<5, N>(Lam5, Lmod5, Jh, jh, mi, mb, mcol, beta, jt_dec, general_bie, dropped, act);
	// (the control law of this lane's joint ran behind M(q): fi); its range coordinates by sums over the lanes
	const double ai = ddq_d - wr;
	double a1[5], b1[5];
	UNR for (int c = 0; c < 5; c++) {
		a1[c] = octl_sum(uown[c] * ai);
		b1[c] = octl_sum(uown[c] * fi);
	}
	double tj = tau_r;
	UNR for (int c = 0; c < 5; c++) {
		double gc = 0.0;
		UNR for (int k5 = 0; k5 < 5; k5++) gc = fma(Lam5[c][k5], a1[k5], fma(Lmod5[c][k5], b1[k5], gc));
		tj = fma(jh[c], (c < rank) ? gc : 0.0, tj);
	}
	return tj;
}

// joint limit avoidance wrap, RobotController.cpp:96-112: tau = JLA.computeTorques(tau) + N_c^T tau with
// N_c^T = I - S^T (S M^-1 S^T)^-1 S M^-1 over the joints inside a limit zone (padded to 7 x 7 with identity rows).  The zone logic is
// per joint = per lane; the rest only runs when some instance of the wavefront touches a zone.  mi: this lane's column of M^-1; tv: the
// torque of this lane's joint so far; returns the wrapped one (flagged instances -- singular -- keep theirs).
template <bool DUO, int N>
__device__ __forceinline__ double oct_jla_wrap(const CycleParams& P, OctInst& sm, const int lane, const double q_r, const double dq_r, const double (&mi)[N],
                                               const bool singular, double tv) {
	const ModelDev& md = *P.model;
	const int r = octl_r(lane), rr = r < N ? r : N - 1;
	const bool act = r < N;
	bool zone;
	const double tj = jla_joint(q_r, dq_r, md.q_lower[rr], md.q_upper[rr], md.vel_limit[rr], md.effort[rr], tv, &zone);
	const bool in_zone = zone && act && !singular;
	if (__any(in_zone)) {
		sm.vec[1][r] = tv;
		sm.vec[3][r] = in_zone ? 1.0 : 0.0;
		oct_sync<DUO>();
		double tall[N], zall[N];
		UNR for (int j = 0; j < N; j++) {
			tall[j] = sm.vec[1][j];
			zall[j] = sm.vec[3][j];
		}
		double sacc = 0.0;
		UNR for (int j = 0; j < N; j++) sacc = fma(mi[j], tall[j], sacc);  // (M^-1 tau)_rr
		sm.vec[4][r] = in_zone ? sacc : 0.0;
		UNR for (int j = 0; j < N; j++) sm.N1[r][j] = (in_zone && zall[j] != 0.0) ? mi[j] : ((j == rr) ? 1.0 : 0.0);  // N1 is dead: masked M^-1
		oct_sync<DUO>();
		double L[N][N], dinv[N], y[N], x[N];
		UNR for (int i = 0; i < N; i++)
			UNR for (int j = 0; j <= i; j++) L[i][j] = sm.N1[i][j];
		oct_cholesky<N>(L, dinv);
		UNR for (int i = 0; i < N; i++) {
			double sy = sm.vec[4][i];
			UNR for (int k = 0; k < i; k++) sy = fma(-L[i][k], y[k], sy);
			y[i] = sy * dinv[i];
		}
		UNR for (int i = N - 1; i >= 0; i--) {
			double sx = y[i];
			UNR for (int k = i + 1; k < N; k++) sx = fma(-L[k][i], x[k], sx);
			x[i] = sx * dinv[i];
		}
		double yr = 0.0;
		UNR for (int i = 0; i < N; i++) yr = (i == rr) ? x[i] : yr;
		if (in_zone) tv = tj + tv - yr;
		if (P.torque_sat) {
			const double lim = md.effort[rr];
			tv = tv > lim ? lim : (tv < -lim ? -lim : tv);
		}
	}
	return tv;
}

}  // namespace saip
