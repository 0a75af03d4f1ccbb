// Rollout recorder: the observation of ONE closed-loop period of saip_batch_rollout_async, taken right behind the period's integration
// (one lane per instance).  What it observes: the state q, dq as the integration left it, the torques that were applied during the
// period, the status byte of the period's cycle and, for one motion-force task, the pose of its control frame and its selection-projected
// position / orientation error against the user goal at that state.  A sampled period copies the selected channels into one slot of the
// log ring; the running summaries are advanced on every period.  It writes the log, the status log and the summary array and nothing
// else: no task, OTG, integrator, handler, torque or state array is touched.
#include "saip_law.h"
#include "saip_fk.h"

namespace saip {

// |e|^2 of three components as ((e0 e0 + e1 e1) + e2 e2) with every product and sum rounded on its own (no contraction into FMAs): a host
// that has the logged error rows reproduces the summary maxima bit for bit
__device__ __forceinline__ double rec_norm2(const double* e) {
#pragma clang fp contract(off)
	return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// Rows of a sample: q (n), dq (n), tau (n, NaN kept), pose (12: position 3, rotation 9 row-major -- the arithmetic of
// saip_batch_get_current_pose_host), error (6: rows 0..5 of the task diagnostics, saip_task_diag.hip), each only when its REC_* bit is
// set.  Every row is a [ld] array, so a wavefront's stores are contiguous.  Each instance owns its column of the summary array: a plain
// read-modify-write.  TREE: kinematic trees (the walk over the ancestors of the task's body only).
template <bool TREE>
__global__ void __launch_bounds__(64) saip_rollout_record(const RecordParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.B) return;
	const int ld = P.ld, n = P.n;
	const unsigned ch = P.slot >= 0 ? P.channels : 0u;
	const bool sums = P.summary != nullptr;
	double* row = ch ? P.log + ((size_t)P.slot * P.rows) * ld + b : nullptr;  // next row of this sample
	if (ch & REC_Q) {
		for (int j = 0; j < n; j++, row += ld) *row = P.q[(size_t)j * ld + b];
	}
	double vmax = 0.0, tmax = 0.0, tt = 0.0;
	if ((ch & REC_DQ) || sums) {
		for (int j = 0; j < n; j++) {
			const double v = P.dq[(size_t)j * ld + b];
			vmax = fmax(vmax, fabs(v));
			if (ch & REC_DQ) {
				*row = v;
				row += ld;
			}
		}
	}
	if ((ch & REC_TAU) || sums) {
		for (int j = 0; j < n; j++) {
			const double t = P.tau[(size_t)j * ld + b];
			const double t0 = t == t ? t : 0.0;  // a NaN torque is no torque: the integrator coasts
			tmax = fmax(tmax, fabs(t0));
			tt += t0 * t0;
			if (ch & REC_TAU) {
				*row = t;
				row += ld;
			}
		}
	}
	const uint8_t st = P.status[b];
	if (P.slot >= 0) P.status_log[(size_t)P.slot * ld + b] = st;
	double ep2 = 0.0, eo2 = 0.0;
	if (P.task >= 0 && ((ch & (REC_POSE | REC_ERROR)) || sums)) {
		const ModelDev& md = *P.model;
		const TaskDev& task_ref = P.tasks[P.task];
		const double* q = P.q;
		double pos[3], Rc[9];
		{
			const TaskDev& tk = task_ref;  // (the walk names the task `tk`, by reference)
			SAIP_FK_WALK(TREE)
		}
		if (ch & REC_POSE) {
			for (int e = 0; e < 3; e++, row += ld) *row = pos[e];
			for (int e = 0; e < 9; e++, row += ld) *row = Rc[e];
		}
		if ((ch & REC_ERROR) || sums) {
			// sigma_pos (x_goal - x) and sigma_ori orientationError(R_goal, Rc), as the task diagnostics form them
			const TaskDev* const tk = &task_ref;  // (the law's macros take the task by pointer)
			const double* goal = P.goal;
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
			if (ch & REC_ERROR) {
				for (int e = 0; e < 6; e++, row += ld) *row = r[e];
			}
			ep2 = rec_norm2(r);
			eo2 = rec_norm2(r + 3);
		}
	}
	if (sums) {
		double* s = P.summary + b;
		s[0] += P.T * tt;
		s[(size_t)ld] += P.T * ep2;
		s[(size_t)2 * ld] += P.T * eo2;
		s[(size_t)3 * ld] = fmax(s[(size_t)3 * ld], sqrt(ep2));
		s[(size_t)4 * ld] = fmax(s[(size_t)4 * ld], sqrt(eo2));
		s[(size_t)5 * ld] = fmax(s[(size_t)5 * ld], tmax);
		s[(size_t)6 * ld] = fmax(s[(size_t)6 * ld], vmax);
		s[(size_t)7 * ld] += st != 0 ? 1.0 : 0.0;
	}
}

hipError_t launch_rollout_record(const RecordParams& P, bool tree, hipStream_t stream) {
	if (tree) hipLaunchKernelGGL(saip_rollout_record<true>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	else hipLaunchKernelGGL(saip_rollout_record<false>, dim3((P.B + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
