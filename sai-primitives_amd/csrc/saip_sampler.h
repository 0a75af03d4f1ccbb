// Resident rollout sampler (saip_sampler.hip): everything its kernels compute per element -- the counter-based random numbers, the
// perturbation of one instance's keyframes, the cost of one instance, the per-lane parts of the softmin update and what the first lane
// does with the reduced sums -- shared by the kernels and by host-compiled checks (plain C++ when no HIP compiler is reading it).
// Nothing here is contracted into a fused multiply-add: every product and every sum is rounded once, so a host restatement runs the
// same operations in the same order and differs only by what log / sqrt / sin / cos / atan2 / exp of the two maths libraries differ.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAIP_SAMP_HD __host__ __device__
#else
#define SAIP_SAMP_HD
#endif

namespace saip {

enum { SAMP_LANES = 256, SAMP_WAVE = 64, SAMP_MAX_ROWS = 36, SAMP_MAXT = 8, SAMP_SUMMARY_ROWS = 8, SAMP_MAX_SCENARIOS = 64 };
// the risk measure that folds the M scenario costs of one candidate into its group cost (SAIP_SAMPLER_RISK_* of saip.h)
enum { SAMP_RISK_MEAN = 0, SAMP_RISK_MAX = 1, SAMP_RISK_CVAR = 2 };

// the result of one update, resident on the device (saip_batch_sampler_result_host)
struct SamplerResult {
	int best;         // lowest index that attains the minimum finite cost, -1 without a finite cost
	int n_valid;      // finite costs
	double min_cost;  // beta
	double sum_w;     // sum of the weights
	double ess;       // (sum w)^2 / sum w^2
};

// one sampled task.  The sampler coordinates are the rows [0, count) of the schedule's range in order, the nine rotation rows
// (r_rot .. r_rot + 8 inside the range, rot != 0) replaced by three tangent coordinates: d = count - 6 with a rotation, count without.
// count <= SAMP_MAX_ROWS, checked at attach: the per-lane and LDS arrays of the kernels are sized by it.
struct SamplerEntry {
	double* key;          // the schedule's resident keyframes [K][count][ld]
	double* nominal;      // [K][count] the nominal plan, batch-uniform
	const double* sigma;  // [d]
	int count, K, d;
	int rot, r_rot;       // r_rot: first rotation row inside the range (count without a rotation)
	int task;             // task id: part of the random-number counter
	int exempt;           // instances 0 .. exempt - 1 keep the nominal rows
	int pad_;
};
// Scenario groups: a batch of B = C M instances is M scenario blocks of C candidate plans, instance i = s C + c.  C == B (M = 1) is
// the ungrouped sampler: every instance its own candidate.
struct SamplerParams {
	int B, ld, n, C;      // n: entries in use; C: candidates (B without scenario groups)
	uint32_t seed_lo, seed_hi, round, pad2_;
	SamplerEntry e[SAMP_MAXT];
};
struct SamplerCostParams {
	int B, ld;
	const double* summary;  // [8][ld] the recorder's running summaries (nullptr: no summary term)
	const double* log;      // [capacity][rows][ld] the recorder's ring (nullptr: no target terms)
	int rows, pose_row0;    // rows of one sample; first of the three position rows inside it
	int capacity, first_slot, n_samples;  // the ring: slot of the oldest sample and samples held, computed on the host at enqueue time
	int has_target;
	double w[SAMP_SUMMARY_ROWS];
	double target[3];
	double w_path, w_final;
	double* cost;           // [ld]
};

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library)
SAIP_SAMP_HD inline void samp_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
	uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
	for (int r = 0; r < 10; r++) {
		if (r) {
			k0 += 0x9E3779B9u;
			k1 += 0xBB67AE85u;
		}
		const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t)p1;
		c3 = (uint32_t)p0;
		c0 = n0;
		c2 = n2;
	}
	out[0] = c0;
	out[1] = c1;
	out[2] = c2;
	out[3] = c3;
}
// 53 bits of two words as a uniform in (0, 1]: integers, one addition of 0.5 and one exact scaling
SAIP_SAMP_HD inline double samp_uniform(uint32_t hi, uint32_t lo) {
	const uint64_t n = ((uint64_t)(hi >> 5) << 26) + (uint64_t)(lo >> 6);
	return ((double)n + 0.5) * 0x1p-53;
}
// the two uniforms of counter (instance, keyframe, (task << 16) | p, round): words 0, 1 make u1, words 2, 3 make u2
SAIP_SAMP_HD inline void samp_uniforms(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int task, int i, int k, int p, double u[2]) {
	const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)k, ((uint32_t)task << 16) | (uint32_t)p, round}, key[2] = {seed_lo, seed_hi};
	uint32_t w[4];
	samp_philox4x32_10(ctr, key, w);
	u[0] = samp_uniform(w[0], w[1]);
	u[1] = samp_uniform(w[2], w[3]);
}
// Box-Muller: the normals of coordinates 2p and 2p + 1
SAIP_SAMP_HD inline void samp_normals(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int task, int i, int k, int p, double z[2]) {
#pragma clang fp contract(off)
	double u[2];
	samp_uniforms(seed_lo, seed_hi, round, task, i, k, p, u);
	const double r = sqrt(-2.0 * log(u[0])), a = 6.283185307179586 * u[1];
	z[0] = r * cos(a);
	z[1] = r * sin(a);
}

// ---- SO(3), row-major 3 x 3, the forms of the goal schedule's interpolation (saip_goal_schedule.hip)
// out = R0 Exp(v): Rodrigues' formula as cos I + sin [k]x + (1 - cos) k k^T with k = v / |v|; v = 0 gives R0's bits
SAIP_SAMP_HD inline void samp_exp_apply(const double* R0, const double* v, double* out) {
#pragma clang fp contract(off)
	const double ang = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
	if (ang == 0.0) {
		for (int e = 0; e < 9; e++) out[e] = R0[e];
		return;
	}
	const double k[3] = {v[0] / ang, v[1] / ang, v[2] / ang};
	const double sa = sin(ang), ca = cos(ang), c1 = 1.0 - ca;
	double E[9];
	E[0] = (c1 * k[0]) * k[0] + ca;
	E[1] = (c1 * k[0]) * k[1] - sa * k[2];
	E[2] = (c1 * k[0]) * k[2] + sa * k[1];
	E[3] = (c1 * k[1]) * k[0] + sa * k[2];
	E[4] = (c1 * k[1]) * k[1] + ca;
	E[5] = (c1 * k[1]) * k[2] - sa * k[0];
	E[6] = (c1 * k[2]) * k[0] - sa * k[1];
	E[7] = (c1 * k[2]) * k[1] + sa * k[0];
	E[8] = (c1 * k[2]) * k[2] + ca;
	double T[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) T[3 * i + j] = (R0[3 * i] * E[j] + R0[3 * i + 1] * E[3 + j]) + R0[3 * i + 2] * E[6 + j];
	for (int e = 0; e < 9; e++) out[e] = T[e];
}
// w = Log(R0^T R1) as a rotation vector: through the antisymmetric part and atan2
SAIP_SAMP_HD inline void samp_log(const double* R0, const double* R1, double* w) {
#pragma clang fp contract(off)
	double M[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) M[3 * i + j] = (R0[i] * R1[j] + R0[3 + i] * R1[3 + j]) + R0[6 + i] * R1[6 + j];
	const double w0 = 0.5 * (M[7] - M[5]), w1 = 0.5 * (M[2] - M[6]), w2 = 0.5 * (M[3] - M[1]);
	const double sn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
	const double cs = 0.5 * (((M[0] + M[4]) + M[8]) - 1.0);
	if (sn == 0.0) {
		w[0] = w[1] = w[2] = 0.0;
		return;
	}
	const double ang = atan2(sn, cs);
	w[0] = ang * (w0 / sn);
	w[1] = ang * (w1 / sn);
	w[2] = ang * (w2 / sn);
}

// sampler coordinate of row r of the range (not one of the nine rotation rows)
SAIP_SAMP_HD inline int samp_coord(const SamplerEntry& E, int r) { return (E.rot && r >= E.r_rot + 9) ? r - 6 : r; }

// ---- perturb: every keyframe of instance i, which rolls out candidate c (c == i without scenario groups).  Candidates below `exempt`
// get the nominal rows bit for bit, the others nominal + sigma * z per linear row and R_nom Exp(sigma o z) for the rotation, the noise
// counter's instance word being c: a candidate has the same keyframes in every scenario block.  Only column i is written.
SAIP_SAMP_HD inline void samp_perturb_candidate(const SamplerEntry& E, int ld, int i, int c, uint32_t seed_lo, uint32_t seed_hi, uint32_t round) {
#pragma clang fp contract(off)
	for (int k = 0; k < E.K; k++) {
		const double* nom = E.nominal + (size_t)k * E.count;
		double* key = E.key + (size_t)k * E.count * ld + i;
		if (c < E.exempt) {
			for (int r = 0; r < E.count; r++) key[(size_t)r * ld] = nom[r];
			continue;
		}
		double z[SAMP_MAX_ROWS];
		for (int p = 0; 2 * p < E.d; p++) {
			double zz[2];
			samp_normals(seed_lo, seed_hi, round, E.task, c, k, p, zz);
			z[2 * p] = zz[0];
			if (2 * p + 1 < E.d) z[2 * p + 1] = zz[1];
		}
		for (int r = 0; r < E.count; r++) {
			if (E.rot && r >= E.r_rot && r < E.r_rot + 9) continue;
			const int j = samp_coord(E, r);
			key[(size_t)r * ld] = nom[r] + E.sigma[j] * z[j];
		}
		if (E.rot) {
			double v[3], R[9];
			for (int e = 0; e < 3; e++) v[e] = E.sigma[E.r_rot + e] * z[E.r_rot + e];
			samp_exp_apply(nom + E.r_rot, v, R);
			for (int e = 0; e < 9; e++) key[(size_t)(E.r_rot + e) * ld] = R[e];
		}
	}
}

SAIP_SAMP_HD inline void samp_perturb_instance(const SamplerEntry& E, int ld, int i, uint32_t seed_lo, uint32_t seed_hi, uint32_t round) {
	samp_perturb_candidate(E, ld, i, i, seed_lo, seed_hi, round);
}

// ---- cost of instance i: sum over the summary rows with a non-zero weight, then w_path * sum over the samples (oldest first) of
// |p - target|^2, then w_final * |p(last sample) - target|^2; left to right from 0.0, |e|^2 as ((e0 e0 + e1 e1) + e2 e2)
SAIP_SAMP_HD inline double samp_cost_instance(const SamplerCostParams& P, int i) {
#pragma clang fp contract(off)
	double c = 0.0;
	if (P.summary)
		for (int r = 0; r < SAMP_SUMMARY_ROWS; r++)
			if (P.w[r] != 0.0) c = c + P.w[r] * P.summary[(size_t)r * P.ld + i];
	if (P.has_target) {
		double path = 0.0, last = 0.0;
		for (int s = 0; s < P.n_samples; s++) {
			const int slot = (P.first_slot + s) % P.capacity;
			const double* p = P.log + ((size_t)slot * P.rows + P.pose_row0) * P.ld + i;
			const double e0 = p[0] - P.target[0], e1 = p[(size_t)P.ld] - P.target[1], e2 = p[(size_t)2 * P.ld] - P.target[2];
			last = (e0 * e0 + e1 * e1) + e2 * e2;
			path = path + last;
		}
		c = c + P.w_path * path;
		c = c + P.w_final * last;
	}
	return c;
}

// ---- group cost of candidate c over its M scenarios v_s = cost[s C + c].  One v_s that is not finite makes it +inf (the candidate is
// invalid whatever the others say).  MEAN: (((0.0 + v_0) + v_1) + ... + v_{M-1}) / M.  MAX: the largest v_s.  CVAR: the `tail` largest
// v_s added in descending order from 0.0, divided by tail; tail = 1 is MAX bit for bit ((0.0 + v) / 1.0 == v; a largest value of -0.0
// comes out as +0.0 under both, see below).  CVAR selects by rank and re-reads the costs instead of sorting a per-lane array: the t-th
// largest is the value with fewer than t + 1 values ahead of it in the order (larger value, then lower scenario), found by counting --
// O(tail M^2) loads of M L2-resident values, no run-time-indexed registers.
SAIP_SAMP_HD inline bool samp_finite(double c) { return fabs(c) <= 1.7976931348623157e308; }  // false for NaN and the infinities
SAIP_SAMP_HD inline double samp_group_cost(const double* cost, int C, int M, int c, int risk, int tail) {
#pragma clang fp contract(off)
	const double* v = cost + c;
	double sum = 0.0, mx = 0.0;
	for (int s = 0; s < M; s++) {
		const double x = v[(size_t)s * C];
		if (!samp_finite(x)) return INFINITY;
		sum = sum + x;
		mx = (s == 0 || x > mx) ? x : mx;
	}
	if (risk == SAMP_RISK_MEAN) return sum / (double)M;
	if (risk == SAMP_RISK_MAX) return 0.0 + mx;  // -0.0 becomes +0.0, as CVAR's first addition makes it
	double top = 0.0;
	for (int t = 0; t < tail; t++)
		for (int s = 0; s < M; s++) {  // the scenario of rank t: exactly t others are ahead of it
			const double x = v[(size_t)s * C];
			int ahead = 0;
			for (int o = 0; o < M; o++) {
				const double y = v[(size_t)o * C];
				ahead += (y > x || (y == x && o < s)) ? 1 : 0;
			}
			if (ahead == t) {
				top = top + x;
				break;
			}
		}
	return top / (double)tail;
}
// the best map of a grouped update: every scenario block takes its own copy of the best candidate
SAIP_SAMP_HD inline int samp_group_map(int i, int C, int best) { return best < 0 ? -1 : (i / C) * C + best; }

// ---- update.  Reduction shape, the same for every sum and for the minimum: lane l of SAMP_LANES takes instances l, l + 256, ... in
// that order; inside each group of 64 lanes the lane values are folded as v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1; the four
// group results are combined as (g0 + g1) + (g2 + g3).
// the smaller of two (cost, index) candidates, the lower index on a tie; index -1: no candidate
SAIP_SAMP_HD inline void samp_min_combine(double& m, int& im, double o, int io) {
	if (io >= 0 && (im < 0 || o < m || (o == m && io < im))) {
		m = o;
		im = io;
	}
}
SAIP_SAMP_HD inline void samp_lane_minimum(const double* cost, int B, int lane, double& m, int& im, int& n_valid) {
	m = 0.0;
	im = -1;
	n_valid = 0;
	for (int i = lane; i < B; i += SAMP_LANES) {
		const double c = cost[i];
		if (!samp_finite(c)) continue;
		n_valid++;
		samp_min_combine(m, im, c, i);
	}
}
SAIP_SAMP_HD inline double samp_weight(double cost, double beta, double temperature) {
#pragma clang fp contract(off)
	return samp_finite(cost) ? exp(-((cost - beta) / temperature)) : 0.0;
}
// the weights of a lane's instances (written to w[]), their sum and the sum of their squares
SAIP_SAMP_HD inline void samp_lane_weights(const double* cost, int B, int lane, double beta, double temperature, double* w, double& sw, double& sw2) {
#pragma clang fp contract(off)
	sw = 0.0;
	sw2 = 0.0;
	for (int i = lane; i < B; i += SAMP_LANES) {
		const double x = samp_weight(cost[i], beta, temperature);
		w[i] = x;
		sw = sw + x;
		sw2 = sw2 + x * x;
	}
}
// a lane's share of the weighted sums of keyframe k: acc[j] = sum of w_i * (row of coordinate j), the three tangent coordinates from
// w_i * Log(R_nom^T R_i)
SAIP_SAMP_HD inline void samp_lane_accumulate(const SamplerEntry& E, int k, int ld, int B, const double* w, int lane, double* acc) {
#pragma clang fp contract(off)
	for (int j = 0; j < E.d; j++) acc[j] = 0.0;
	const double* nom = E.nominal + (size_t)k * E.count;
	for (int i = lane; i < B; i += SAMP_LANES) {
		const double wi = w[i];
		const double* key = E.key + (size_t)k * E.count * ld + i;
		for (int r = 0; r < E.count; r++) {
			if (E.rot && r >= E.r_rot && r < E.r_rot + 9) continue;
			const int j = samp_coord(E, r);
			acc[j] = acc[j] + wi * key[(size_t)r * ld];
		}
		if (E.rot) {
			double R[9], l[3];
			for (int e = 0; e < 9; e++) R[e] = key[(size_t)(E.r_rot + e) * ld];
			samp_log(nom + E.r_rot, R, l);
			for (int e = 0; e < 3; e++) acc[E.r_rot + e] = acc[E.r_rot + e] + wi * l[e];
		}
	}
}
// what one lane does with the reduced sums tot[d] of keyframe k: the new nominal rows.  When all the weight is on one instance in
// double precision (sum w == 1 and sum w^2 == 1: the minimum's weight is exp(0) = 1 and nothing else adds to it), the rotation rows
// are instance `best`'s own rows -- Exp(Log(.)) of a single rotation would add nothing but its roundings.
SAIP_SAMP_HD inline void samp_finish_keyframe(const SamplerEntry& E, int k, int ld, const double* tot, double sum_w, double sum_w2, int best) {
#pragma clang fp contract(off)
	double* nom = E.nominal + (size_t)k * E.count;
	for (int r = 0; r < E.count; r++) {
		if (E.rot && r >= E.r_rot && r < E.r_rot + 9) continue;
		nom[r] = tot[samp_coord(E, r)] / sum_w;
	}
	if (E.rot) {
		double R[9];
		if (sum_w == 1.0 && sum_w2 == 1.0) {
			const double* key = E.key + ((size_t)k * E.count + E.r_rot) * ld + best;
			for (int e = 0; e < 9; e++) R[e] = key[(size_t)e * ld];
		} else {
			const double delta[3] = {tot[E.r_rot] / sum_w, tot[E.r_rot + 1] / sum_w, tot[E.r_rot + 2] / sum_w};
			samp_exp_apply(nom + E.r_rot, delta, R);
		}
		for (int e = 0; e < 9; e++) nom[E.r_rot + e] = R[e];
	}
}
// nominal[k] <- nominal[min(k + n, K - 1)] for column c of the plan (ascending k: what is read has not been written yet)
SAIP_SAMP_HD inline void samp_shift_column(double* nominal, int K, int count, int n, int c) {
	for (int k = 0; k < K; k++) nominal[(size_t)k * count + c] = nominal[(size_t)(k + n < K ? k + n : K - 1) * count + c];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- scenario groups on the host: the grouped perturb and the group-cost kernel, instance by instance and candidate by candidate
inline void samp_host_perturb_grouped(const SamplerEntry& E, int ld, int B, int C, uint32_t seed_lo, uint32_t seed_hi, uint32_t round) {
	for (int i = 0; i < B; i++) samp_perturb_candidate(E, ld, i, i % C, seed_lo, seed_hi, round);
}
inline void samp_host_group_cost(const double* cost, int C, int M, int risk, int tail, double* group) {
	for (int c = 0; c < C; c++) group[c] = samp_group_cost(cost, C, M, c, risk, tail);
}
inline void samp_host_group_map(int B, int C, int best, int* best_map) {
	for (int i = 0; i < B; i++) best_map[i] = samp_group_map(i, C, best);
}
// ---- the reduction shape on the host: `v` holds the SAMP_LANES lane values (overwritten)
inline double samp_tree_sum(double* v) {
	for (int g = 0; g < SAMP_LANES; g += SAMP_WAVE)
		for (int off = SAMP_WAVE / 2; off >= 1; off /= 2)
			for (int l = 0; l < off; l++) v[g + l] = v[g + l] + v[g + l + off];
	return (v[0] + v[SAMP_WAVE]) + (v[2 * SAMP_WAVE] + v[3 * SAMP_WAVE]);
}
// the two update kernels, lane by lane: weights, result and best map, then the nominal of every keyframe of every entry
inline void samp_host_weights(const double* cost, int B, double temperature, double* w, SamplerResult* res, int* best_map) {
	double m = 0.0, v[SAMP_LANES], v2[SAMP_LANES];
	int im = -1, n_valid = 0;
	for (int l = 0; l < SAMP_LANES; l++) {
		double ml;
		int il, nl;
		samp_lane_minimum(cost, B, l, ml, il, nl);
		samp_min_combine(m, im, ml, il);
		n_valid += nl;
	}
	for (int l = 0; l < SAMP_LANES; l++) samp_lane_weights(cost, B, l, m, temperature, w, v[l], v2[l]);
	const double sw = samp_tree_sum(v), sw2 = samp_tree_sum(v2);
	res->best = im;
	res->n_valid = n_valid;
	res->min_cost = n_valid ? m : 0.0;
	res->sum_w = n_valid ? sw : 0.0;
	res->ess = n_valid ? (sw * sw) / sw2 : 0.0;
	for (int i = 0; i < B; i++) best_map[i] = im;
}
inline void samp_host_update(const SamplerEntry& E, int ld, int B, const double* w, const SamplerResult& res) {
	if (res.n_valid == 0) return;
	double v[SAMP_LANES], v2[SAMP_LANES];
	for (int l = 0; l < SAMP_LANES; l++) {
		v[l] = v2[l] = 0.0;
		for (int i = l; i < B; i += SAMP_LANES) {
			v[l] = v[l] + w[i];
			v2[l] = v2[l] + w[i] * w[i];
		}
	}
	const double sw = samp_tree_sum(v), sw2 = samp_tree_sum(v2);
	for (int k = 0; k < E.K; k++) {
		static thread_local double acc[SAMP_LANES][SAMP_MAX_ROWS];
		double tot[SAMP_MAX_ROWS];
		for (int l = 0; l < SAMP_LANES; l++) samp_lane_accumulate(E, k, ld, B, w, l, acc[l]);
		for (int j = 0; j < E.d; j++) {
			for (int l = 0; l < SAMP_LANES; l++) v[l] = acc[l][j];
			tot[j] = samp_tree_sum(v);
		}
		samp_finish_keyframe(E, k, ld, tot, sw, sw2, res.best);
	}
}
#endif

}  // namespace saip
