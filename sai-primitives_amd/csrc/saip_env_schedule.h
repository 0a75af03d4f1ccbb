// Environment schedules of the resident simulator (saip_env_schedule.hip): what the robot touches or avoids, as a function of the rollout
// period.  The per-item arithmetic, shared by the kernel and by host-compiled checks (plain C++ when no HIP compiler is reading it, like
// saip_contact.h and saip_clearance.h).
//
// A schedule belongs to one target table of a batch -- the clearance monitor's obstacles, the single-point contact planes, or the planes of
// one contact patch -- and covers the items [first, first + n_items) of it.  Its keyframes are [K][n_items][W] (batch-uniform table) or
// [K][n_items][W][ld] (per-instance table): W = 8 for an obstacle (the words of saip_clearance.h), W = ENV_PLANE_WORDS = 12 for a plane: the
// eight plane words of saip_contact.h, a surface velocity u[3] in the base frame, and one reserved word that is 0.
//
// Timing is the host's (env_timing): for the period index x the schedule sees, i = x / stride and s = (x % stride) / stride, the last
// keyframe held.  Contact targets see the rollout period c (the planes are held through the period's substeps); the clearance target
// sees c + 1, the time of the state the monitor looks at behind the period's integration.
//
// HOLD writes keyframe i.  LINEAR between keyframes a = i and b = i + 1 writes a + s (b - a) per word (env_lerp: difference, product and sum
// each rounded on its own); at s == 0 the row is a exactly; an obstacle's kind is a's; a unit normal (half-space a[3], plane n[3]) is
// interpolated the same way and divided by sqrt(cl_dot(m, m)).  For a plane the kernel also writes the velocity row { v_p[3], w_n }:
//   v_p = u + w_n n     w_n = (o_b - o_a) / (stride T) in LINEAR between two keyframes, 0 in HOLD and past the last keyframe
// with u interpolated like any word and n the normal just written.  The rotation of a normal contributes no velocity.
// tests/env_schedule_ref.py restates all of it in NumPy bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "saip_clearance.h"

#if defined(__HIPCC__)
#define SAIP_ENV_HD __host__ __device__
#else
#define SAIP_ENV_HD
#endif

namespace saip {

enum { ENV_MAX_SCHEDULES = 4, ENV_OBSTACLE_WORDS = 8, ENV_PLANE_WORDS = 12, ENV_TABLE_WORDS = 8, ENV_VELOCITY_WORDS = 4 };
enum { ENV_TARGET_OBSTACLES = 0, ENV_TARGET_PLANES = 1, ENV_TARGET_PATCH = 2 };
enum { ENV_HOLD = 0, ENV_LINEAR = 1 };

// a + s (b - a), nothing contracted (as sched_lerp of saip_goal_schedule.hip)
SAIP_ENV_HD inline double env_lerp(double a, double b, double s) {
#pragma clang fp contract(off)
	return a + s * (b - a);
}

// the period index a schedule sees in rollout period c: the planes of period c are held through its substeps; the monitor looks at the state
// behind the period's integration, at (c + 1) T
inline long long env_period_index(long long c, int planes) { return planes ? c : c + 1; }
// the keyframe index, the fraction and whether the schedule is between two keyframes, for the period index x >= 0 it sees
inline void env_timing(long long x, int K, int stride, int mode, int* i, double* s, int* moving) {
	const bool past = x >= (long long)(K - 1) * stride;  // the last keyframe is held
	*i = past ? K - 1 : (int)(x / stride);
	*s = past ? 0.0 : (double)(x % stride) / (double)stride;
	*moving = mode == ENV_LINEAR && !past;
}

// One item.  ka, kb: word 0 of the item in keyframes i and i + 1 (kb = ka unless `moving`), word w at [w * ks]; row: word 0 of the item in
// the target table, vel: word 0 of its velocity row (planes only), both with words ts apart.  span = stride T.
template <bool PLANES>
SAIP_ENV_HD inline void env_write_item(const double* ka, const double* kb, long long ks, int moving, double s, double span, double* row, double* vel,
										long long ts) {
#pragma clang fp contract(off)
	constexpr int W = PLANES ? ENV_PLANE_WORDS : ENV_OBSTACLE_WORDS, N0 = PLANES ? 0 : 1;  // N0: the first word of a normal
	const bool lerp = moving && s != 0.0;
	double w[W];
	for (int k = 0; k < W; k++) w[k] = lerp ? env_lerp(ka[k * ks], kb[k * ks], s) : ka[k * ks];
	if constexpr (!PLANES) w[0] = ka[0];
	if (lerp && (PLANES || ka[0] == (double)CLEARANCE_HALF_SPACE)) {
		const double nn = sqrt(cl_dot(&w[N0], &w[N0]));
		for (int e = 0; e < 3; e++) w[N0 + e] = w[N0 + e] / nn;
	}
	for (int k = 0; k < ENV_TABLE_WORDS; k++) row[k * ts] = w[k];
	if constexpr (PLANES) {
		const double wn = moving ? (kb[3 * ks] - ka[3 * ks]) / span : 0.0;
		for (int e = 0; e < 3; e++) vel[e * ts] = w[8 + e] + wn * w[e];
		vel[3 * ts] = wn;
	}
}

// one schedule of a launch
struct EnvEntry {
	double* table;          // the target: [items][8] or [items][8][ld]
	double* vel;            // planes: [items][4] or [items][4][ld]
	const double* key;      // [K][n_items][W] or [K][n_items][W][ld]
	int planes, per_instance, first, n_items;
	int i, moving;          // env_timing
	double s, span;
};
// one launch of saip_env_schedule_apply.  Passed to the kernel by value.
struct EnvScheduleParams {
	int B, ld, n, pad_;
	EnvEntry e[ENV_MAX_SCHEDULES];
};

// item `item` of entry E for one column: stride ld and col = the instance for a per-instance table, stride 1 and col 0 for a batch-uniform one
SAIP_ENV_HD inline void env_entry_item(const EnvEntry& E, int item, long long stride, long long col) {
	const long long W = E.planes ? ENV_PLANE_WORDS : ENV_OBSTACLE_WORDS;
	const double* ka = E.key + (((long long)E.i * E.n_items + item) * W) * stride + col;
	const double* kb = E.moving ? ka + (long long)E.n_items * W * stride : ka;
	double* row = E.table + (long long)(E.first + item) * ENV_TABLE_WORDS * stride + col;
	if (E.planes) env_write_item<true>(ka, kb, stride, E.moving, E.s, E.span, row, E.vel + (long long)(E.first + item) * ENV_VELOCITY_WORDS * stride + col, stride);
	else env_write_item<false>(ka, kb, stride, E.moving, E.s, E.span, row, nullptr, stride);
}

// (host only)  What an attach asks of the keyframes [K][n_items][W][cols] beyond the table's own rules (plane keyframes arrive normalised): every word
// finite, the reserved plane word 0, a half-space normal within 1e-6 of unit length, one obstacle kind per item, and in LINEAR no two
// consecutive normals with n_a . n_b < 0 (then |m|^2 >= 1/2 and the division above is safe).  false: `msg` says what is wrong.
inline bool env_check_keyframes(const double* key, int planes, int K, int n_items, size_t cols, int mode, char* msg, size_t len) {
	const size_t W = planes ? ENV_PLANE_WORDS : ENV_OBSTACLE_WORDS, N0 = planes ? 0 : 1;
	const char* what = planes ? "plane" : "obstacle";
	for (int it = 0; it < n_items; it++)
		for (size_t c = 0; c < cols; c++) {
			char where[48] = "";
			if (cols > 1) snprintf(where, sizeof(where), " of instance %zu", c);
			for (int k = 0; k < K; k++) {
				const double* w = key + (((size_t)k * n_items + it) * W) * cols + c;
				for (size_t j = 0; j < W; j++)
					if (!cl_finite(w[j * cols])) return snprintf(msg, len, "keyframe %d, %s %d%s: word %zu is not finite", k, what, it, where, j), false;
				if (planes && w[11 * cols] != 0.0) return snprintf(msg, len, "keyframe %d, plane %d%s: the reserved word 11 is not 0", k, it, where), false;
				if (!planes) {
					const double kind = w[0];
					if (kind != (double)CLEARANCE_CAPSULE && kind != (double)CLEARANCE_HALF_SPACE)
						return snprintf(msg, len, "keyframe %d, obstacle %d%s: unknown kind %g (0 capsule, 1 half-space)", k, it, where, kind), false;
					if (kind != key[((size_t)it * W) * cols + c])
						return snprintf(msg, len, "keyframe %d, obstacle %d%s: kind %g differs from keyframe 0", k, it, where, kind), false;
					if (kind == (double)CLEARANCE_CAPSULE && w[7 * cols] < 0)
						return snprintf(msg, len, "keyframe %d, obstacle %d%s: radius %g below 0", k, it, where, w[7 * cols]), false;
					if (kind == (double)CLEARANCE_HALF_SPACE) {
						const double nn = sqrt(w[cols] * w[cols] + w[2 * cols] * w[2 * cols] + w[3 * cols] * w[3 * cols]);
						if (!(fabs(nn - 1.0) <= 1e-6))
							return snprintf(msg, len, "keyframe %d, obstacle %d%s: the half-space normal has length %.9g, not 1", k, it, where, nn), false;
					}
				}
				if (mode == ENV_LINEAR && k > 0 && (planes || w[0] == (double)CLEARANCE_HALF_SPACE)) {
					const double* a = w - (size_t)n_items * W * cols;
					const double na[3] = {a[N0 * cols], a[(N0 + 1) * cols], a[(N0 + 2) * cols]}, nb[3] = {w[N0 * cols], w[(N0 + 1) * cols], w[(N0 + 2) * cols]};
					if (cl_dot(na, nb) < 0.0)
						return snprintf(msg, len, "keyframes %d and %d, %s %d%s: the normals are more than a right angle apart (n_a . n_b < 0)", k - 1, k, what, it, where), false;
				}
			}
		}
	return true;
}

}  // namespace saip
