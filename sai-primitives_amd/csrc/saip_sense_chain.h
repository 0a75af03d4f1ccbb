// The sensing chain of the resident simulator (saip_sense_chain.hip): the optional second stage of the sensing model (saip_sense.h).  Per
// joint it turns the measured sample (q_m, dq_m) into what the controller reads, through a delay line of up to SENSE_CHAIN_MAX_DEPTH
// samples, an optional finite-difference velocity and a first-order low-pass.  The per-element arithmetic, shared by the kernels and by
// host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_sense.h).
//
// A joint is SENSE_CHAIN_WORDS words: delay, vel_mode, a_q, a_dq.  One sample of one (joint, instance):
//   d = (int)delay                                     integer-valued, 0..depth (validated at upload; clamped here)
//   if (!primed) { every tap = (q_m, dq_m); q_prev = q_m; y_q = q_m; y_dq = dq_m; primed = 1 }
//   x = d ? tap_q[d-1] : q_m;  v = d ? tap_dq[d-1] : dq_m     the sample taken d samples ago
//   taps 1..d-1 take their predecessor, tap 0 the new sample
//   if (vel_mode == 1) { v = (x - q_prev) / sample_time;  q_prev = x }
//   y_q  = a_q  > 0 ? y_q  + a_q  (x - y_q)  : x
//   y_dq = a_dq > 0 ? y_dq + a_dq (v - y_dq) : v
// and (y_q, y_dq) is what the controller reads.  The neutral row is all zeros and returns its input bits.  The state is the taps
// ([2 depth] per joint: q then dq), q_prev, y_q, y_dq and the flag `primed`; nothing else, in particular no ring head and no counter: a
// shift register needs nothing outside the instance's column, so the state moves through a snapshot's source index like any other array.
//
// Every product, sum and quotient is rounded on its own (no contraction into FMAs), in the order written, and there is no transcendental
// function, so a NumPy restatement (tests/sensing_chain_ref.py) reproduces the arithmetic bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_sense.h"

namespace saip {

enum { SENSE_CHAIN_WORDS = 4, SENSE_CHAIN_MAX_DEPTH = 8, SENSE_CHAIN_FILT_ROWS = 3 };
enum { SENSE_CHAIN_DELAY = 0, SENSE_CHAIN_VEL_MODE, SENSE_CHAIN_A_Q, SENSE_CHAIN_A_DQ };
enum { SENSE_CHAIN_Q_PREV = 0, SENSE_CHAIN_Y_Q, SENSE_CHAIN_Y_DQ };
// the table id inside the random-number counter: 0..7 are the plant's, the inertia table's and the sensing model's.  pl_draw puts the id
// into a counter word of its own (32 bits), so 8 fits
enum { SENSE_TABLE_CHAIN = 8 };

// One sample of one (joint, instance).  Word k of the joint is w[k * stride] (as se_joint).  Tap k of q is tap_q[k * ss], of dq
// tap_dq[k * ss], row r of the filter state filt[r * ss]: ss is the distance between two rows of one instance's column (ld on the device).
// Only taps 0..d-1 are read or shifted; priming fills all `depth` of them.
SAIP_SE_HD inline void sc_step(const double* w, long long stride, int depth, double sample_time, double* tap_q, double* tap_dq, double* filt, int* primed, long long ss,
								double q_m, double dq_m, double* q_meas, double* dq_meas) {
#pragma clang fp contract(off)
	const double dd = w[SENSE_CHAIN_DELAY * stride], a_q = w[SENSE_CHAIN_A_Q * stride], a_dq = w[SENSE_CHAIN_A_DQ * stride];
	const int d = dd >= 1.0 ? (dd < (double)depth ? (int)dd : depth) : 0;  // a table written through the device pointer cannot index past the taps
	double q_prev = filt[SENSE_CHAIN_Q_PREV * ss], y_q = filt[SENSE_CHAIN_Y_Q * ss], y_dq = filt[SENSE_CHAIN_Y_DQ * ss];
	const bool fresh = !*primed;
	// Taps 0..d-1 are all loaded before any is stored: a loop that loads tap k-1 and stores tap k in turn makes every load wait for the store
	// before it (the compiler cannot tell the rows apart), up to `depth` memory round trips in a row.  The copies are indexed by unrolled
	// constants only, so they are registers, not an array in memory.
	double tq[SENSE_CHAIN_MAX_DEPTH], tdq[SENSE_CHAIN_MAX_DEPTH];
#pragma unroll
	for (int k = 0; k < SENSE_CHAIN_MAX_DEPTH; k++) {
		tq[k] = q_m;
		tdq[k] = dq_m;
		if (k < d) {
			const double a = tap_q[k * ss], b = tap_dq[k * ss];
			if (!fresh) {
				tq[k] = a;
				tdq[k] = b;
			}
		}
	}
	if (fresh) {
		for (int k = 0; k < depth; k++) {
			tap_q[k * ss] = q_m;
			tap_dq[k * ss] = dq_m;
		}
		q_prev = q_m;
		y_q = q_m;
		y_dq = dq_m;
		*primed = 1;
	}
	double x = q_m, v = dq_m;
#pragma unroll
	for (int k = 0; k < SENSE_CHAIN_MAX_DEPTH; k++)
		if (k == d - 1) {
			x = tq[k];
			v = tdq[k];
		}
#pragma unroll
	for (int k = 1; k < SENSE_CHAIN_MAX_DEPTH; k++)
		if (k < d) {
			tap_q[k * ss] = tq[k - 1];
			tap_dq[k * ss] = tdq[k - 1];
		}
	if (d) {
		tap_q[0] = q_m;
		tap_dq[0] = dq_m;
	}
	if (w[SENSE_CHAIN_VEL_MODE * stride] == 1.0) {
		v = (x - q_prev) / sample_time;
		q_prev = x;
	}
	y_q = a_q > 0.0 ? y_q + a_q * (x - y_q) : x;
	y_dq = a_dq > 0.0 ? y_dq + a_dq * (v - y_dq) : v;
	filt[SENSE_CHAIN_Q_PREV * ss] = q_prev;
	filt[SENSE_CHAIN_Y_Q * ss] = y_q;
	filt[SENSE_CHAIN_Y_DQ * ss] = y_dq;
	*q_meas = y_q;
	*dq_meas = y_dq;
}

// The random draw of word `word` (joint j word k is 4 j + k) of instance i: pl_draw of saip_plant.h under the chain's table id; delay and
// vel_mode are rounded to the nearest integer, floor(x + 0.5), and clamped to 0..depth and 0..1.
SAIP_SE_HD inline double sc_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int i, int word, double lo, double hi, int depth) {
#pragma clang fp contract(off)
	double v = pl_draw(seed_lo, seed_hi, round, SENSE_TABLE_CHAIN, i, word, lo, hi, false);
	const int k = word % SENSE_CHAIN_WORDS;
	if (k == SENSE_CHAIN_DELAY || k == SENSE_CHAIN_VEL_MODE) {
		const double top = k == SENSE_CHAIN_DELAY ? (double)depth : 1.0;
		v = floor(v + 0.5);
		v = v < 0.0 ? 0.0 : (v > top ? top : v);
	}
	return v;
}

// one launch of saip_sense_chain_apply: the sensing model's launch and the chain behind its joint rows.  Passed to the kernel by value.
struct SenseChainParams {
	SenseParams S;
	int per_instance, depth;
	double sample_time;
	const double* table;         // [n][4] or [n][4][ld]
	double* taps;                // [n][2][depth][ld]: joint j, q (0) or dq (1), tap k is row (2 j + c) depth + k; null at depth 0
	double* filt;                // [n][3][ld]: q_prev, y_q, y_dq
	int* primed;                 // [n][ld]
};
// one launch of saip_sense_chain_randomize
struct SenseChainRandomParams {
	int B, ld, n, depth;
	uint32_t seed_lo, seed_hi, round, pad_;
	double* table;               // [n][4][ld]
	const double* lo;            // [n][4], device
	const double* hi;
};

}  // namespace saip
