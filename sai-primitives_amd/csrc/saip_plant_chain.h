// The actuation chain of the resident simulator (saip_plant.hip): the optional second stage of the plant model (saip_plant.h), the
// command-side twin of the sensing chain (saip_sense_chain.h).  Per joint it stands between the commanded torque and pl_joint's input t:
// a delay line of up to PLANT_CHAIN_MAX_DEPTH control periods, then a slew-rate limit, then a first-order lag.  The per-element
// arithmetic, shared by the kernels and by host-compiled checks (plain C++ when no HIP compiler is reading it, like saip_plant.h).
//
// A joint is PLANT_CHAIN_WORDS words: delay, rate_max, tau_lag.  One call per (joint, instance) per integration substep of length dt;
// advance is 1 in the first substep of a period and 0 otherwise:
//   x0 = (t == t) ? t : 0                              a NaN command is no torque, as pl_joint reads it
//   d  = (int)delay                                    integer-valued, 0..depth (validated at upload; clamped here)
//   if (advance) {
//       if (!primed) { every tap = x0; x_held = y_rate = y_lag = x0; primed = 1 }
//       x_held = d ? tap[d-1] : x0                     the command issued d periods ago
//       taps 1..d-1 take their predecessor, tap 0 the new command
//   }
//   step   = rate_max dt
//   y_rate = rate_max < +inf ? y_rate + min(max(x_held - y_rate, -step), step) : x_held
//   y_lag  = tau_lag > 0 ? y_lag + (dt / (tau_lag + dt)) (y_rate - y_lag) : y_rate        backward Euler of tau_lag y' + y = u
// and y_lag is what pl_joint gets.  The neutral row is 0, +inf, 0 and returns the sanitised command's bits.  The delay counts control
// periods; the rate limit and the lag are actuator dynamics and run every substep with that substep's dt.  The state is the taps
// ([depth] per joint), x_held, y_rate, y_lag and the flag `primed`; nothing else, in particular no ring head and no counter: a shift
// register needs nothing outside the instance's column, so the state moves through a snapshot's source index like any other array.
//
// Every product, sum and quotient is rounded on its own (no contraction into FMAs), in the order written, and there is no transcendental
// function, so a NumPy restatement (tests/plant_chain_ref.py) reproduces the arithmetic bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "saip_plant.h"

namespace saip {

enum { PLANT_CHAIN_WORDS = 3, PLANT_CHAIN_MAX_DEPTH = 8, PLANT_CHAIN_FILT_ROWS = 3 };
enum { PLANT_CHAIN_DELAY = 0, PLANT_CHAIN_RATE_MAX, PLANT_CHAIN_TAU_LAG };
enum { PLANT_CHAIN_X_HELD = 0, PLANT_CHAIN_Y_RATE, PLANT_CHAIN_Y_LAG };
// the table id inside the random-number counter: 0..8 are the plant's, the inertia table's, the sensing model's and the sensing chain's
enum { PLANT_TABLE_CHAIN = 9 };

// One substep of one (joint, instance) in two halves, so that a caller that walks the joints of one instance (saip_plant_apply) can have
// the loads of the next joint in flight while it finishes this one: pc_load reads the words and the state, pc_finish does the arithmetic
// and the stores and returns what pl_joint gets in place of t; pc_step is one behind the other.  Word k of the joint is w[k * stride] (as
// pl_joint).  Tap k is tap[k * ss], row r of the filter state filt[r * ss]: ss is the distance between two rows of one instance's column
// (ld on the device).  Taps are touched only when advance is set: all `depth` are loaded, taps 0..d-1 are used and shifted; priming
// fills all `depth` of them.  tap may be null at depth 0.
struct PlantChainLoaded {
	double delay, rate_max, tau_lag;
	double x_held, y_rate, y_lag;
	double tp[PLANT_CHAIN_MAX_DEPTH];
	int primed;
};
SAIP_PL_HD inline void pc_load(const double* w, long long stride, int depth, const double* tap, const double* filt, const int* primed, long long ss, bool advance,
								PlantChainLoaded* L) {
	L->delay = w[PLANT_CHAIN_DELAY * stride];
	L->rate_max = w[PLANT_CHAIN_RATE_MAX * stride];
	L->tau_lag = w[PLANT_CHAIN_TAU_LAG * stride];
	L->x_held = filt[PLANT_CHAIN_X_HELD * ss];
	L->y_rate = filt[PLANT_CHAIN_Y_RATE * ss];
	L->y_lag = filt[PLANT_CHAIN_Y_LAG * ss];
	L->primed = 1;
	// The taps are all loaded before any is stored, into copies indexed by unrolled constants only (registers), as sc_step does.  All
	// `depth` of them, not only the d the row uses: depth is the same for every lane and known before the delay word has arrived, so the
	// loads go out together with the words' and the filter state's, not one memory round trip behind them; taps d.. are not used.
#pragma unroll
	for (int k = 0; k < PLANT_CHAIN_MAX_DEPTH; k++) L->tp[k] = 0.0;
	if (advance) {
		L->primed = *primed;
#pragma unroll
		for (int k = 0; k < PLANT_CHAIN_MAX_DEPTH; k++)
			if (k < depth) L->tp[k] = tap[k * ss];
	}
}
SAIP_PL_HD inline double pc_finish(const PlantChainLoaded& L, int depth, double* tap, double* filt, int* primed, long long ss, double t, double dt, bool advance) {
#pragma clang fp contract(off)
	const double dd = L.delay, rate_max = L.rate_max, tau_lag = L.tau_lag;
	const double x0 = t == t ? t : 0.0;
	const int d = dd >= 1.0 ? (dd < (double)depth ? (int)dd : depth) : 0;  // a table written through the device pointer cannot index past the taps
	double x_held = L.x_held, y_rate = L.y_rate, y_lag = L.y_lag;
	if (advance) {
		const bool fresh = !L.primed;
		if (fresh) {
			for (int k = 0; k < depth; k++) tap[k * ss] = x0;
			y_rate = x0;
			y_lag = x0;
			*primed = 1;
		}
		x_held = x0;
#pragma unroll
		for (int k = 0; k < PLANT_CHAIN_MAX_DEPTH; k++)
			if (k == d - 1) x_held = fresh ? x0 : L.tp[k];
#pragma unroll
		for (int k = 1; k < PLANT_CHAIN_MAX_DEPTH; k++)
			if (k < d) tap[k * ss] = fresh ? x0 : L.tp[k - 1];
		if (d) tap[0] = x0;
		filt[PLANT_CHAIN_X_HELD * ss] = x_held;
	}
	const double step = rate_max * dt;
	y_rate = rate_max < (double)INFINITY ? y_rate + pl_min(pl_max(x_held - y_rate, -step), step) : x_held;
	y_lag = tau_lag > 0.0 ? y_lag + (dt / (tau_lag + dt)) * (y_rate - y_lag) : y_rate;
	filt[PLANT_CHAIN_Y_RATE * ss] = y_rate;
	filt[PLANT_CHAIN_Y_LAG * ss] = y_lag;
	return y_lag;
}
SAIP_PL_HD inline double pc_step(const double* w, long long stride, int depth, double* tap, double* filt, int* primed, long long ss, double t, double dt, bool advance) {
	PlantChainLoaded L;
	pc_load(w, stride, depth, tap, filt, primed, ss, advance, &L);
	return pc_finish(L, depth, tap, filt, primed, ss, t, dt, advance);
}

// The random draw of word `word` (joint j word k is 3 j + k) of instance i: pl_draw under the chain's table id; delay is rounded to the
// nearest integer, floor(x + 0.5), and clamped to 0..depth.  lo == hi gives lo exactly, so a rate_max of +inf stays +inf.
SAIP_PL_HD inline double pc_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int i, int word, double lo, double hi, int depth) {
#pragma clang fp contract(off)
	double v = pl_draw(seed_lo, seed_hi, round, PLANT_TABLE_CHAIN, i, word, lo, hi, false);
	if (word % PLANT_CHAIN_WORDS == PLANT_CHAIN_DELAY) {
		const double top = (double)depth;
		v = floor(v + 0.5);
		v = v < 0.0 ? 0.0 : (v > top ? top : v);
	}
	return v;
}

// one launch of saip_plant_apply<*, true>: the plant's launch and the chain in front of its joint rows.  Passed to the kernel by value.
struct PlantChainParams {
	PlantParams P;
	int per_instance, depth, advance, pad_;
	const double* table;         // [n][3] or [n][3][ld]
	double* taps;                // [n][depth][ld]: tap k of joint j is row j depth + k; null at depth 0
	double* filt;                // [n][3][ld]: x_held, y_rate, y_lag
	int* primed;                 // [n][ld]
};
// one launch of saip_plant_chain_randomize
struct PlantChainRandomParams {
	int B, ld, n, depth;
	uint32_t seed_lo, seed_hi, round, pad_;
	double* table;               // [n][3][ld]
	const double* lo;            // [n][3], device
	const double* hi;
};

}  // namespace saip
