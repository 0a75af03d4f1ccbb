// Host-only value types of the engine's cycle path (saip_engine.cpp): what plan_cycle decides, and the state of the device-side
// work list that launch_cycle keeps between launches.  No device code.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/saip.h"
#include "saip_device.h"

enum class KernelChoice : int { Auto = 0, Wg = 1, Lane = 2, Oct = 3, Wave = 4 };  // saip_batch_set_kernel's integers

enum class CycleKernel { Wg, Lane, Oct, OctJf, Wave };
enum class Recompute { None, Tail, List };  // of flagged instances: not at all, in the kernel's own slow tail, by the list launch behind it

struct OctFit {  // whether a stack fits the eight-lane kernel, and in which instantiation
	bool ok = false;
	int general_joint = 0, partial_mf = 0, truncate = 0;  // CycleParams::oct_*
};

static const char* const kOctRefusal = "the eight-lanes-per-instance kernel does not cover this robot/task stack";
static const char* const kLaneRefusal = "the lane-per-instance kernel does not cover this robot/task stack";
static const char* const kWaveRefusal = "the wavefront-per-instance kernel covers chains of 9 to 32 dof without a passivity controller";

struct CyclePlan {
	CycleKernel kernel = CycleKernel::Wg;
	Recompute recompute = Recompute::None;
	bool fuse_sim = false;  // the launch integrates the state as well (rollouts)
	OctFit oct;             // set whenever the stack fits the eight-lane kernel; only that kernel reads CycleParams::oct_*
	saip_status refused = SAIP_OK;  // a saip_batch_set_kernel choice that does not cover the stack ...
	const char* why = nullptr;      // ... and the message
};

struct SimRequest {  // rollouts: the integration the cycle launch should do itself if it can
	int substeps;
	double dt, damping, gravity[3];
};

// The device-side work list of the slow path: two { count[32], list[ld] } pairs used alternately (CycleParams::flag_*).  The lane,
// eight-lane or wavefront kernel of a cycle appends to the current pair and zeroes the count of the other one, whose last readers (the
// list launch of the cycle before) have finished by then.
class FlagList {
public:
	int* buf = nullptr;  // [2 * (32 + ld)], zeroed at allocation
	void bind(saip::CycleParams& P, int ld) const {
		int* cur = buf + (size_t)(flag_parity & 1u) * (ld + 32);
		P.flag_count = cur;
		P.flag_list = cur + 32;
		P.flag_count_next = buf + (size_t)((flag_parity + 1u) & 1u) * (ld + 32);
	}
	// before the launch: if the current pair was not zeroed by the cycle before (a cycle without a list, another kernel choice, or a
	// failed launch came in between), zero its count here, or stale entries would be recomputed a second time
	hipError_t zero_current(const saip::CycleParams& P, hipStream_t stream) {  // (P: as bound)
		if (clean[flag_parity & 1u]) return hipSuccess;
		const hipError_t e = hipMemsetAsync(P.flag_count, 0, sizeof(int), stream);
		if (e == hipSuccess) clean[flag_parity & 1u] = true;
		return e;
	}
	// after a launch that succeeded and really took the pair: the kernel appended to the current pair and zeroed the other one
	void handed_over() {
		clean[flag_parity & 1u] = false;
		clean[(flag_parity + 1u) & 1u] = true;
		flag_parity++;
	}

private:
	unsigned flag_parity = 0;      // advanced only by a launch that hands the pair to a kernel
	bool clean[2] = {true, true};  // whether each pair's count is known to be zero
};
