// What the eight-lane cycle kernels (saip_kernel_oct.hip, saip_kernel_octjf.hip) share besides the lane layout of saip_oct_common.h: the general
// kernel's body as their slow tail, and the launch-time question whether a second wavefront per instance group still fits the chip.
#pragma once
#include <hip/hip_runtime.h>

#include "saip_device.h"
// the general kernel's body as these kernels' slow tail: one wavefront plays the 64-thread workgroup, so its synchronisation points are
// wavefront-local (the other wavefront of a two-wavefront workgroup has left by then)
#define SAIP_WG_SYNC()                                          \
	do {                                                        \
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
		__builtin_amdgcn_wave_barrier();                        \
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
	} while (0)
#include "saip_wg_cycle.h"

namespace saip {

// Slow tail (round 4): the instances of this wavefront that ended flagged -- outside SingularityHandler's non-singular branch with the blended
// strategies on (SingularityHandler.cpp:100-121, 146-158, 310-367), a reduced task with fewer than two directions left, an ambiguous rank
// gap -- are recomputed here, one after the other, by the general kernel's body (saip_wg_cycle.h: Jacobi eigen-pairs of the Gram matrix,
// U_ns / U_s split, blended type-1 / type-2 strategies with their per-instance state) on this wavefront's own LDS block (eight instance blocks
// of type Inst), which the cycle no longer needs.  The instance's inputs are untouched (nothing was written for it, no integrator advanced), so
// the result is what the list launch behind the kernel used to produce -- without the launch, which cost 4.5 us per cycle whether or not
// anything was on the list.  Everything the tail needs is in HBM or batch-uniform: no register of the ordinary path lives across it.
template <class Inst>
__device__ __forceinline__ void oct_slow_tail(const CycleParams& P, const bool flagged, Inst* lds) {
	const unsigned long long votes = __ballot(flagged);
	if (__builtin_expect(votes == 0ull, 1)) return;  // wave-uniform: the usual case
	static_assert(sizeof(WgSmem<8>) <= 8 * sizeof(Inst), "the general kernel's block fits the eight instance blocks of a wavefront");
	WgSmem<8>& wsm = *reinterpret_cast<WgSmem<8>*>(lds);
	for (int g = 0; g < 8; g++) {
		const int l0 = ((g >> 1) << 4) | (g & 1);  // the lane of joint 0 of instance g (octl_grp / octl_r)
		if (((votes >> l0) & 1ull) == 0ull) continue;    // wave-uniform
		SAIP_WG_SYNC();  // the block's previous user (the cycle, or the instance before) is done with it
		wg_cycle<8, 64>(P, (int)blockIdx.x * 8 + g, wsm);
	}
}

// does a launch of `workgroups` two-wavefront workgroups fit the chip in one round (two workgroups per CU = one wavefront per SIMD: 4096
// instances on 256 CUs)?  Beyond that the second wavefront only competes for issue slots (measured, B = 6144: 14.3 us against 10.8 us).
inline bool oct_duo_enabled(const int workgroups) {
	static int cus = 0;
	if (cus == 0) {
		int dev = 0, n = 0;
		if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
		cus = n;
	}
	return workgroups <= 2 * cus;
}

}  // namespace saip
