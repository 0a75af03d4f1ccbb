// State snapshots: one launch that moves every per-instance array of a batch between the engine's arrays and a snapshot's copies,
// through a per-instance source index on the way back (restore, broadcast, resample: saip.h).
//
// Work: one workgroup of SNAP_CHUNK lanes per (segment, SNAP_CHUNK consecutive words of a row, block of SNAP_ROWS rows).  `unit_seg`
// (written once when the snapshot is created) maps the workgroup to its segment, the segment table gives the rest: both are
// wave-uniform scalar loads.  A lane writes the same word position in up to SNAP_ROWS rows, so every store instruction of a wavefront
// covers 64 consecutive words -- whole [ld] runs of the SoA arrays, whole gs-wide runs of the grouped OTG state, and the records of the
// array of structs as consecutive 8-byte words (never one lane per record).  The loads are whatever the map makes them: contiguous for
// a save, an identity restore and inside a record or lane group, scattered between instances otherwise.  No atomics, no counter, no LDS.
#include <hip/hip_runtime.h>

#include "saip_state_snapshot.h"

namespace saip {

__global__ void __launch_bounds__(SNAP_CHUNK) saip_state_gather(const SnapSeg* __restrict__ table, const int* __restrict__ unit_seg, int B,
																 const int* __restrict__ map, int save) {
	const SnapSeg S = table[unit_seg[blockIdx.x]];
	snap_gather_unit_any(S, B, map, save, (int)blockIdx.x - S.unit0, (int)threadIdx.x);
}

hipError_t launch_state_gather(const SnapSeg* table, const int* unit_seg, int units, int B, const int* map, int save, hipStream_t stream) {
	if (units <= 0) return hipSuccess;
	hipLaunchKernelGGL(saip_state_gather, dim3(units), dim3(SNAP_CHUNK), 0, stream, table, unit_seg, B, map, save);
	return hipGetLastError();
}

}  // namespace saip
