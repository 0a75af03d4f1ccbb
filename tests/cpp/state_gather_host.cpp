// The indexing of the state-snapshot gather kernel (csrc/saip_state_snapshot.h) compiled for the host as a plain function: every work
// unit and lane of one segment, in order.  Built by tests/test_state_snapshot_cpu.py as a shared object and called through ctypes.
#include "../../sai-primitives_amd/csrc/saip_state_snapshot.h"

extern "C" int saip_test_gather_segment(char* live, char* snap, long long row_stride, int rows, int wpi, int word_bytes, int B, const int* map, int save) {
	saip::SnapSeg S;
	S.live = live;
	S.snap = snap;
	S.row_stride = row_stride;
	S.words = (long long)B * wpi;
	S.rows = rows;
	S.wpi = wpi;
	S.word_bytes = word_bytes;
	S.unit0 = 0;
	S.chunks = (int)((S.words + saip::SNAP_CHUNK - 1) / saip::SNAP_CHUNK);
	S.pad_ = 0;
	const int units = S.chunks * ((rows + saip::SNAP_ROWS - 1) / saip::SNAP_ROWS);
	for (int u = 0; u < units; u++)
		for (int lane = 0; lane < saip::SNAP_CHUNK; lane++) saip::snap_gather_unit_any(S, B, map, save, u, lane);
	return units;
}
