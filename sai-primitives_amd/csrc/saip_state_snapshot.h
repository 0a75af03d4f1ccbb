// State snapshots (saip_state_snapshot.hip): the descriptor of one per-instance device array and the indexing of the gather, shared by
// the kernel and by host-compiled checks (the function below is plain C++ when no HIP compiler is reading it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SAIP_SNAP_HD __host__ __device__
#else
#define SAIP_SNAP_HD
#endif

namespace saip {

// The three layouts the engine has reduce to one: an array is `rows` rows of `row_stride` words, and instance i owns the `wpi`
// consecutive words i*wpi .. i*wpi + wpi - 1 of every row.
//   rows x [ld] SoA of doubles / int / uint8_t:  wpi = 1, word = the element, row_stride = ld
//   lane-grouped OTG state [fields][B*gs]:       wpi = gs, word = 8 bytes, row_stride = B*gs
//   array of structs (ShState[ld]):              wpi = sizeof(record) / word, word = 8 (or 4) bytes, one row
enum { SNAP_SOA = 0, SNAP_GROUPED = 1, SNAP_AOS = 2 };
enum { SNAP_CHUNK = 256, SNAP_ROWS = 8 };  // one work unit (= one workgroup of SNAP_CHUNK lanes): SNAP_CHUNK consecutive words of up to SNAP_ROWS rows
enum { SNAP_MAX_SEGS = 4 + 13 * 8 };       // q dq tau status + 13 arrays per task (SAIP_MAXT tasks)

struct SnapSeg {
	char* live;             // the engine's array
	char* snap;             // the snapshot's copy: same shape
	long long row_stride;   // words
	long long words;        // B * wpi: the words of one row that belong to instances 0 .. B-1 (what lies behind is never touched)
	int rows, wpi, word_bytes;
	int unit0;              // first work unit of this segment
	int chunks;             // work units per row block = ceil(words / SNAP_CHUNK); unit u of the segment: chunk u % chunks, row block u / chunks
	int pad_;
};

// what lane `lane` of work unit `unit` (counted inside the segment) does.  save: snap <- live, column for column (map unused);
// otherwise live column i <- snap column map[i] (map == nullptr: i).  An entry outside 0 .. B-1 leaves the instance untouched and no
// address is formed from it.  Consecutive lanes write consecutive words.
template <typename W>
SAIP_SNAP_HD inline void snap_gather_unit(const SnapSeg& S, int B, const int* map, int save, int unit, int lane) {
	const int chunk = unit % S.chunks, rb = unit / S.chunks;
	const long long w = (long long)chunk * SNAP_CHUNK + lane;
	if (w >= S.words) return;
	const long long i = S.wpi == 1 ? w : w / S.wpi;
	const long long k = w - i * S.wpi;
	long long s = i;
	if (!save && map) {
		const int m = map[i];
		if (m < 0 || m >= B) return;
		s = m;
	}
	W* dst = (W*)(save ? S.snap : S.live) + w;
	const W* src = (const W*)(save ? S.live : S.snap) + (s * S.wpi + k);
	const int r0 = rb * SNAP_ROWS, r1 = r0 + SNAP_ROWS < S.rows ? r0 + SNAP_ROWS : S.rows;
	for (int r = r0; r < r1; r++) dst[(long long)r * S.row_stride] = src[(long long)r * S.row_stride];
}
SAIP_SNAP_HD inline void snap_gather_unit_any(const SnapSeg& S, int B, const int* map, int save, int unit, int lane) {
	if (S.word_bytes == 8) snap_gather_unit<uint64_t>(S, B, map, save, unit, lane);
	else if (S.word_bytes == 4) snap_gather_unit<uint32_t>(S, B, map, save, unit, lane);
	else snap_gather_unit<uint8_t>(S, B, map, save, unit, lane);
}

}  // namespace saip
