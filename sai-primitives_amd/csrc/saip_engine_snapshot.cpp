#include "saip_engine_internal.h"

// ---- state snapshots (saip_state_snapshot.hip): every per-instance array the engine owns, captured and written back through a
// per-instance source index.  The directory below is the list of those arrays; what is NOT on it is scratch or configuration.
struct SnapSegHost {
	std::string name;
	void* base = nullptr;      // the live array (nullptr on a configuration-only batch)
	int rows = 0, elem_bytes = 0, group = 1, kind = saip::SNAP_SOA;
	size_t bytes = 0;          // of the whole array, padding columns included
	size_t offset = 0;         // of the copy inside the snapshot's arena
};
static void snapshot_directory(const saip_batch* b, std::vector<SnapSegHost>& D) {
	D.clear();
	const size_t ld = b->ld;
	auto soa = [&](const std::string& name, void* base, int rows, int elem) {
		SnapSegHost S;
		S.name = name;
		S.base = base;
		S.rows = rows;
		S.elem_bytes = elem;
		S.bytes = (size_t)rows * ld * elem;
		D.push_back(S);
	};
	const int n = b->model->n;
	soa("q", b->q, n, 8);
	soa("dq", b->dq, n, 8);
	soa("tau", commanded_tau(b), n, 8);  // whichever the integrator reads
	soa("status", b->status, 1, 1);
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskHost& T = b->tasks[t];
		const std::string p = "task" + std::to_string(t) + ".";
		soa(p + "goal", T.goal_dev, T.dev.goal_comps, 8);
		soa(p + "integ", T.integ_dev, T.integ_rows, 8);
		soa(p + "integ_new", T.integ_new_dev, T.integ_rows, 8);
		if (T.otg_alloc) {
			soa(p + "desired", T.desired_dev, T.dev.goal_comps, 8);
			SnapSegHost S;
			S.name = p + "otg.state";
			S.base = T.otg.state;
			S.rows = saip::otg_state_fields();
			S.elem_bytes = 8;
			S.group = T.otg.gs;
			S.kind = saip::SNAP_GROUPED;
			S.bytes = (size_t)S.rows * (size_t)T.otg.lanes * 8;
			D.push_back(S);
			soa(p + "otg.time", T.otg.time, 1, 8);
			soa(p + "otg.duration", T.otg.duration, 1, 8);
			soa(p + "otg.flags", T.otg.flags, 1, 4);
			soa(p + "otg.seen_epoch", T.otg.seen_epoch, 1, 4);
			soa(p + "otg.result", T.otg.result, 1, 4);
			if (T.otg.frame) soa(p + "otg.frame", T.otg.frame, 21, 8);
		}
		if (T.dev.sh) {
			SnapSegHost S;
			S.name = p + "sh";
			S.base = T.dev.sh;
			S.rows = 1;
			S.elem_bytes = (int)sizeof(saip::ShState);
			S.kind = saip::SNAP_AOS;
			S.bytes = ld * sizeof(saip::ShState);
			D.push_back(S);
		}
		if (T.dev.popc) soa(p + "popc", T.dev.popc, 7 + T.dev.popc_cap, 8);
	}
	// the chains, sensing then actuation: attachments with state (delay taps, filter state, primed flags); absent while detached, so a
	// snapshot of another chain layout differs in a segment the comparison names
	for (const auto& [K, H] : {std::pair<const ChainKind&, const Chain&>{sense_chain_kind(), b->sensing.chain}, {plant_chain_kind(), b->plant.chain}}) {
		if (!H.attached) continue;
		const std::string p = std::string(K.snapshot) + ".";
		if (H.depth > 0) soa(p + "taps", H.taps, K.tap_rows * H.depth * n, 8);
		soa(p + "filt", H.filt, K.filt_rows * n, 8);
		soa(p + "primed", H.primed, n, 4);
	}
	// the guards: phase, counters and latch of every instance; absent while detached, like the chains
	if (b->guard.attached) {
		saip::GuardParams P;
		guard_segments(b, &P);
		soa("guard.phase", P.phase, 1, 4);
		soa("guard.since", P.since, 1, 4);
		soa("guard.clock", P.clock, 1, 4);
		soa("guard.run", P.run, P.G, 4);
		soa("guard.entry", P.entry, P.P, 4);
		soa("guard.fires", P.fires, P.G, 4);
		soa("guard.latch", P.latch, saip::GUARD_LATCH_ROWS, 8);
	}
	// the pushed object of link contact: pose and twist of every instance's body; absent while detached
	if (b->link_object.attached) soa("link_object.state", b->link_object.state, saip::LINK_OBJECT_STATE_ROWS, 8);
}
static_assert(sizeof(saip::ShState) % 4 == 0, "ShState is moved as 4- or 8-byte words");
static uint64_t snapshot_fingerprint(const saip_batch* b, const std::vector<SnapSegHost>& D) {
	uint64_t h = 1469598103934665603ull;  // FNV-1a
	auto mix = [&h](const void* p, size_t nb) {
		for (size_t i = 0; i < nb; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
	};
	auto mix_int = [&mix](int v) {
		const int32_t x = v;
		mix(&x, sizeof(x));
	};
	mix_int(b->model->n);
	mix_int(b->B);
	mix_int(b->ld);
	for (const auto& S : D) {
		mix(S.name.c_str(), S.name.size() + 1);
		mix_int(S.rows);
		mix_int(S.elem_bytes);
		mix_int(S.group);
	}
	return h;
}

// the host blob of saip_snapshot_export_host: this header, zero padding up to SNAP_HEADER_BYTES, then the segments at their offsets
struct SnapHeader {
	char magic[8];
	uint32_t version, n_segments;
	uint64_t fingerprint, bytes;
	int32_t otg_prelaunched, n_tasks;
	struct { int32_t sh_cycle, otg_inited; } task[SAIP_MAXT];
};
static const char kSnapMagic[8] = {'S', 'A', 'I', 'P', 'S', 'N', 'A', 'P'};
enum { SNAP_VERSION = 1, SNAP_HEADER_BYTES = 256, SNAP_ALIGN = 256 };
static_assert(sizeof(SnapHeader) == 104 && sizeof(SnapHeader) <= SNAP_HEADER_BYTES, "documented in saip.h");

struct saip_snapshot {
	saip_batch* owner = nullptr;         // nullptr once the batch is gone
	std::vector<SnapSegHost> segs;       // the layout fixed at creation (bases as they were then)
	uint64_t fingerprint = 0;
	size_t arena_bytes = 0;
	char* arena = nullptr;               // the copies, at segs[i].offset
	saip::SnapSeg* table = nullptr;      // [segs] device
	int* unit_seg = nullptr;             // [units] device: segment of every work unit
	int units = 0;
	int* map_dev = nullptr;              // [B]
	int* map_stage = nullptr;            // [B] pinned: the host map on its way to map_dev
	hipEvent_t map_ev = nullptr;         // the last upload from map_stage
	bool map_busy = false;
	bool filled = false;                 // a save or an import has happened: there is something to restore
	SnapHeader host;                     // the host scalars of the last save / import (and the header of an export)
};
void saip::eng::snapshot_release_device(saip_snapshot* s) {
	if (s->map_ev) (void)hipEventDestroy(s->map_ev);
	for (void* p : {(void*)s->arena, (void*)s->table, (void*)s->unit_seg, (void*)s->map_dev})
		if (p) (void)hipFree(p);
	if (s->map_stage) (void)hipHostFree(s->map_stage);
	s->arena = nullptr;
	s->table = nullptr;
	s->unit_seg = nullptr;
	s->map_dev = s->map_stage = nullptr;
	s->map_ev = nullptr;
	s->owner = nullptr;
}
static size_t snapshot_layout(std::vector<SnapSegHost>& D) {  // arena offsets; returns the arena size
	size_t at = 0;
	for (auto& S : D) {
		S.offset = at;
		at += (S.bytes + SNAP_ALIGN - 1) / SNAP_ALIGN * SNAP_ALIGN;
	}
	return at;
}
static void snapshot_host_scalars(const saip_batch* b, SnapHeader& H) {
	H.otg_prelaunched = b->otg_prelaunched ? 1 : 0;
	H.n_tasks = (int32_t)b->tasks.size();
	for (int t = 0; t < SAIP_MAXT; t++) {
		H.task[t].sh_cycle = t < (int)b->tasks.size() ? b->tasks[t].sh_cycle : 0;
		H.task[t].otg_inited = t < (int)b->tasks.size() && b->tasks[t].otg_inited ? 1 : 0;
	}
}
// the batch's directory as it is now against the snapshot's: the first segment that differs is named
static saip_status snapshot_match(saip_batch* b, const saip_snapshot* s, const char* fn) {
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch (a snapshot restores only into the batch that created it)", fn);
	if (!s->filled && strcmp(fn, "saip_batch_snapshot_save") != 0)
		return fail(SAIP_ERR_ORDER, "%s: the snapshot is empty (saip_batch_snapshot_save or saip_snapshot_import_host first)", fn);
	saip_status st = ensure_lazy_state(b);
	if (st) return st;
	std::vector<SnapSegHost> D;
	snapshot_directory(b, D);
	const size_t n = D.size() < s->segs.size() ? D.size() : s->segs.size();
	for (size_t i = 0; i <= n; i++) {
		const SnapSegHost* a = i < D.size() ? &D[i] : nullptr;
		const SnapSegHost* c = i < s->segs.size() ? &s->segs[i] : nullptr;
		if (!a && !c) break;
		if (!a || !c)
			return fail(SAIP_ERR_ORDER, "%s: the state layout changed since the snapshot was created: segment [%s] %s (create a new snapshot)", fn,
						(a ? a : c)->name.c_str(), a ? "is new" : "is gone");
		if (a->name != c->name || a->rows != c->rows || a->elem_bytes != c->elem_bytes || a->group != c->group || a->kind != c->kind)
			return fail(SAIP_ERR_ORDER, "%s: the state layout changed since the snapshot was created: segment [%s] where the snapshot has [%s] (create a new snapshot)",
						fn, a->name.c_str(), c->name.c_str());
		if (a->base != c->base)
			return fail(SAIP_ERR_ORDER, "%s: segment [%s] lives in another array than when the snapshot was created (create a new snapshot)", fn, a->name.c_str());
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_snapshot_create(saip_batch* b, saip_snapshot** out) {
	const char* fn = "saip_batch_snapshot_create";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = ensure_lazy_state(b))) return st;
	auto* s = new saip_snapshot();
	s->owner = b;
	snapshot_directory(b, s->segs);
	s->fingerprint = snapshot_fingerprint(b, s->segs);
	s->arena_bytes = snapshot_layout(s->segs);
	// the device table: one SnapSeg per segment, and the segment of every work unit
	std::vector<saip::SnapSeg> table;
	std::vector<int> unit_seg;
	long long units = 0;
	for (const auto& H : s->segs) {
		saip::SnapSeg S;
		memset(&S, 0, sizeof(S));
		S.rows = H.rows;
		if (H.kind == saip::SNAP_SOA) {
			S.wpi = 1;
			S.word_bytes = H.elem_bytes;
			S.row_stride = b->ld;
		} else if (H.kind == saip::SNAP_GROUPED) {
			S.wpi = H.group;
			S.word_bytes = 8;
			S.row_stride = (long long)b->B * H.group;
		} else {
			S.word_bytes = H.elem_bytes % 8 == 0 ? 8 : 4;
			S.wpi = H.elem_bytes / S.word_bytes;
			S.row_stride = 0;
		}
		S.words = (long long)b->B * S.wpi;
		const long long chunks = (S.words + saip::SNAP_CHUNK - 1) / saip::SNAP_CHUNK;
		const long long u = chunks * ((S.rows + saip::SNAP_ROWS - 1) / saip::SNAP_ROWS);
		if (units + u > 0x7fffffffll) {
			delete s;
			return fail(SAIP_ERR_UNSUPPORTED, "%s: the state of this batch is too large for one gather launch", fn);
		}
		S.chunks = (int)chunks;
		S.unit0 = (int)units;
		units += u;
		unit_seg.insert(unit_seg.end(), (size_t)u, (int)table.size());
		table.push_back(S);
	}
	s->units = (int)units;
	auto cleanup = [&](saip_status e) {
		snapshot_release_device(s);
		delete s;
		return e;
	};
	auto alloc = [&](void** p, size_t bytes) -> saip_status {
		HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
		return SAIP_OK;
	};
	if ((st = alloc((void**)&s->arena, s->arena_bytes)) || (st = alloc((void**)&s->table, table.size() * sizeof(saip::SnapSeg))) ||
		(st = alloc((void**)&s->unit_seg, unit_seg.size() * sizeof(int))) || (st = alloc((void**)&s->map_dev, (size_t)b->B * sizeof(int))))
		return cleanup(st);
	if (hipHostMalloc((void**)&s->map_stage, (size_t)b->B * sizeof(int), hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s->map_ev, hipEventDisableTiming) != hipSuccess)
		return cleanup(fail(SAIP_ERR_DEVICE, "%s: could not allocate the map staging buffer", fn));
	for (size_t i = 0; i < table.size(); i++) {
		table[i].live = (char*)s->segs[i].base;
		table[i].snap = s->arena + s->segs[i].offset;
	}
	if (hipMemsetAsync(s->arena, 0, s->arena_bytes ? s->arena_bytes : 1, b->stream) != hipSuccess ||
		hipMemcpyAsync(s->table, table.data(), table.size() * sizeof(saip::SnapSeg), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
		hipMemcpyAsync(s->unit_seg, unit_seg.data(), unit_seg.size() * sizeof(int), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
		hipStreamSynchronize(b->stream) != hipSuccess)  // table and unit_seg are stack objects
		return cleanup(fail(SAIP_ERR_DEVICE, "%s: could not write the segment table", fn));
	memset(&s->host, 0, sizeof(s->host));
	memcpy(s->host.magic, kSnapMagic, 8);
	s->host.version = SNAP_VERSION;
	s->host.n_segments = (uint32_t)s->segs.size();
	s->host.fingerprint = s->fingerprint;
	s->host.bytes = SNAP_HEADER_BYTES + s->arena_bytes;
	snapshot_host_scalars(b, s->host);
	b->snapshots.push_back(s);
	*out = s;
	return SAIP_OK;
}
extern "C" void saip_snapshot_destroy(saip_snapshot* s) {
	if (!s) return;
	if (s->owner) {
		saip_batch* b = s->owner;
		(void)hipSetDevice(b->device);
		if (b->stream) (void)hipStreamSynchronize(b->stream);  // a save or restore may still be in flight
		for (size_t i = 0; i < b->snapshots.size(); i++)
			if (b->snapshots[i] == s) {
				b->snapshots.erase(b->snapshots.begin() + i);
				break;
			}
		snapshot_release_device(s);
	}
	delete s;
}
// entry checks shared by save / restore / export: arguments first, then the device, then the layout
static saip_status snapshot_ready(saip_batch* b, const saip_snapshot* s, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if ((st = need_ready(b, fn))) return st;
	return snapshot_match(b, s, fn);
}
extern "C" saip_status saip_batch_snapshot_save(saip_batch* b, saip_snapshot* s) {
	const char* fn = "saip_batch_snapshot_save";
	saip_status st = snapshot_ready(b, s, fn);
	if (st) return st;
	hipError_t e = saip::launch_state_gather(s->table, s->unit_seg, s->units, b->B, nullptr, 1, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	snapshot_host_scalars(b, s->host);
	s->filled = true;
	return SAIP_OK;
}
static saip_status snapshot_restore(saip_batch* b, const saip_snapshot* s, const int* map_dev, const char* fn) {
	hipError_t e = saip::launch_state_gather(s->table, s->unit_seg, s->units, b->B, map_dev, 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	// the host scalars that give the restored arrays their meaning; the restored state is a new state
	for (size_t t = 0; t < b->tasks.size(); t++) {
		b->tasks[t].sh_cycle = s->host.task[t].sh_cycle;
		b->tasks[t].otg_inited = s->host.task[t].otg_inited != 0;
	}
	b->otg_prelaunched = s->host.otg_prelaunched != 0;
	b->models_valid = false;
	b->state_epoch++;
	b->state_pushed = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_snapshot_restore(saip_batch* b, const saip_snapshot* cs, const int* src_host) {
	const char* fn = "saip_batch_snapshot_restore";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!cs) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (src_host)
		for (int i = 0; i < b->B; i++)
			if (src_host[i] < 0 || src_host[i] >= b->B)
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: source index %d of instance %d is outside 0 .. %d", fn, src_host[i], i, b->B - 1);
	if ((st = need_ready(b, fn))) return st;
	if ((st = snapshot_match(b, cs, fn))) return st;
	if (!src_host) return snapshot_restore(b, cs, nullptr, fn);
	saip_snapshot* s = const_cast<saip_snapshot*>(cs);  // the staging buffer is the snapshot's own scratch, not part of what it holds
	if (s->map_busy) HIP_TRY(hipEventSynchronize(s->map_ev));  // the previous map has left the staging buffer (that upload only, not the device)
	memcpy(s->map_stage, src_host, (size_t)b->B * sizeof(int));
	HIP_TRY(hipMemcpyAsync(s->map_dev, s->map_stage, (size_t)b->B * sizeof(int), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipEventRecord(s->map_ev, b->stream));
	s->map_busy = true;
	return snapshot_restore(b, s, s->map_dev, fn);
}
extern "C" saip_status saip_batch_snapshot_restore_device(saip_batch* b, const saip_snapshot* s, const int* src_dev) {
	const char* fn = "saip_batch_snapshot_restore_device";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (!src_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null source map", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = snapshot_match(b, s, fn))) return st;
	return snapshot_restore(b, s, src_dev, fn);
}
extern "C" int saip_snapshot_segments(const saip_snapshot* s) { return s ? (int)s->segs.size() : 0; }
extern "C" saip_status saip_snapshot_segment_info(const saip_snapshot* s, int i, const char** name, int* rows, int* elem_bytes, int* group, int* kind, size_t* offset) {
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_snapshot_segment_info: null snapshot");
	if (i < 0 || i >= (int)s->segs.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_snapshot_segment_info: segment %d out of range (%d segments)", i, (int)s->segs.size());
	const SnapSegHost& S = s->segs[i];
	if (name) *name = S.name.c_str();
	if (rows) *rows = S.rows;
	if (elem_bytes) *elem_bytes = S.elem_bytes;
	if (group) *group = S.group;
	if (kind) *kind = S.kind;
	if (offset) *offset = SNAP_HEADER_BYTES + S.offset;
	return SAIP_OK;
}
extern "C" size_t saip_snapshot_bytes(const saip_snapshot* s) { return s ? SNAP_HEADER_BYTES + s->arena_bytes : 0; }
extern "C" saip_status saip_snapshot_export_host(saip_batch* b, const saip_snapshot* s, void* out, size_t bytes) {
	const char* fn = "saip_snapshot_export_host";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch", fn);
	if (bytes < SNAP_HEADER_BYTES + s->arena_bytes)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the buffer holds %zu bytes, the snapshot needs %zu (saip_snapshot_bytes)", fn, bytes, SNAP_HEADER_BYTES + s->arena_bytes);
	if ((st = need_ready(b, fn))) return st;
	memset(out, 0, SNAP_HEADER_BYTES);
	memcpy(out, &s->host, sizeof(SnapHeader));
	if (s->arena_bytes) HIP_TRY(hipMemcpyAsync((char*)out + SNAP_HEADER_BYTES, s->arena, s->arena_bytes, hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_snapshot_import_host(saip_batch* b, saip_snapshot* s, const void* in, size_t bytes) {
	const char* fn = "saip_snapshot_import_host";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!in) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null buffer", fn);
	// the blob against the layout of this batch: nothing here needs the device
	if (bytes < SNAP_HEADER_BYTES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: short buffer: %zu bytes do not hold the %d-byte header", fn, bytes, (int)SNAP_HEADER_BYTES);
	SnapHeader H;
	memcpy(&H, in, sizeof(H));
	if (memcmp(H.magic, kSnapMagic, 8) != 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: bad magic: not a state snapshot", fn);
	if (H.version != SNAP_VERSION) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: snapshot format version %u, this library reads version %d", fn, H.version, (int)SNAP_VERSION);
	std::vector<SnapSegHost> D;
	if (s) D = s->segs;
	else snapshot_directory(b, D);
	const uint64_t fp = s ? s->fingerprint : snapshot_fingerprint(b, D);
	const size_t need = SNAP_HEADER_BYTES + (s ? s->arena_bytes : snapshot_layout(D));
	if (H.fingerprint != fp)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrong fingerprint: the blob was taken from another state layout (%016llx, expected %016llx)", fn,
					(unsigned long long)H.fingerprint, (unsigned long long)fp);
	if (H.n_segments != D.size() || H.n_tasks != (int32_t)b->tasks.size() || H.bytes != need)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: inconsistent header (%u segments, %d tasks, %llu bytes)", fn, H.n_segments, (int)H.n_tasks, (unsigned long long)H.bytes);
	if (bytes < need) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: short buffer: %zu bytes, the snapshot has %zu", fn, bytes, need);
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch", fn);
	if ((st = need_ready(b, fn))) return st;
	if (s->arena_bytes) HIP_TRY(hipMemcpyAsync(s->arena, (const char*)in + SNAP_HEADER_BYTES, s->arena_bytes, hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the caller's buffer may be reused right away
	s->host = H;
	s->filled = true;
	return SAIP_OK;
}
