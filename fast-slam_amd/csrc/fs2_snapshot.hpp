// fs2_snapshot.hpp -- the compact snapshot of a handle (fs2_snapshot_save / _load /
// _check, include/fs2.h): its byte layout and its validation, as host/device code so
// that the host validator and the device's check kernel (fs2_snapshot.hip) run the
// same tests.
//
// A snapshot is the device representation written once: the particle scalars, the
// page table with its entries renumbered, every distinct live page, every distinct
// live record.  Little-endian; every section starts on a 64-byte boundary; pad bytes
// (between sections, after the last one up to `total`) are zero.
//
//   header   256 B  SnapHeader
//   scalars  36 N   x[N], y[N], yaw[N], w[N] fp64, cnt[N] int32 (the current buffer set)
//   rows     4 R N  uint32 [R][N], row-major like the device page table: the compact id
//                   of the page, kOwned (bit 31) copied from the live entry; entries of
//                   rows at or past ceil(cnt_i / 8) are 0xffffffff
//   pages    128 U  the 8 mirrors verbatim (fp32 x, y, s with the slot index in the low
//                   12 bits of s), .w = the compact record id, or 0xffffffff when the
//                   mirror's record is not live
//   records  48 C   fp64 x, y, P00, P01, P10, P11 verbatim
//
// R = ceil(max cnt / 8).  Compact ids are the rank of the pool id among the live pool
// ids, in id order, so a save of an unchanged handle is deterministic.  A page is live
// when a row below ceil(cnt_i / 8) names it; a record is live when a mirror of a live
// page names it (all 8 mirrors, as the pool's collection marks them: a mirror past the
// map's end in a partly filled last page may keep a stale record alive).  The row
// boxes are not stored: a restore rebuilds them from the pages.
//
// Selections (fs2_snapshot_save_select: particles idx[0 .. m) of a handle, repeats
// allowed, m may exceed N).  The result is an ordinary snapshot of m particles: output
// particle k carries x, y, yaw, w, cnt and the map of particle idx[k] verbatim (weights
// are not renormalised); scan, org, cell, ext_seen, slb and cnt_upper are the handle's.
//   - Liveness is over the selection: R = ceil(max selected cnt / 8) (0 when every
//     selected map is empty), a page is live when a row below ceil(cnt / 8) of a
//     selected particle names it, a record when a mirror of such a page names it.
//     Compact ids are the rank among those live ids, so R, U, C are the selection's own.
//   - An entry keeps its owned bit only if its source particle occurs exactly once in
//     idx (snap_select_classes); otherwise the bit is cleared.  That is sufficient for
//     the rule below: in the handle no other particle names an owned page, so in the
//     selection only copies of the same particle could, and theirs are all cleared.
//     The copies of a repeated particle share its pages un-owned and copy them at their
//     first write, as resampled siblings do.
//   - idx = 0 .. N - 1 gives the full save byte for byte: the same marks, every
//     particle taken once.
//   - Not promised: an un-owned entry whose sharers were not selected stays un-owned
//     (one page copy more at its first write, nothing else).
//
// Valid (snap_check_header, then snap_check_particles passes 0 and 1):
//   - the header is self-consistent: magic, version, header size, the layout constants,
//     counts in range, the section table equal to snap_layout's, total == size;
//   - 0 <= cnt_i <= min(8 R, cnt_upper), and some map needs exactly R rows;
//   - every row entry below ceil(cnt_i / 8) names a page < U;
//   - mirror position p < min(8, cnt_i - 8 r) of that page has a record id < C and a
//     slot index < cnt_i (positions past the map's end are not looked at);
//   - a page named by an entry with the owned bit is named by no other entry.
// Every index is tested before it addresses anything.  NOT checked: that the slot
// indices of a map are a permutation of 0 .. cnt - 1.  A snapshot whose maps repeat or
// skip an index loads; such a map exports (fs2_get_state) with a slot written twice and
// another left zero, and associates in the order its pages give, but no access leaves
// its buffers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fs2 {

constexpr uint32_t kSnapVersion = 1;
constexpr int kSnapHeaderBytes = 256;
constexpr int kSnapAlign = 64;
constexpr uint32_t kSnapNone = 0xffffffffu;      // a row entry past the map, a mirror without a live record
constexpr uint32_t kSnapOwned = 0x80000000u;     // == kOwned
constexpr uint32_t kSnapSlotBits = 0xfffu;       // == kSlotBits
constexpr int64_t kSnapMaxRows = 512;            // == kMaxRows
constexpr int64_t kSnapMaxParticles = (int64_t)1 << 40;
enum : int { kSnapScalars, kSnapRows, kSnapPages, kSnapRecords, kSnapSections };

struct SnapHeader {
    char magic[8];               // "FS2SNAP\0"
    uint32_t version;            // kSnapVersion
    uint32_t header_bytes;       // 256
    int64_t total;               // bytes of the whole snapshot
    uint32_t page_slots;         // 8
    uint32_t page_bytes;         // 128
    uint32_t rec_bytes;          // 48
    int32_t cnt_upper;           // the handle's upper bound on every map size
    int64_t n;                   // particles N
    int64_t rows;                // R
    int64_t pages;               // U
    int64_t records;             // C
    uint64_t scan;               // scans run (the Philox stream index of rng="device")
    float org, cell;             // summary grid (SumFrame; icell = 1 / cell)
    float ext_seen;              // largest |x|, |y| imported so far
    float slb;                   // lower bound on every nonzero mirror s
    int64_t sec[kSnapSections][2];   // offset, bytes of scalars, rows, pages, records
    uint8_t pad[96];
};
static_assert(sizeof(SnapHeader) == kSnapHeaderBytes, "SnapHeader layout");

__host__ __device__ inline int64_t snap_align(int64_t b) { return (b + kSnapAlign - 1) / kSnapAlign * kSnapAlign; }

// The section table of a snapshot of N particles, R rows, U pages, C records; returns
// the total byte count.
__host__ __device__ inline int64_t snap_layout(int64_t N, int64_t R, int64_t U, int64_t C,
                                               int64_t sec[kSnapSections][2]) {
    const int64_t bytes[kSnapSections] = {36 * N, 4 * R * N, 128 * U, 48 * C};
    int64_t at = kSnapHeaderBytes;
    for (int k = 0; k < kSnapSections; ++k) {
        sec[k][0] = at;
        sec[k][1] = bytes[k];
        at = snap_align(at + bytes[k]);
    }
    return at;
}

enum : int {
    kSnapOk = 0, kSnapShort, kSnapMagic, kSnapVersionBad, kSnapHeaderSize, kSnapConstants, kSnapCounts,
    kSnapSectionTable, kSnapTotal, kSnapCnt, kSnapRowsExact, kSnapMissing, kSnapEntry, kSnapRecord, kSnapSlot,
    kSnapOwnedShared, kSnapNumErrors
};
inline const char *snap_error_text(int code) {
    static const char *const t[kSnapNumErrors] = {
        "ok",
        "buffer shorter than the 256-byte header",
        "wrong magic",
        "unsupported format version",
        "wrong header size",
        "layout constants differ (8 slots per page, 128-byte pages, 48-byte records)",
        "a count is out of range (N, R, U, C, cnt_upper)",
        "a section lies outside the buffer, overlaps another or is not where the layout puts it",
        "size differs from the header's total",
        "a map size is outside [0, 8 R] or above cnt_upper",
        "no map needs R rows (R must be ceil(max cnt / 8))",
        "a row entry below ceil(cnt / 8) is missing (0xffffffff)",
        "a row entry names a page >= U",
        "a live mirror names a record >= C",
        "a live mirror's slot index is >= its map's size",
        "a page named by an owned entry is named by another entry",
    };
    return code >= 0 && code < kSnapNumErrors ? t[code] : "unknown";
}

__host__ __device__ inline int snap_check_header(const SnapHeader &h, int64_t size) {
    const char magic[8] = {'F', 'S', '2', 'S', 'N', 'A', 'P', 0};
    for (int k = 0; k < 8; ++k)
        if (h.magic[k] != magic[k]) return kSnapMagic;
    if (h.version != kSnapVersion) return kSnapVersionBad;
    if (h.header_bytes != (uint32_t)kSnapHeaderBytes) return kSnapHeaderSize;
    if (h.page_slots != 8 || h.page_bytes != 128 || h.rec_bytes != 48) return kSnapConstants;
    if (h.n < 1 || h.n > kSnapMaxParticles || h.rows < 0 || h.rows > kSnapMaxRows || h.pages < 0 ||
        h.pages > (int64_t)0x7fffffff || h.records < 0 || h.records > (int64_t)0xfffffffe ||
        h.pages > h.rows * h.n || h.records > 8 * h.pages || h.cnt_upper < 0 || h.cnt_upper > 8 * kSnapMaxRows)
        return kSnapCounts;
    // the one layout these counts have: sections in order, 64-byte aligned, disjoint
    int64_t sec[kSnapSections][2];
    const int64_t total = snap_layout(h.n, h.rows, h.pages, h.records, sec);
    for (int k = 0; k < kSnapSections; ++k)
        if (h.sec[k][0] != sec[k][0] || h.sec[k][1] != sec[k][1] || h.sec[k][0] < kSnapHeaderBytes ||
            h.sec[k][0] > size || h.sec[k][1] > size - h.sec[k][0])
            return kSnapSectionTable;
    if (h.total != total || size != total) return kSnapTotal;
    return kSnapOk;
}

// The sections as the checks address them.  On the device the pages are already
// installed in the pool, page k at pool id page_ids[k]; a host buffer has them in
// place (page_ids null).
struct SnapView {
    int64_t n, rows, pages, records;
    int32_t cnt_upper;
    const int32_t *cnt;          // [n]
    const uint32_t *row;         // [rows][stride]
    int64_t stride;
    const char *page;            // page k at page + 128 (page_ids ? page_ids[k] : k)
    const uint32_t *page_ids;
};

__host__ __device__ inline void snap_count_owner(uint32_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, 1u);            // (a valid snapshot: one owner per page, no two lanes meet)
#else
    *p += 1;
#endif
}

// Particles [i0, i1): the host runs it over all of them, a device lane over its own.
// pass 0 tests counts, entries and live mirrors and records who names each page:
// owners[k] counts the owned entries naming page k, shared[k] is set by an entry
// without the owned bit; *full is set by a map that needs all R rows.  pass 1 (after
// pass 0 of every particle) tests the owned entries against them.  Returns the first
// violated rule.
__host__ __device__ inline int snap_check_particles(const SnapView &v, int64_t i0, int64_t i1, int pass,
                                                    uint32_t *owners, uint8_t *shared, uint32_t *full) {
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t c = v.cnt[i];
        if (c < 0 || c > 8 * v.rows || c > v.cnt_upper) return kSnapCnt;
        const int64_t rows = (c + 7) / 8;
        if (pass == 0 && rows == v.rows) *full = 1u;
        for (int64_t r = 0; r < rows; ++r) {
            const uint32_t e = v.row[r * v.stride + i];
            const uint32_t id = e & ~kSnapOwned;
            if (e == kSnapNone) return kSnapMissing;
            if ((int64_t)id >= v.pages) return kSnapEntry;
            if (pass == 1) {
                if ((e & kSnapOwned) && (owners[id] != 1u || shared[id])) return kSnapOwnedShared;
                continue;
            }
            if (e & kSnapOwned) snap_count_owner(&owners[id]);
            else shared[id] = 1;
            const uint32_t *m =
                reinterpret_cast<const uint32_t *>(v.page + 128 * (int64_t)(v.page_ids ? v.page_ids[id] : id));
            const int64_t live = c - 8 * r < 8 ? c - 8 * r : 8;
            for (int64_t p = 0; p < live; ++p) {
                if ((int64_t)m[4 * p + 3] >= v.records) return kSnapRecord;
                if ((int64_t)(m[4 * p + 2] & kSnapSlotBits) >= c) return kSnapSlot;
            }
        }
    }
    if (pass == 0 && i0 == 0 && i1 == v.n && v.rows > 0 && !*full) return kSnapRowsExact;
    return kSnapOk;
}

// A selection's index list, in one pass on the host: sel[i] (n bytes, zero on entry)
// becomes 0, 1 or 2 -- particle i taken never, once, more than once.  Returns the first
// position k with idx[k] outside [0, n), or -1 when there is none.
inline int64_t snap_select_classes(const int64_t *idx, int64_t m, int64_t n, uint8_t *sel) {
    for (int64_t k = 0; k < m; ++k) {
        const int64_t i = idx[k];
        if (i < 0 || i >= n) return k;
        if (sel[i] < 2) ++sel[i];
    }
    return -1;
}

}  // namespace fs2
