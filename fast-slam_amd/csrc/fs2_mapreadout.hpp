// fs2_mapreadout.hpp -- what the host entry points and the kernels of the map readout
// share (fs2_mapreadout.hip; fs2.h fs2_map_summary / fs2_map_density):
// the layout of the per-page scratch and of the results, and the launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs2_kernels.hpp"

namespace fs2 {

// ---- per-page scratch: one block of npool * kMrPageBytes bytes, zeroed before a tally ----
//   amount[npool] uint64   sum of the amounts q_i of the particles that refer to the page
//   fill[npool]   uint8    live positions of the page: min(cnt_i - 8 row, 8), the same
//                          for every referent (DESIGN.md §15 "fill")
//   ref[npool]    uint8    1 when a live page-table entry names the page (a weighted
//                          page whose referents all have q = 0 still counts in U)
constexpr size_t kMrPageBytes = 8 + 1 + 1;
struct MapTally {
    unsigned long long *amount;
    uint8_t *fill, *ref;
    unsigned long long *bad;               // the kMcBad cell of the counts (set by the caller)
};
inline MapTally map_tally_views(void *scratch, int64_t npool) {
    char *p = static_cast<char *>(scratch);
    return MapTally{reinterpret_cast<unsigned long long *>(p), reinterpret_cast<uint8_t *>(p + 8 * (size_t)npool),
                    reinterpret_cast<uint8_t *>(p + 9 * (size_t)npool), nullptr};
}

// ---- the counts of cnt: integer cells, zeroed by the caller ----
// kMcBad: live page-table entries naming a page past the pool and live mirrors naming a
// record past the pool, counted by the tally and the page passes.  Never nonzero on a
// sound handle; the entry points turn it into FS2_ERR_STATE instead of a quietly short grid.
enum { kMcT = 0, kMcR, kMcMax, kMcBad, kMcCells };

// ---- the page passes: 8 lanes per pool page, a fixed grid striding over the pool ----
constexpr unsigned kMrGrid = 2048;
// rows of the summary pass's partials part[kMeRows][blocks]: a sum, two minima, two maxima
enum { kMeU = 0, kMeMinX, kMeMinY, kMeMaxX, kMeMaxY, kMeRows };
inline int64_t map_page_blocks(int64_t npool) {
    const int64_t b = (npool * kPageSlots + kBlock - 1) / kBlock;
    return b < 1 ? 1 : (b > (int64_t)kMrGrid ? (int64_t)kMrGrid : b);
}

// The bin pass's LDS table: kMbSlots cell keys (int32, -1 free) and as many 64-bit
// amounts, 12 KiB -- inside the 16 KiB of the posterior's window (DESIGN.md §14
// "window size"), so it never limits occupancy either.  A lane probes kMbProbes
// consecutive slots before it adds straight to memory.
constexpr int kMbSlots = 1024;
constexpr int kMbProbes = 8;

// ---- launchers (fs2_mapreadout.hip); every buffer is the caller's ----
// counts[kMcCells], zeroed on s by the caller
hipError_t launch_map_counts(const int32_t *cnt, int64_t n, unsigned long long *counts, hipStream_t s);
// rows: page-table rows to visit (ceil(max cnt / 8) <= map.rows); w / e: the weighted
// amounts rint(w 2^e), w null: every amount 1.  The scratch was zeroed on s.
hipError_t launch_map_tally(MapRef map, const int32_t *cnt, const double *w, int64_t n, int32_t rows, int32_t e,
                            int64_t npool, MapTally t, hipStream_t s);
// part: [kMeRows][map_page_blocks(npool)] doubles; out[kMeRows]
hipError_t launch_map_extent(const char *pool, const char *recs, int64_t npool, int64_t nrecs, MapTally t,
                             double *part, double *out, hipStream_t s);
// grid: [ny][nx] counters followed by the outside counter, zeroed by the caller on s.
// Built with -DFS2_MAP_BIN_DIRECT=1 (build.py --variant) the pass has no LDS table:
// every landmark is one global atomic (the A/B of scripts/map_probe.py).
#ifndef FS2_MAP_BIN_DIRECT
#define FS2_MAP_BIN_DIRECT 0
#endif
// -DFS2_MAP_TALLY_PER_ENTRY=1: the tally adds one atomic per shared entry instead of one per
// run of equal page ids in a wave (the other A/B of scripts/map_probe.py).
#ifndef FS2_MAP_TALLY_PER_ENTRY
#define FS2_MAP_TALLY_PER_ENTRY 0
#endif
hipError_t launch_map_bin(const char *pool, const char *recs, int64_t npool, int64_t nrecs, MapTally t, double x0,
                          double y0, double cell, int32_t nx, int32_t ny, unsigned long long *grid, hipStream_t s);

}  // namespace fs2
