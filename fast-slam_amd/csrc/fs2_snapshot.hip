// fs2_snapshot.hip -- kernels of the compact snapshot (fs2_snapshot.hpp: format and
// validation; fs2_api.hip: fs2_snapshot_save / fs2_snapshot_load).
//
// Save.  The pools' collection marks (fs2_pages.hip: k_mark, k_mark_recs, a fresh
// epoch) say which pages and records are live; per pool
//   k_snap_count  live ids per 4096-id block, from 16-byte mark loads
//   k_sweep_scan  exclusive scan of the block counts (fs2_pages.hip)
//   k_snap_table  old id -> compact id (0xffffffff: not live), 64 B of table per lane,
//                 and compact id -> old id, staged in LDS and stored contiguously
// then, piece by piece into the staging buffer,
//   k_snap_rows   the page table's rows, entries renumbered, the owned bit kept
//   k_snap_gather pages (8 lanes x 16 B each, the record id renumbered in the lane that
//                 holds it) and records (3 lanes x 16 B each), contiguous stores
// A selection (fs2_snapshot_save_select: particles idx[0 .. m)) differs in what is
// marked and in how the per-particle sections are read:
//   k_snap_mark_sel     the page marks of the selected maps alone (m x R entries)
//   k_snap_scalars_sel  x, y, yaw, w, cnt gathered through idx
//   k_snap_rows_sel     the rows gathered through idx; the owned bit only where the
//                       source particle was taken once
// The record marks, the compaction and the gathers of pages and records are the same.
//
// Restore.  Pieces of the pages and records sections are scattered to the reserved
// pool ids (k_snap_scatter), still with the snapshot's compact record ids; the rows
// and counts wait in the handle's other buffer set.  k_snap_check then runs
// snap_check_particles on what is installed (pass 0: ranges, who names each page;
// pass 1: the owned entries), and only when it found nothing do k_snap_commit_pages /
// k_snap_commit_rows renumber mirrors and entries to pool ids, the rows into the live
// page table.  Nothing the handle reads changes before that.
#include "fs2_reduce.hpp"
#include "fs2_snapshot.hpp"

namespace fs2 {

static_assert(kSnapOwned == kOwned && kSnapSlotBits == kSlotBits && kSnapMaxRows == kMaxRows, "snapshot constants");

constexpr int kSnapPer = 16;                        // ids per thread: one 16-byte mark load
constexpr int kSnapBlock = kBlock * kSnapPer;       // ids per workgroup (== the sweep's: collect_blocks)

// live ids among the kSnapPer consecutive ids from id0 (bit e: id0 + e)
__device__ __forceinline__ unsigned live_bits(const uint8_t *mark, int64_t npool, uint8_t epoch, int64_t id0) {
    unsigned bits = 0;
    if (id0 + kSnapPer <= npool) {
        const uint4 v = *reinterpret_cast<const uint4 *>(mark + id0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (((w[q] >> (8 * b)) & 0xffu) == epoch) bits |= 1u << (4 * q + b);
    } else {
        for (int e = 0; e < kSnapPer; ++e)
            if (id0 + e < npool && mark[id0 + e] == epoch) bits |= 1u << e;
    }
    return bits;
}

__global__ __launch_bounds__(kBlock) void k_snap_count(const uint8_t *mark, int64_t npool, uint8_t epoch,
                                                       int64_t *bcnt) {
    __shared__ int lds[kBlock / 64];
    const int64_t id0 = (int64_t)blockIdx.x * kSnapBlock + (int64_t)threadIdx.x * kSnapPer;
    int tot;
    block_excl_scan(__popc(live_bits(mark, npool, epoch, id0)), lds, &tot);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_snap_table(const uint8_t *mark, int64_t npool, uint8_t epoch,
                                                       const int64_t *bcnt, uint32_t *tab, uint32_t *list) {
    __shared__ int lds[kBlock / 64];
    __shared__ uint32_t s_ids[kSnapBlock];
    const int64_t id0 = (int64_t)blockIdx.x * kSnapBlock + (int64_t)threadIdx.x * kSnapPer;
    const unsigned bits = live_bits(mark, npool, epoch, id0);
    int tot;
    int pos = block_excl_scan(__popc(bits), lds, &tot);
    const int64_t base = bcnt[blockIdx.x];
    uint32_t v[kSnapPer];
#pragma unroll
    for (int e = 0; e < kSnapPer; ++e) {
        v[e] = kSnapNone;
        if (bits & (1u << e)) {
            v[e] = (uint32_t)(base + pos);
            s_ids[pos++] = (uint32_t)(id0 + e);
        }
    }
    if (id0 + kSnapPer <= npool) {
        uint4 *q = reinterpret_cast<uint4 *>(tab + id0);
#pragma unroll
        for (int k = 0; k < kSnapPer / 4; ++k) q[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
        for (int e = 0; e < kSnapPer; ++e)
            if (id0 + e < npool) tab[id0 + e] = v[e];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tot; j += kBlock) list[base + j] = s_ids[j];
}

hipError_t launch_snap_count(const uint8_t *mark, int64_t npool, uint8_t epoch, int64_t *bcnt, hipStream_t s) {
    const int64_t nb = collect_blocks(npool);
    if (nb > 0) hipLaunchKernelGGL(k_snap_count, dim3((unsigned)nb), dim3(kBlock), 0, s, mark, npool, epoch, bcnt);
    return hipGetLastError();
}

hipError_t launch_snap_table(const uint8_t *mark, int64_t npool, uint8_t epoch, const int64_t *bcnt, uint32_t *tab,
                             uint32_t *list, hipStream_t s) {
    const int64_t nb = collect_blocks(npool);
    if (nb > 0)
        hipLaunchKernelGGL(k_snap_table, dim3((unsigned)nb), dim3(kBlock), 0, s, mark, npool, epoch, bcnt, tab, list);
    return hipGetLastError();
}

static unsigned snap_grid(int64_t total) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kBlock - 1) / kBlock, 8192));
}

// rows [r0, r0 + nrows) of the page table as the snapshot stores them
__global__ __launch_bounds__(kBlock) void k_snap_rows(const Desc *pt, int64_t n, const int32_t *cnt,
                                                      const uint32_t *ptab, int64_t npool, int r0, int nrows,
                                                      uint32_t *out) {
    const int64_t total = (int64_t)nrows * n;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int r = r0 + (int)(t / n);
        const int64_t i = t % n;
        uint32_t o = kSnapNone;
        if (r < (cnt[i] + kPageSlots - 1) / kPageSlots) {
            const uint32_t e = pt[(int64_t)r * n + i];
            const uint32_t id = e & kIdMask;
            if ((int64_t)id < npool) o = ptab[id] | (e & kOwned);
        }
        out[t] = o;
    }
}

hipError_t launch_snap_rows(MapRef map, const int32_t *cnt, const uint32_t *ptab, int64_t npool, int r0, int nrows,
                            uint32_t *out, hipStream_t s) {
    const int64_t total = (int64_t)nrows * map.n;
    if (total > 0)
        hipLaunchKernelGGL(k_snap_rows, dim3(snap_grid(total)), dim3(kBlock), 0, s, map.pt, map.n, cnt, ptab, npool,
                           r0, nrows, out);
    return hipGetLastError();
}

// ---- a selection: particles idx[0 .. m) of the handle (fs2_snapshot_save_select) ----

// The page marks of the selected maps alone.  One lane per (block of 8 rows, k), k
// fastest: the idx loads coalesce, and so do the table loads of a contiguous idx (a
// slice).  The entries are loaded 8 at a time before the mark stores, which may alias
// them (k_mark, fs2_pages.hip).  A source taken twice stores the same byte to the same
// address twice.
__global__ __launch_bounds__(kBlock) void k_snap_mark_sel(const MapRef map, const int32_t *cnt, const int64_t *idx,
                                                          int64_t m, int nblk, int64_t npool, uint8_t *mark,
                                                          uint8_t epoch) {
    const int64_t total = (int64_t)nblk * m;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int r0 = (int)(t / m) * 8;
        const int64_t i = idx[t % m];
        const int rows = (cnt[i] + kPageSlots - 1) / kPageSlots;
        if (r0 >= rows) continue;
        uint32_t e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = *pt_entry(map, min(r0 + u, rows - 1), i);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t id = e[u] & kIdMask;
            if (r0 + u < rows && (int64_t)id < npool) mark[id] = epoch;
        }
    }
}

hipError_t launch_snap_mark_sel(MapRef map, const int32_t *cnt, const int64_t *idx, int64_t m, int R, int64_t npool,
                                uint8_t *mark, uint8_t epoch, hipStream_t s) {
    const int nblk = (R + 7) / 8;
    if (nblk > 0)
        hipLaunchKernelGGL(k_snap_mark_sel, dim3(snap_grid(nblk * m)), dim3(kBlock), 0, s, map, cnt, idx, m, nblk,
                           npool, mark, epoch);
    return hipGetLastError();
}

// rows [r0, r0 + nrows) of the selection's page table: column k is particle idx[k]'s;
// the owned bit survives only where that particle was taken once (sel == 1)
__global__ __launch_bounds__(kBlock) void k_snap_rows_sel(const Desc *pt, int64_t n, const int32_t *cnt,
                                                          const int64_t *idx, const uint8_t *sel, int64_t m,
                                                          const uint32_t *ptab, int64_t npool, int r0, int nrows,
                                                          uint32_t *out) {
    const int64_t total = (int64_t)nrows * m;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int r = r0 + (int)(t / m);
        const int64_t i = idx[t % m];
        uint32_t o = kSnapNone;
        if (r < (cnt[i] + kPageSlots - 1) / kPageSlots) {
            const uint32_t e = pt[(int64_t)r * n + i];
            const uint32_t id = e & kIdMask;
            if ((int64_t)id < npool) o = ptab[id] | (sel[i] == 1 ? e & kOwned : 0u);
        }
        out[t] = o;
    }
}

hipError_t launch_snap_rows_sel(MapRef map, const int32_t *cnt, const int64_t *idx, const uint8_t *sel, int64_t m,
                                const uint32_t *ptab, int64_t npool, int r0, int nrows, uint32_t *out,
                                hipStream_t s) {
    const int64_t total = (int64_t)nrows * m;
    if (total > 0)
        hipLaunchKernelGGL(k_snap_rows_sel, dim3(snap_grid(total)), dim3(kBlock), 0, s, map.pt, map.n, cnt, idx, sel,
                           m, ptab, npool, r0, nrows, out);
    return hipGetLastError();
}

// out[j] = src[idx[j]], j < k: a piece of x, y, yaw, w (fp64) or of cnt
template <typename T>
__global__ __launch_bounds__(kBlock) void k_snap_scalars_sel(const T *src, const int64_t *idx, int64_t k, T *out) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < k; t += (int64_t)gridDim.x * kBlock)
        out[t] = src[idx[t]];
}

hipError_t launch_snap_scalars_sel(const double *src, const int64_t *idx, int64_t k, double *out, hipStream_t s) {
    if (k > 0) hipLaunchKernelGGL(k_snap_scalars_sel<double>, dim3(snap_grid(k)), dim3(kBlock), 0, s, src, idx, k, out);
    return hipGetLastError();
}

hipError_t launch_snap_scalars_sel(const int32_t *src, const int64_t *idx, int64_t k, int32_t *out, hipStream_t s) {
    if (k > 0) hipLaunchKernelGGL(k_snap_scalars_sel<int32_t>, dim3(snap_grid(k)), dim3(kBlock), 0, s, src, idx, k, out);
    return hipGetLastError();
}

// Items ids[0 .. k) of a pool of L x 16-byte items (a page: 8, a record: 3) into out,
// one 16-byte lane per piece.  rtab (pages only): the record id in each mirror's .w
// renumbered, 0xffffffff when it names no live record.
__global__ __launch_bounds__(kBlock) void k_snap_gather(const char *pool, const uint32_t *ids, int64_t k, int L,
                                                        const uint32_t *rtab, int64_t nrecs, uint4 *out) {
    const int64_t total = k * L;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t item = t / L;
        const int q = (int)(t % L);
        uint4 v = reinterpret_cast<const uint4 *>(pool)[(int64_t)ids[item] * L + q];
        if (rtab) v.w = (int64_t)v.w < nrecs ? rtab[v.w] : kSnapNone;
        out[t] = v;
    }
}

hipError_t launch_snap_gather(const char *pool, const uint32_t *ids, int64_t k, int L, const uint32_t *rtab,
                              int64_t nrecs, void *out, hipStream_t s) {
    if (k > 0)
        hipLaunchKernelGGL(k_snap_gather, dim3(snap_grid(k * L)), dim3(kBlock), 0, s, pool, ids, k, L, rtab, nrecs,
                           reinterpret_cast<uint4 *>(out));
    return hipGetLastError();
}

// The reverse: item j of in to pool id ids[j], verbatim.
__global__ __launch_bounds__(kBlock) void k_snap_scatter(const uint4 *in, const uint32_t *ids, int64_t k, int L,
                                                         char *pool) {
    const int64_t total = k * L;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock)
        reinterpret_cast<uint4 *>(pool)[(int64_t)ids[t / L] * L + t % L] = in[t];
}

hipError_t launch_snap_scatter(const void *in, const uint32_t *ids, int64_t k, int L, char *pool, hipStream_t s) {
    if (k > 0)
        hipLaunchKernelGGL(k_snap_scatter, dim3(snap_grid(k * L)), dim3(kBlock), 0, s,
                           reinterpret_cast<const uint4 *>(in), ids, k, L, pool);
    return hipGetLastError();
}

// One lane per particle.  flags[0]: the first violated rule a lane met (0: none),
// flags[1]: some map needs all R rows.
__global__ __launch_bounds__(kBlock) void k_snap_check(const SnapView v, int pass, uint32_t *owners, uint8_t *shared,
                                                       uint32_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= v.n) return;
    const int code = snap_check_particles(v, i, i + 1, pass, owners, shared, flags + 1);
    if (code != kSnapOk && code != kSnapRowsExact) atomicCAS(flags, 0u, (uint32_t)code);
}

hipError_t launch_snap_check(const SnapView &v, int pass, uint32_t *owners, uint8_t *shared, uint32_t *flags,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_snap_check, dim3((unsigned)((v.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, v, pass,
                       owners, shared, flags);
    return hipGetLastError();
}

// The installed pages' mirrors: compact record id -> the pool id it was installed at
// (one lane per mirror; a mirror that names no record of the snapshot gets 0xffffffff).
__global__ __launch_bounds__(kBlock) void k_snap_commit_pages(char *pool, const uint32_t *pids, int64_t U,
                                                              const uint32_t *rids, int64_t C) {
    const int64_t total = U * kPageSlots;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        uint32_t *w = reinterpret_cast<uint32_t *>(pool + (int64_t)pids[t / kPageSlots] * kPageBytes +
                                                   (t % kPageSlots) * 16 + 12);
        const uint32_t r = *w;
        *w = (int64_t)r < C ? rids[r] : kSnapNone;
    }
}

// The checked rows src [R][n] into the live page table dst, compact page id -> pool
// id; entries past a map's end are left as they are (never read).
__global__ __launch_bounds__(kBlock) void k_snap_commit_rows(const uint32_t *src, Desc *dst, int64_t n, int R,
                                                             const int32_t *cnt, const uint32_t *pids, int64_t U) {
    const int64_t total = (int64_t)R * n;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int r = (int)(t / n);
        const int64_t i = t % n;
        if (r >= (cnt[i] + kPageSlots - 1) / kPageSlots) continue;
        const uint32_t e = src[t];
        const uint32_t id = e & kIdMask;
        if ((int64_t)id < U) dst[t] = pids[id] | (e & kOwned);
    }
}

hipError_t launch_snap_commit(char *pool, const uint32_t *pids, int64_t U, const uint32_t *rids, int64_t C,
                              const uint32_t *src, Desc *dst, int64_t n, int R, const int32_t *cnt, hipStream_t s) {
    if (U > 0)
        hipLaunchKernelGGL(k_snap_commit_pages, dim3(snap_grid(U * kPageSlots)), dim3(kBlock), 0, s, pool, pids, U,
                           rids, C);
    if (R > 0)
        hipLaunchKernelGGL(k_snap_commit_rows, dim3(snap_grid((int64_t)R * n)), dim3(kBlock), 0, s, src, dst, n, R,
                           cnt, pids, U);
    return hipGetLastError();
}

}  // namespace fs2
