// fs2_mapreadout.hip -- the map readout on the device (fs2.h fs2_map_summary,
// fs2_map_density): the counts, the bounding box and a 2-D histogram of
// every live landmark of every particle, from the page pool as it stands.  Resampled
// siblings share pages, so the readout opens each distinct page once, weighted by the
// particles that refer to it.  Nothing here writes filter state.
//
//   k_map_counts  T = sum cnt, R = sum ceil(cnt / 8), max cnt: integer reductions of cnt
//   k_map_tally   one lane per (page-table row, particle), rows outer: the live entry's
//                 page gets the particle's amount q (1, or rint(w 2^e)) added to
//                 amount[page], its fill (live positions) and its referenced mark
//   k_map_extent  one lane per (pool page, position): the bounding box of the fp64 means
//                 of the referenced pages' live positions and the count U of those pages
//   k_map_bin     the same lanes: amount[page] added to the cell of each live position's
//                 fp64 mean, through a per-workgroup LDS table keyed by cell
//
// Every sum is of integers in 64-bit counters (integer atomics only), exact and
// independent of order; the box is a minimum / maximum, independent of order as well.
#include <hip/hip_runtime.h>

#include "fs2_mapreadout.hpp"
#include "fs2_reduce.hpp"

namespace fs2 {

namespace {

constexpr unsigned kMcGrid = 1024;

__global__ __launch_bounds__(kBlock) void k_map_counts(const int32_t *__restrict__ cnt, int64_t n,
                                                       unsigned long long *__restrict__ counts) {
    __shared__ unsigned long long lds[kBlock / 64];
    unsigned long long T = 0, R = 0;
    int mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int c = max(cnt[i], 0);
        T += (unsigned long long)c;
        R += (unsigned long long)((c + kPageSlots - 1) / kPageSlots);
        mx = max(mx, c);
    }
    T = block_sum_u64<kBlock>(T, lds);
    R = block_sum_u64<kBlock>(R, lds);
    mx = wave_max_i(mx);
    if (threadIdx.x == 0) {
        if (T) atomicAdd(counts + kMcT, T);
        if (R) atomicAdd(counts + kMcR, R);
    }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(counts + kMcMax, (unsigned long long)mx);
}

// One lane per (row, particle), rows outer: a wave reads 64 consecutive entries of one
// page-table row.  An owned entry is its page's only referent (fs2_kernels.hpp), so its
// amount is stored; a shared page's referents add theirs.  Every referent stores the
// same fill (DESIGN.md §15 "fill").
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_map_tally(MapRef map, const int32_t *__restrict__ cnt,
                                                      const double *__restrict__ w, int64_t n, int64_t lanes,
                                                      int32_t e, int64_t npool, MapTally tl) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool live = t < lanes;
    int row = 0, c = 0;
    int64_t i = 0;
    if (live) {
        row = (int)(t / n);
        i = t % n;
        c = cnt[i];
        live = row * kPageSlots < c;
    }
    Desc d = 0;
    if (live) d = *pt_entry(map, row, i);
    const int64_t id = (int64_t)(d & kIdMask);
    if (live && id >= npool) {                                 // no live entry names a page past the pool:
        atomicAdd(tl.bad, 1ull);                               // counted, and the call fails on the host
        live = false;
    }
    unsigned long long q = 0;
    if (live) q = WEIGHTED ? (unsigned long long)rint(ldexp(w[i], e)) : 1ull;
    const bool shared = live && !(d & kOwned);
    // Resampled siblings sit side by side and name the same page: the shared entries of a
    // run of equal page ids in the wave add once, from the run's last lane (a segmented
    // sum over the wave; integers, so grouping changes nothing).
    const int64_t key = shared ? id : -1;
    const int64_t prev = __shfl_up(key, 1);
    const int head = (FS2_MAP_TALLY_PER_ENTRY || lane == 0 || key < 0 || key != prev) ? 1 : 0;
    const int next_head = __shfl_down(head, 1);               // (every lane takes part: no short-circuit)
    const bool last = lane == 63 || next_head != 0;
    unsigned long long v = q;
    int f = head;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long vu = __shfl_up(v, s);
        const int fu = __shfl_up(f, s);
        if (lane >= s && !f) {
            v += vu;
            f = fu;
        }
    }
    if (!live || (shared && !last)) return;
    tl.fill[id] = (uint8_t)min(c - row * kPageSlots, kPageSlots);
    tl.ref[id] = 1;
    if (!shared)
        tl.amount[id] = q;
    else if (v)
        atomicAdd(tl.amount + id, v);
}

// 8 consecutive lanes per page of the pool, each taking one position: its 16-byte
// mirror (one 128-byte line per 8 lanes) names the record whose fp64 mean is read.  A
// fixed grid strides over the pool, kMrAhead items per lane with their loads issued
// together (most pages of a pool are unreferenced; as k_mark_recs).
// f(amount, mx, my) for every live position of every referenced page; g() once per
// referenced page.
constexpr int kMrAhead = 4;
template <typename F, typename G>
__device__ __forceinline__ void for_live_landmarks(const char *__restrict__ pool, const char *__restrict__ recs,
                                                   int64_t npool, int64_t nrecs, const MapTally &tl, F f, G g) {
    const int64_t lanes = npool * kPageSlots;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; t0 < lanes; t0 += kMrAhead * stride) {
        bool live[kMrAhead];
        unsigned long long a[kMrAhead];
        uint32_t r[kMrAhead];
#pragma unroll
        for (int u = 0; u < kMrAhead; ++u) {
            const int64_t t = t0 + u * stride;
            const int64_t p = t / kPageSlots;
            const int pos = (int)(t % kPageSlots);
            const bool refd = t < lanes && tl.ref[p] != 0;
            if (refd && pos == 0) g();
            live[u] = refd && pos < (int)tl.fill[p];
            a[u] = live[u] ? tl.amount[p] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kMrAhead; ++u) {
            const int64_t t = t0 + u * stride;
            r[u] = live[u] ? mirror_rec(load_mirror(pool + (t / kPageSlots) * kPageBytes, (int)(t % kPageSlots)))
                           : 0xffffffffu;
        }
#pragma unroll
        for (int u = 0; u < kMrAhead; ++u) {
            if (!live[u]) continue;
            if ((int64_t)r[u] >= nrecs) {                      // no live mirror names a record past the pool:
                atomicAdd(tl.bad, 1ull);                       // counted, and the call fails on the host
                continue;
            }
            const double2 m = *reinterpret_cast<const double2 *>(recs + (int64_t)r[u] * kRecBytes);
            f(a[u], m.x, m.y);
        }
    }
}

__device__ __forceinline__ double me_identity(int r) {
    return r == kMeU ? 0.0 : (r <= kMeMinY ? (double)INFINITY : -(double)INFINITY);
}
__device__ __forceinline__ double me_combine(int r, double a, double b) {
    return r == kMeU ? a + b : (r <= kMeMinY ? fmin(a, b) : fmax(a, b));
}
// The workgroup's reduction of each lane's v[kMeRows] (waves on DPP, then the four wave
// results in wave order), row r stored to dst[r * stride].  The count is a sum of
// integers below 2^31 in doubles: exact in any order.
__device__ __forceinline__ void me_block_store(const double (&v)[kMeRows], double *dst, int64_t stride) {
    __shared__ double s_p[kBlock / 64][kMeRows];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < kMeRows; ++r) {
        double t;
        if (r == kMeU)
            t = wave_sum(v[r]);
        else if (r <= kMeMinY)
            t = lane63(dpp_scan(v[r], (double)INFINITY, [](double a, double b) { return fmin(a, b); }));
        else
            t = lane63(dpp_scan(v[r], -(double)INFINITY, [](double a, double b) { return fmax(a, b); }));
        if (lane == 0) s_p[wid][r] = t;
    }
    __syncthreads();
    if (threadIdx.x < kMeRows) {
        const int r = threadIdx.x;
        double t = s_p[0][r];
#pragma unroll
        for (int q = 1; q < kBlock / 64; ++q) t = me_combine(r, t, s_p[q][r]);
        dst[(int64_t)r * stride] = t;
    }
}

__global__ __launch_bounds__(kBlock) void k_map_extent(const char *__restrict__ pool, const char *__restrict__ recs,
                                                       int64_t npool, int64_t nrecs, MapTally tl,
                                                       double *__restrict__ part) {
    double v[kMeRows];
#pragma unroll
    for (int r = 0; r < kMeRows; ++r) v[r] = me_identity(r);
    for_live_landmarks(
        pool, recs, npool, nrecs, tl,
        [&](unsigned long long, double mx, double my) {
            v[kMeMinX] = fmin(v[kMeMinX], mx);
            v[kMeMinY] = fmin(v[kMeMinY], my);
            v[kMeMaxX] = fmax(v[kMeMaxX], mx);
            v[kMeMaxY] = fmax(v[kMeMaxY], my);
        },
        [&]() { v[kMeU] += 1.0; });
    me_block_store(v, part + blockIdx.x, gridDim.x);
}

// the nb columns of part[kMeRows][nb] into out[kMeRows] (one workgroup)
__global__ __launch_bounds__(kBlock) void k_map_fold(const double *__restrict__ part, int64_t nb,
                                                     double *__restrict__ out) {
    double v[kMeRows];
#pragma unroll
    for (int r = 0; r < kMeRows; ++r) v[r] = me_identity(r);
    for (int64_t b = threadIdx.x; b < nb; b += kBlock) {
#pragma unroll
        for (int r = 0; r < kMeRows; ++r) v[r] = me_combine(r, v[r], part[(int64_t)r * nb + b]);
    }
    me_block_store(v, out, 1);
}

// The table: a lane claims a free slot for its cell with an integer compare-and-swap
// and adds its amount with a 64-bit integer LDS add; after kMbProbes occupied slots of
// other cells (a full neighbourhood) it adds to memory.  Keys are never released, so a
// slot read as another cell's stays that cell's.  The table lives for the workgroup's
// whole stride over the pool and its nonzero amounts go to memory once, one global
// integer atomic each.
__global__ __launch_bounds__(kBlock) void k_map_bin(const char *__restrict__ pool, const char *__restrict__ recs,
                                                    int64_t npool, int64_t nrecs, MapTally tl, double x0, double y0,
                                                    double cell, int32_t nx, int32_t ny,
                                                    unsigned long long *__restrict__ grid) {
    __shared__ unsigned long long s_red[kBlock / 64];
#if !FS2_MAP_BIN_DIRECT
    __shared__ int s_key[kMbSlots];
    __shared__ unsigned long long s_val[kMbSlots];
    for (int c = threadIdx.x; c < kMbSlots; c += kBlock) {
        s_key[c] = -1;
        s_val[c] = 0;
    }
    __syncthreads();
#endif
    unsigned long long out = 0;
    for_live_landmarks(
        pool, recs, npool, nrecs, tl,
        [&](unsigned long long a, double mx, double my) {
            if (!a) return;
            const double fx = floor((mx - x0) / cell), fy = floor((my - y0) / cell);
            if (!(fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny)) {     // (true for NaN)
                out += a;
                return;
            }
            const int c = (int)fy * nx + (int)fx;              // < nx ny <= 2^24
#if FS2_MAP_BIN_DIRECT
            atomicAdd(grid + c, a);
#else
            int slot = (int)(((uint32_t)c * 2654435761u) >> 22);                       // 10 bits: kMbSlots
            static_assert(kMbSlots == 1 << 10, "hash width");
            bool done = false;
            for (int p = 0; p < kMbProbes && !done; ++p) {
                int k = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (k == -1) {
                    const int prev = atomicCAS(&s_key[slot], -1, c);
                    k = prev == -1 ? c : prev;
                }
                if (k == c) {
                    atomicAdd(&s_val[slot], a);
                    done = true;
                }
                slot = (slot + 1) & (kMbSlots - 1);
            }
            if (!done) atomicAdd(grid + c, a);
#endif
        },
        []() {});
#if !FS2_MAP_BIN_DIRECT
    __syncthreads();
    for (int c = threadIdx.x; c < kMbSlots; c += kBlock) {
        const int k = s_key[c];
        const unsigned long long t = s_val[c];
        if (k >= 0 && t) atomicAdd(grid + k, t);               // k < nx ny
    }
#endif
    out = block_sum_u64<kBlock>(out, s_red);
    if (threadIdx.x == 0 && out) atomicAdd(grid + (int64_t)nx * ny, out);              // the outside counter
}

}  // namespace

hipError_t launch_map_counts(const int32_t *cnt, int64_t n, unsigned long long *counts, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t nb = std::min<int64_t>((n + kBlock - 1) / kBlock, kMcGrid);
    hipLaunchKernelGGL(k_map_counts, dim3((unsigned)nb), dim3(kBlock), 0, s, cnt, n, counts);
    return hipGetLastError();
}

hipError_t launch_map_tally(MapRef map, const int32_t *cnt, const double *w, int64_t n, int32_t rows, int32_t e,
                            int64_t npool, MapTally t, hipStream_t s) {
    const int64_t lanes = (int64_t)rows * n;
    if (lanes <= 0 || npool <= 0) return hipSuccess;
    const int64_t nb = (lanes + kBlock - 1) / kBlock;
    if (nb > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    if (w)
        hipLaunchKernelGGL(k_map_tally<true>, dim3((unsigned)nb), dim3(kBlock), 0, s, map, cnt, w, n, lanes, e, npool, t);
    else
        hipLaunchKernelGGL(k_map_tally<false>, dim3((unsigned)nb), dim3(kBlock), 0, s, map, cnt, w, n, lanes, e, npool,
                           t);
    return hipGetLastError();
}

hipError_t launch_map_extent(const char *pool, const char *recs, int64_t npool, int64_t nrecs, MapTally t,
                             double *part, double *out, hipStream_t s) {
    const int64_t nb = map_page_blocks(npool);
    hipLaunchKernelGGL(k_map_extent, dim3((unsigned)nb), dim3(kBlock), 0, s, pool, recs, npool, nrecs, t, part);
    hipLaunchKernelGGL(k_map_fold, dim3(1), dim3(kBlock), 0, s, part, nb, out);
    return hipGetLastError();
}

hipError_t launch_map_bin(const char *pool, const char *recs, int64_t npool, int64_t nrecs, MapTally t, double x0,
                          double y0, double cell, int32_t nx, int32_t ny, unsigned long long *grid, hipStream_t s) {
    if (npool <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_bin, dim3((unsigned)map_page_blocks(npool)), dim3(kBlock), 0, s, pool, recs, npool, nrecs,
                       t, x0, y0, cell, nx, ny, grid);
    return hipGetLastError();
}

}  // namespace fs2
