// fs2_subsample.hip -- the weighted subsample on the device (fs2.h fs2_subsample;
// DESIGN.md §16): k particle indices drawn in proportion to the integer amounts
// q_i = rint(w_i 2^e) by the systematic sampler, and the drawn particles' scalars.
// Nothing here writes filter state.
//
// Scan.  The inclusive prefix C of the amounts, reduce-then-scan with a kernel boundary
// between the stages (no workgroup ever waits on another):
//   k_sub_totals   the total of each chunk of kPostChunk consecutive particles;
//   k_sub_bases    one workgroup: the exclusive prefix of the chunk totals, kPostBlock
//                  a turn with a running carry, and the grand total Q after them;
//   k_sub_rescan   each chunk scanned again from its base into C.
// Everything is 64-bit integer addition (Q <= 2^62), so C does not depend on the order
// of the additions, on the CU count or on scheduling.
// Select.  k_sub_select: one lane per output j; t_j by sub_threshold, then the chunk
// by a binary search of the bases and the particle by one inside the chunk's slice of C
// (-DFS2_SUB_FLAT_SELECT, the A/B of DESIGN.md §16: one search over the whole of C).
// Gather.  k_sub_gather: one lane per output copies the scalars of particle idx[j].
#include <hip/hip_runtime.h>

#include "fs2_reduce.hpp"
#include "fs2_subsample.hpp"

namespace fs2 {

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v) {
    return dpp_scan(v, 0ull, [](u64 a, u64 b) { return a + b; });
}

// the amount of particle i (k_pose_density's expression)
__device__ __forceinline__ u64 sub_amount(const double *__restrict__ w, int64_t i, int32_t e) {
    return (u64)rint(ldexp(w[i], e));
}

// The exclusive prefix of v over the workgroup and the workgroup's total.  Every thread
// calls it; s_w is free for reuse after the next barrier.
__device__ __forceinline__ u64 block_excl_scan_u64(u64 v, u64 (&s_w)[kPostBlock / 64], u64 *tot) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 inc = wave_incl_scan_u64(v);
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    u64 off = 0, t = 0;
#pragma unroll
    for (int u = 0; u < kPostBlock / 64; ++u) {
        if (u < wid) off += s_w[u];
        t += s_w[u];
    }
    *tot = t;
    return off + inc - v;
}

__global__ __launch_bounds__(kPostBlock) void k_sub_totals(const double *__restrict__ w, int64_t n, int32_t e,
                                                           u64 *__restrict__ tot) {
    __shared__ u64 s_w[kPostBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kPostChunk + threadIdx.x;
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < kPostPer; ++k) {
        const int64_t i = base + (int64_t)k * kPostBlock;
        if (i < n) v += sub_amount(w, i, e);
    }
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
#pragma unroll
        for (int u = 0; u < kPostBlock / 64; ++u) t += s_w[u];
        tot[blockIdx.x] = t;
    }
}

// one workgroup; base[b] = tot[0] + ... + tot[b - 1], base[nb] = Q
__global__ __launch_bounds__(kPostBlock) void k_sub_bases(const u64 *__restrict__ tot, int64_t nb,
                                                          u64 *__restrict__ base) {
    __shared__ u64 s_w[kPostBlock / 64];
    u64 carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kPostBlock) {          // (uniform: every thread takes every turn)
        const int64_t b = b0 + threadIdx.x;
        u64 turn;
        const u64 ex = block_excl_scan_u64(b < nb ? tot[b] : 0ull, s_w, &turn);
        if (b < nb) base[b] = carry + ex;
        carry += turn;
        __syncthreads();                                       // s_w is written again next turn
    }
    if (threadIdx.x == 0) base[nb] = carry;
}

__global__ __launch_bounds__(kPostBlock) void k_sub_rescan(const double *__restrict__ w, int64_t n, int32_t e,
                                                           const u64 *__restrict__ base, u64 *__restrict__ C) {
    __shared__ u64 s_w[kPostBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kPostChunk + (int64_t)threadIdx.x * kPostPer;
    u64 q[kPostPer];                                           // the lane's own inclusive prefix
    u64 v = 0;
    if (i0 + kPostPer <= n) {
#pragma unroll
        for (int k = 0; k < kPostPer; ++k) {
            v += sub_amount(w, i0 + k, e);
            q[k] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPostPer; ++k) {
            if (i0 + k < n) v += sub_amount(w, i0 + k, e);
            q[k] = v;
        }
    }
    u64 turn;
    const u64 off = base[blockIdx.x] + block_excl_scan_u64(v, s_w, &turn);
    if (i0 + kPostPer <= n) {
#pragma unroll
        for (int k = 0; k < kPostPer; ++k) C[i0 + k] = off + q[k];
    } else {
#pragma unroll
        for (int k = 0; k < kPostPer; ++k)
            if (i0 + k < n) C[i0 + k] = off + q[k];
    }
}

// Qp: the total on the device (the scan's base[nb]) or null for Qv.
__global__ __launch_bounds__(kPostBlock) void k_sub_select(SubScan sc, int64_t n, int64_t nb, const u64 *__restrict__ Qp,
                                                           u64 Qv, int64_t k, uint32_t offset,
                                                           int64_t *__restrict__ idx) {
    const int64_t j = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
    if (j >= k) return;
    const u64 Q = Qp ? *Qp : Qv;
    const u64 t = sub_threshold(Q, (u64)k, offset, (u64)j);
    if (!sc.C) {                                               // q_i = 1: C_i = i + 1
        idx[j] = (int64_t)t;                                   // t < Q = n
        return;
    }
    int64_t first = 0, last = n;
#ifndef FS2_SUB_FLAT_SELECT
    {
        // the chunk: base[lo] <= t < base[hi] throughout (base[0] = 0, base[nb] = Q > t)
        int64_t lo = 0, hi = nb;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;                // 0 < mid < nb
            if (sc.base[mid] <= t) lo = mid;
            else hi = mid;
        }
        first = lo * kPostChunk;
        last = min(n, first + (int64_t)kPostChunk);
    }
#endif
    // the smallest i of [first, last) with C_i > t; C[last - 1] = base[chunk + 1] > t, so
    // the answer lies in [lo, hi] throughout and mid < hi <= last - 1 < n
    int64_t lo = first, hi = last - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sc.C[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    idx[j] = lo;
}

__global__ __launch_bounds__(kPostBlock) void k_sub_gather(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ yaw,
                                                           const double *__restrict__ w,
                                                           const int32_t *__restrict__ cnt,
                                                           const int64_t *__restrict__ idx, int64_t k, SubGather out) {
    const int64_t j = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
    if (j >= k) return;
    const int64_t i = idx[j];                                  // in [0, n): k_sub_select
    if (out.x) out.x[j] = x[i];
    if (out.y) out.y[j] = y[i];
    if (out.yaw) out.yaw[j] = yaw[i];
    if (out.w) out.w[j] = w[i];
    if (out.cnt) out.cnt[j] = cnt[i];
}

}  // namespace

hipError_t launch_sub_scan(const double *w, int64_t n, int32_t e, SubScan sc, hipStream_t s) {
    const int64_t nb = post_blocks(n);
    hipLaunchKernelGGL(k_sub_totals, dim3((unsigned)nb), dim3(kPostBlock), 0, s, w, n, e, sc.tot);
    hipLaunchKernelGGL(k_sub_bases, dim3(1), dim3(kPostBlock), 0, s, sc.tot, nb, sc.base);
    hipLaunchKernelGGL(k_sub_rescan, dim3((unsigned)nb), dim3(kPostBlock), 0, s, w, n, e, sc.base, sc.C);
    return hipGetLastError();
}

hipError_t launch_sub_select(SubScan sc, int64_t n, uint64_t Q, int64_t k, uint32_t offset, int64_t *idx,
                             hipStream_t s) {
    const int64_t nb = post_blocks(n);
    const u64 *Qp = sc.C ? sc.base + nb : nullptr;
    hipLaunchKernelGGL(k_sub_select, dim3((unsigned)((k + kPostBlock - 1) / kPostBlock)), dim3(kPostBlock), 0, s, sc, n,
                       nb, Qp, (u64)Q, k, offset, idx);
    return hipGetLastError();
}

hipError_t launch_sub_gather(const double *x, const double *y, const double *yaw, const double *w, const int32_t *cnt,
                             const int64_t *idx, int64_t k, SubGather out, hipStream_t s) {
    hipLaunchKernelGGL(k_sub_gather, dim3((unsigned)((k + kPostBlock - 1) / kPostBlock)), dim3(kPostBlock), 0, s, x, y,
                       yaw, w, cnt, idx, k, out);
    return hipGetLastError();
}

}  // namespace fs2
