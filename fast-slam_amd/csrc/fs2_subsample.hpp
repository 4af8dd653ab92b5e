// fs2_subsample.hpp -- what the host entry points and the kernels of the weighted
// subsample share (fs2_subsample.hip; fs2.h fs2_subsample): the
// threshold arithmetic, the scan shape, the layout of the scratch and the launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs2_posterior.hpp"

namespace fs2 {

constexpr int64_t kSubMaxK = int64_t(1) << 30;
constexpr uint64_t kSubMaxTotal = uint64_t(1) << 62;

// Threshold t_j = floor((j Q + s) / k), s = floor(offset Q / 2^32), of output j of k over
// the total Q, for 1 <= Q <= 2^62, 1 <= k <= 2^30, 0 <= j < k, in 64 bits:
//   s   = offset (Q >> 32) + ((offset (Q & 0xffffffff)) >> 32)    (each product < 2^64; exact,
//         as offset (Q >> 32) 2^32 is a multiple of 2^32)
//   Q   = a k + b, s = a_s k + b_s (b, b_s < k)
//   t_j = j a + a_s + floor((j b + b_s) / k)                       (j b + b_s < k^2 <= 2^60)
// and t_j <= ((k - 1) Q + s) / k < Q because s < Q.  The kernel and
// fs2_subsample_threshold both call this and nothing else.
__host__ __device__ inline uint64_t sub_threshold(uint64_t Q, uint64_t k, uint32_t offset, uint64_t j) {
    const uint64_t s = (uint64_t)offset * (Q >> 32) + (((uint64_t)offset * (Q & 0xffffffffull)) >> 32);
    const uint64_t a = Q / k, b = Q - a * k;
    const uint64_t as = s / k, bs = s - as * k;
    return j * a + as + (j * b + bs) / k;
}

// ---- scan shape: a function of n alone ----
// Chunks of kPostChunk consecutive particles (the posterior readout's), one workgroup of
// kPostBlock threads each; in the rescan lane t takes the chunk's particles
// [t kPostPer, (t + 1) kPostPer).  One workgroup scans the chunk totals, kPostBlock a turn.
//
// Scratch of the scan, 8-byte words: base[nb + 1] (exclusive prefix of the chunk totals,
// base[nb] = Q), then tot[nb] (the chunk totals), then C[n] (the inclusive prefix).
inline size_t sub_scan_words(int64_t n) { return (size_t)(2 * post_blocks(n) + 1) + (size_t)n; }
struct SubScan {
    unsigned long long *base, *tot, *C;
};
inline SubScan sub_scan_views(unsigned long long *scr, int64_t n) {
    const int64_t nb = post_blocks(n);
    return SubScan{scr, scr + nb + 1, scr + 2 * nb + 1};
}

// ---- launchers (fs2_subsample.hip); every buffer is the caller's ----
// The inclusive prefix C of q_i = rint(w_i 2^e) and its chunk bases (three kernels).
hipError_t launch_sub_scan(const double *w, int64_t n, int32_t e, SubScan sc, hipStream_t s);
// idx[j] = the smallest i with C_i > t_j; sc.C == nullptr: q_i = 1 (idx[j] = t_j).
hipError_t launch_sub_select(SubScan sc, int64_t n, uint64_t Q, int64_t k, uint32_t offset, int64_t *idx,
                             hipStream_t s);
// out[j] = in[idx[j]] for the non-null outputs
struct SubGather {
    double *x, *y, *yaw, *w;
    int32_t *cnt;
};
hipError_t launch_sub_gather(const double *x, const double *y, const double *yaw, const double *w, const int32_t *cnt,
                             const int64_t *idx, int64_t k, SubGather out, hipStream_t s);

}  // namespace fs2
