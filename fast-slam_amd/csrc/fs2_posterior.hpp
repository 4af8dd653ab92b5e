// fs2_posterior.hpp -- what the host entry points and the kernels of the posterior
// readout share (fs2_posterior.hip; fs2.h fs2_pose_moments / fs2_pose_density;
// DESIGN.md §14): the reduction shapes, the layout of the partials, the weight
// quantisation of the density grid and the launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace fs2 {

// ---- reduction shape: a function of n alone ----
// A first-stage workgroup of kPostBlock threads reduces kPostChunk consecutive
// particles: lane t takes particles t, t + kPostBlock, ... of the chunk (strided
// per-lane partials), the waves reduce on DPP, the workgroup's four wave results
// are added in wave order and stored as column b of part[k][nb].  One second-stage
// workgroup folds the nb columns the same way.
constexpr int kPostBlock = 256;
constexpr int kPostPer = 8;
constexpr int kPostChunk = kPostBlock * kPostPer;
inline int64_t post_blocks(int64_t n) { return (n + kPostChunk - 1) / kPostChunk; }

// Rows of the partials: sums first, then minima, then maxima.
// first pass of the moments (about the pivot: particle 0's pose)
enum {
    kPmW = 0, kPmW2, kPmSx, kPmSy, kPmSs, kPmSc, kPmBad,       // sums
    kPmMinX, kPmMinY,                                          // minima
    kPmMaxX, kPmMaxY, kPmWmax,                                 // maxima
    kPmRows
};
constexpr int kPmSums = 7, kPmMins = 2;
// second pass (about the mean)
enum { kPcXX = 0, kPcXY, kPcXT, kPcYY, kPcYT, kPcTT, kPcRows };
// the density's weight pass
enum { kPwBad = 0, kPwWmax, kPwRows };
constexpr int kPostRowsMax = kPmRows;

// d into [-pi, pi): d - 2 pi floor((d + pi) / (2 pi)), exactly d when the floor is 0
// (the second pass's yaw deviation and the host's mean_yaw; the tests restate it).
__host__ __device__ inline double wrap_pi(double d) {
    const double two_pi = 6.283185307179586, pi = 3.141592653589793;
    return d - two_pi * floor((d + pi) / two_pi);
}

// ---- density grid ----
// A histogram workgroup of kPostBlock threads takes kPdChunk consecutive particles.
// kPdWindow 64-bit LDS counters (16 KiB): ten workgroups' windows fit a CU's 160 KiB,
// eight workgroups of four waves fill its 32 wave slots, so the window never limits
// occupancy.
constexpr int kPdPer = 4;
constexpr int kPdChunk = kPostBlock * kPdPer;
constexpr int kPdWindow = 2048;
constexpr int64_t kPdMaxCells = int64_t(1) << 24;

// The exponent e of the weighted amounts q = rint(w 2^e): wmax = m 2^ex with m in
// [0.5, 1) (frexp), e = B - ex, B = min(52, 62 - ceil(log2(max(n, 2)))).  Every
// q <= 2^B and n q <= 2^62.  e may exceed 1023 (a subnormal wmax: up to 1126): 2^e is
// then no double, but w 2^e < 2^B is, and ldexp(w, e) takes any int exponent, so
// nothing is clamped.  False when wmax is not a positive finite number or n < 1.
inline bool density_scale(double wmax, int64_t n, int32_t *e) {
    if (!(wmax > 0.0) || !std::isfinite(wmax) || n < 1) return false;
    int ex = 0;
    (void)std::frexp(wmax, &ex);
    const uint64_t m = (uint64_t)(n < 2 ? 2 : n) - 1;          // ceil(log2(v)) = bits of v - 1, v >= 2
    const int cl = 64 - __builtin_clzll(m);
    const int B = 62 - cl < 52 ? 62 - cl : 52;
    *e = (int32_t)(B - ex);
    return true;
}

// ---- launchers (fs2_posterior.hip); every buffer is the caller's ----
// part: [kPostRowsMax][post_blocks(n)] doubles; out: kPostRowsMax doubles.
// out[k] of launch_pose_first: the kPm* rows; then the pivot (x, y, yaw of particle 0)
// at out[kPmRows .. kPmRows + 3).
constexpr int kPostOut = kPmRows + 3;
hipError_t launch_pose_first(const double *x, const double *y, const double *yaw, const double *w, int64_t n,
                             int weighted, double *part, double *out, hipStream_t s);
hipError_t launch_pose_second(const double *x, const double *y, const double *yaw, const double *w, int64_t n,
                              int weighted, double mx, double my, double myaw, double *part, double *out,
                              hipStream_t s);
hipError_t launch_weight_scan(const double *w, int64_t n, double *part, double *out, hipStream_t s);
// grid: [ny][nx] counters followed by the outside counter, zeroed by the caller on s
hipError_t launch_pose_density(const double *x, const double *y, const double *w, int64_t n, int weighted,
                               double x0, double y0, double cell, int32_t nx, int32_t ny, int32_t e,
                               unsigned long long *grid, hipStream_t s);

}  // namespace fs2
