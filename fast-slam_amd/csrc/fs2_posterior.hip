// fs2_posterior.hip -- the posterior readout on the device (fs2.h fs2_pose_moments,
// fs2_pose_density): weighted pose moments and a 2-D density grid of
// the particle cloud from the device-resident x / y / yaw / w.  Nothing here writes
// filter state.
//
// Moments.  Two passes, each a first stage of post_blocks(n) workgroups and one
// second-stage workgroup (fs2_posterior.hpp: the shape depends on n alone, no
// floating-point atomics, so the same state gives the same bits):
//   k_pose_first   W, sum w^2, the first moments about the pivot (particle 0's pose:
//                  sum w (x - x_p), sum w (y - y_p), sum w sin / cos (yaw - yaw_p)),
//                  the bounding box, the largest weight and the count of invalid ones;
//   k_pose_second  the six second moments about the mean the host formed from the
//                  first pass (never raw second moments: they cancel for a tight
//                  cloud far from the origin).
// Sums about the pivot are the sums of the definition shifted by an exact constant;
// a cloud of one particle gets its own pose as the mean and a covariance of exactly 0.
//
// Density.  k_pose_density: integer amounts (1, or rint(w 2^e)) added to 64-bit
// counters, exact and independent of order.  A workgroup reduces the cell box of its
// kPdChunk particles; a box of at most kPdWindow cells is accumulated in LDS (integer
// LDS atomics) and only its nonzero counters go to memory, one global integer atomic
// each; a larger box is added to memory lane by lane.
#include <hip/hip_runtime.h>

#include "fs2_posterior.hpp"
#include "fs2_reduce.hpp"

namespace fs2 {

namespace {

__device__ __forceinline__ double wave_min_d(double v) {
    return lane63(dpp_scan(v, (double)INFINITY, [](double a, double b) { return fmin(a, b); }));
}
__device__ __forceinline__ double wave_max_d(double v) {
    return lane63(dpp_scan(v, -(double)INFINITY, [](double a, double b) { return fmax(a, b); }));
}
__device__ __forceinline__ int wave_min_i(int v) {
    return lane63(dpp_scan(v, INT_MAX, [](int a, int b) { return min(a, b); }));
}

// rows [0, NSUM) are sums, [NSUM, NSUM + NMIN) minima, the rest maxima
template <int NSUM, int NMIN>
__device__ __forceinline__ double post_identity(int r) {
    return r < NSUM ? 0.0 : (r < NSUM + NMIN ? (double)INFINITY : -(double)INFINITY);
}
template <int NSUM, int NMIN>
__device__ __forceinline__ double post_combine(int r, double a, double b) {
    return r < NSUM ? a + b : (r < NSUM + NMIN ? fmin(a, b) : fmax(a, b));
}

// The workgroup's reduction of each lane's v[ROWS] (waves on DPP, then the four wave
// results in wave order), row r stored to dst[r * stride].  Every thread calls it.
template <int ROWS, int NSUM, int NMIN>
__device__ __forceinline__ void post_block_store(const double (&v)[ROWS], double *dst, int64_t stride) {
    __shared__ double s_p[kPostBlock / 64][ROWS];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const double t = r < NSUM ? wave_sum(v[r]) : (r < NSUM + NMIN ? wave_min_d(v[r]) : wave_max_d(v[r]));
        if (lane == 0) s_p[wid][r] = t;
    }
    __syncthreads();
    if (threadIdx.x < ROWS) {
        const int r = threadIdx.x;
        double t = s_p[0][r];
#pragma unroll
        for (int q = 1; q < kPostBlock / 64; ++q) t = post_combine<NSUM, NMIN>(r, t, s_p[q][r]);
        dst[(int64_t)r * stride] = t;
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kPostBlock) void k_pose_first(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ yaw,
                                                           const double *__restrict__ w, int64_t n,
                                                           double *__restrict__ part, int64_t nb) {
    const double px = x[0], py = y[0], pt = yaw[0];
    double v[kPmRows];
#pragma unroll
    for (int r = 0; r < kPmRows; ++r) v[r] = post_identity<kPmSums, kPmMins>(r);
    const int64_t base = (int64_t)blockIdx.x * kPostChunk + threadIdx.x;
#pragma unroll 2
    for (int k = 0; k < kPostPer; ++k) {
        const int64_t i = base + (int64_t)k * kPostBlock;
        if (i >= n) break;
        const double wi = WEIGHTED ? w[i] : 1.0;
        const double xi = x[i], yi = y[i];
        double sn, cs;
        sincos(yaw[i] - pt, &sn, &cs);
        v[kPmW] += wi;
        v[kPmW2] += wi * wi;
        v[kPmSx] += wi * (xi - px);
        v[kPmSy] += wi * (yi - py);
        v[kPmSs] += wi * sn;
        v[kPmSc] += wi * cs;
        v[kPmBad] += (wi >= 0.0 && wi < (double)INFINITY) ? 0.0 : 1.0;
        v[kPmMinX] = fmin(v[kPmMinX], xi);
        v[kPmMinY] = fmin(v[kPmMinY], yi);
        v[kPmMaxX] = fmax(v[kPmMaxX], xi);
        v[kPmMaxY] = fmax(v[kPmMaxY], yi);
        v[kPmWmax] = fmax(v[kPmWmax], wi);
    }
    post_block_store<kPmRows, kPmSums, kPmMins>(v, part + blockIdx.x, nb);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kPostBlock) void k_pose_second(const double *__restrict__ x, const double *__restrict__ y,
                                                            const double *__restrict__ yaw,
                                                            const double *__restrict__ w, int64_t n, double mx,
                                                            double my, double myaw, double *__restrict__ part,
                                                            int64_t nb) {
    double v[kPcRows] = {};
    const int64_t base = (int64_t)blockIdx.x * kPostChunk + threadIdx.x;
#pragma unroll 2
    for (int k = 0; k < kPostPer; ++k) {
        const int64_t i = base + (int64_t)k * kPostBlock;
        if (i >= n) break;
        const double wi = WEIGHTED ? w[i] : 1.0;
        const double dx = x[i] - mx, dy = y[i] - my, dt = wrap_pi(yaw[i] - myaw);
        const double wx = wi * dx, wy = wi * dy;
        v[kPcXX] += wx * dx;
        v[kPcXY] += wx * dy;
        v[kPcXT] += wx * dt;
        v[kPcYY] += wy * dy;
        v[kPcYT] += wy * dt;
        v[kPcTT] += (wi * dt) * dt;
    }
    post_block_store<kPcRows, kPcRows, 0>(v, part + blockIdx.x, nb);
}

__global__ __launch_bounds__(kPostBlock) void k_weight_scan(const double *__restrict__ w, int64_t n,
                                                            double *__restrict__ part, int64_t nb) {
    double v[kPwRows] = {0.0, -(double)INFINITY};
    const int64_t base = (int64_t)blockIdx.x * kPostChunk + threadIdx.x;
#pragma unroll 2
    for (int k = 0; k < kPostPer; ++k) {
        const int64_t i = base + (int64_t)k * kPostBlock;
        if (i >= n) break;
        const double wi = w[i];
        v[kPwBad] += (wi >= 0.0 && wi < (double)INFINITY) ? 0.0 : 1.0;
        v[kPwWmax] = fmax(v[kPwWmax], wi);
    }
    post_block_store<kPwRows, 1, 0>(v, part + blockIdx.x, nb);
}

// Second stage: the nb columns of part[ROWS][nb] into out[ROWS] (one workgroup; lane t
// takes columns t, t + kPostBlock, ...).  pivot: particle 0's pose after the rows.
template <int ROWS, int NSUM, int NMIN>
__global__ __launch_bounds__(kPostBlock) void k_post_fold(const double *__restrict__ part, int64_t nb,
                                                          double *__restrict__ out, const double *__restrict__ x,
                                                          const double *__restrict__ y,
                                                          const double *__restrict__ yaw) {
    double v[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = post_identity<NSUM, NMIN>(r);
    for (int64_t b = threadIdx.x; b < nb; b += kPostBlock) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) v[r] = post_combine<NSUM, NMIN>(r, v[r], part[(int64_t)r * nb + b]);
    }
    post_block_store<ROWS, NSUM, NMIN>(v, out, 1);
    if (x && threadIdx.x == 0) {
        out[ROWS] = x[0];
        out[ROWS + 1] = y[0];
        out[ROWS + 2] = yaw[0];
    }
}

// ------------------------------------------------------------- density grid ---

template <bool WEIGHTED>
__global__ __launch_bounds__(kPostBlock) void k_pose_density(const double *__restrict__ x, const double *__restrict__ y,
                                                             const double *__restrict__ w, int64_t n, double x0,
                                                             double y0, double cell, int32_t nx, int32_t ny,
                                                             int32_t e, unsigned long long *__restrict__ grid) {
    __shared__ unsigned long long s_win[kPdWindow];
    __shared__ int s_box[kPostBlock / 64][4];
    __shared__ unsigned long long s_out[kPostBlock / 64];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kPdChunk + threadIdx.x;
    int ix[kPdPer], iy[kPdPer];
    unsigned long long q[kPdPer];
    // the box as minima: (x lo, y lo, -x hi, -y hi); an empty box keeps INT_MAX
    int bx0 = INT_MAX, by0 = INT_MAX, nbx1 = INT_MAX, nby1 = INT_MAX;
    unsigned long long out = 0;
#pragma unroll
    for (int k = 0; k < kPdPer; ++k) {
        const int64_t i = base + (int64_t)k * kPostBlock;
        ix[k] = -1;
        iy[k] = -1;
        q[k] = 0;
        if (i < n) {
            q[k] = WEIGHTED ? (unsigned long long)rint(ldexp(w[i], e)) : 1ull;
            const double fx = floor((x[i] - x0) / cell), fy = floor((y[i] - y0) / cell);
            if (fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny) {      // (false for NaN)
                ix[k] = (int)fx;
                iy[k] = (int)fy;
                bx0 = min(bx0, ix[k]);
                by0 = min(by0, iy[k]);
                nbx1 = min(nbx1, -ix[k]);
                nby1 = min(nby1, -iy[k]);
            } else {
                out += q[k];
                q[k] = 0;
            }
        }
    }
    bx0 = wave_min_i(bx0);
    by0 = wave_min_i(by0);
    nbx1 = wave_min_i(nbx1);
    nby1 = wave_min_i(nby1);
    out = wave_sum_u64(out);
    if (lane == 0) {
        s_box[wid][0] = bx0;
        s_box[wid][1] = by0;
        s_box[wid][2] = nbx1;
        s_box[wid][3] = nby1;
        s_out[wid] = out;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPostBlock / 64; ++u) {
        bx0 = min(bx0, s_box[u][0]);
        by0 = min(by0, s_box[u][1]);
        nbx1 = min(nbx1, s_box[u][2]);
        nby1 = min(nby1, s_box[u][3]);
    }
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int u = 0; u < kPostBlock / 64; ++u) t += s_out[u];
        if (t) atomicAdd(grid + (int64_t)nx * ny, t);          // the outside counter
    }
    if (bx0 == INT_MAX) return;                                // no particle of this workgroup in the grid
    const int bw = -nbx1 - bx0 + 1, bh = -nby1 - by0 + 1;      // 1 <= bw <= nx, 1 <= bh <= ny
    const int64_t cells = (int64_t)bw * bh;
    if (cells <= kPdWindow) {
        for (int c = threadIdx.x; c < (int)cells; c += kPostBlock) s_win[c] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPdPer; ++k) {
            // bx0 <= ix <= bx0 + bw - 1 and likewise in y: c lies in [0, cells)
            const int c = ix[k] >= 0 ? (iy[k] - by0) * bw + (ix[k] - bx0) : -1;
            // a wave whose lanes all name one cell (a cloud tighter than a cell) adds once
            const int c0 = __builtin_amdgcn_readfirstlane(c);
            if (__all(c == c0)) {
                const unsigned long long t = wave_sum_u64(q[k]);
                if (lane == 0 && c0 >= 0 && t) atomicAdd(&s_win[c0], t);
            } else if (c >= 0 && q[k]) {
                atomicAdd(&s_win[c], q[k]);
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < (int)cells; c += kPostBlock) {
            const unsigned long long t = s_win[c];
            if (t) atomicAdd(grid + (int64_t)(by0 + c / bw) * nx + (bx0 + c % bw), t);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPdPer; ++k)
            if (ix[k] >= 0 && q[k]) atomicAdd(grid + (int64_t)iy[k] * nx + ix[k], q[k]);   // ix < nx, iy < ny
    }
}

}  // namespace

hipError_t launch_pose_first(const double *x, const double *y, const double *yaw, const double *w, int64_t n,
                             int weighted, double *part, double *out, hipStream_t s) {
    const int64_t nb = post_blocks(n);
    if (weighted)
        hipLaunchKernelGGL(k_pose_first<true>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, yaw, w, n, part, nb);
    else
        hipLaunchKernelGGL(k_pose_first<false>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, yaw, w, n, part, nb);
    hipLaunchKernelGGL((k_post_fold<kPmRows, kPmSums, kPmMins>), dim3(1), dim3(kPostBlock), 0, s, part, nb, out, x, y,
                       yaw);
    return hipGetLastError();
}

hipError_t launch_pose_second(const double *x, const double *y, const double *yaw, const double *w, int64_t n,
                              int weighted, double mx, double my, double myaw, double *part, double *out,
                              hipStream_t s) {
    const int64_t nb = post_blocks(n);
    if (weighted)
        hipLaunchKernelGGL(k_pose_second<true>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, yaw, w, n, mx, my,
                           myaw, part, nb);
    else
        hipLaunchKernelGGL(k_pose_second<false>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, yaw, w, n, mx, my,
                           myaw, part, nb);
    const double *none = nullptr;
    hipLaunchKernelGGL((k_post_fold<kPcRows, kPcRows, 0>), dim3(1), dim3(kPostBlock), 0, s, part, nb, out, none, none,
                       none);
    return hipGetLastError();
}

hipError_t launch_weight_scan(const double *w, int64_t n, double *part, double *out, hipStream_t s) {
    const int64_t nb = post_blocks(n);
    hipLaunchKernelGGL(k_weight_scan, dim3((unsigned)nb), dim3(kPostBlock), 0, s, w, n, part, nb);
    const double *none = nullptr;
    hipLaunchKernelGGL((k_post_fold<kPwRows, 1, 0>), dim3(1), dim3(kPostBlock), 0, s, part, nb, out, none, none, none);
    return hipGetLastError();
}

hipError_t launch_pose_density(const double *x, const double *y, const double *w, int64_t n, int weighted,
                               double x0, double y0, double cell, int32_t nx, int32_t ny, int32_t e,
                               unsigned long long *grid, hipStream_t s) {
    const int64_t nb = (n + kPdChunk - 1) / kPdChunk;
    if (weighted)
        hipLaunchKernelGGL(k_pose_density<true>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, w, n, x0, y0, cell,
                           nx, ny, e, grid);
    else
        hipLaunchKernelGGL(k_pose_density<false>, dim3((unsigned)nb), dim3(kPostBlock), 0, s, x, y, w, n, x0, y0, cell,
                           nx, ny, e, grid);
    return hipGetLastError();
}

}  // namespace fs2
