// fs2_json.hip -- the viewer JSON's particle block on the device: the text of
//   json.dump([{"x": .., "y": .., "yaw": ..}, ...], indent=4)
// at a nesting depth (reference: fast_slam_2/utils/serializer.py:39), byte for
// byte, from the device-resident poses (digits: fs2_repr.hpp).
//
// Item i of the list is the byte string
//   ("[\n" if i == 0 else ",\n") i1 "{\n" i2 "\"x\": " X ",\n" i2 "\"y\": " Y ",\n" i2 "\"yaw\": " W "\n" i1 "}"
//   (+ "\n" i0 "]" after the last item),  i0 / i1 / i2 = 4 depth / 4 (depth + 1) / 4 (depth + 2) spaces,
// so the whole text is the concatenation of the items.  k_json_sizes sums each
// workgroup's item lengths, k_json_scan turns the sums into 64-bit offsets (the
// text passes 2 GiB at 1.6e7 particles), k_json_write computes the digits again
// (cheaper than a record round trip: 24 B read per particle against ~134 B
// written), assembles its workgroup's contiguous segment in LDS -- placed so that
// LDS byte k and global byte k agree modulo 16 -- and writes it out with aligned
// 16-byte stores per lane; the segment's unaligned head and tail (< 16 bytes each)
// go out as bytes.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "fs2_kernels.hpp"
#include "fs2_repr.hpp"

namespace fs2 {

namespace {

struct JsonFmt {
    int i0, i1, i2;      // indent bytes of the list's bracket, an item's braces, its members
    int fixed;           // bytes of an item without its numbers (separator included)
    int tail;            // bytes after the last item
};
__host__ __device__ inline JsonFmt json_fmt(int depth) {
    JsonFmt f;
    f.i0 = 4 * depth;
    f.i1 = f.i0 + 4;
    f.i2 = f.i0 + 8;
    f.fixed = 27 + 2 * f.i1 + 3 * f.i2;
    f.tail = 2 + f.i0;
    return f;
}

__device__ __forceinline__ int wave_incl_scan_i32(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// exclusive prefix of v over the kJsonBlock threads; *total: the workgroup's sum
__device__ __forceinline__ int json_block_scan(int v, int *wtot, int *total) {
    const int incl = wave_incl_scan_i32(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kJsonBlock / 64; ++w) {
        if (w < wave) base += wtot[w];
        tot += wtot[w];
    }
    *total = tot;
    return base + incl - v;
}

struct JsonItem {
    ReprDec x, y, w;
    int len;
};
__device__ __forceinline__ JsonItem json_item(const uint64_t *tab, const double *x, const double *y,
                                              const double *yaw, int64_t i, int64_t n, const JsonFmt &f) {
    JsonItem it;
    it.x = repr_decompose(x[i], tab);
    it.y = repr_decompose(y[i], tab);
    it.w = repr_decompose(yaw[i], tab);
    it.len = f.fixed + repr_length(it.x) + repr_length(it.y) + repr_length(it.w) + (i == n - 1 ? f.tail : 0);
    return it;
}

__global__ __launch_bounds__(kJsonBlock) void k_json_sizes(const uint64_t *__restrict__ tab,
                                                           const double *__restrict__ x,
                                                           const double *__restrict__ y,
                                                           const double *__restrict__ yaw, int64_t n, int depth,
                                                           int64_t *__restrict__ bsum) {
    __shared__ int wtot[kJsonBlock / 64];
    const JsonFmt f = json_fmt(depth);
    const int64_t i = (int64_t)blockIdx.x * kJsonBlock + threadIdx.x;
    const int len = i < n ? json_item(tab, x, y, yaw, i, n, f).len : 0;
    int total;
    (void)json_block_scan(len, wtot, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// b[k] <- b[0] + ... + b[k - 1], b[nb] <- the total; one workgroup of 1024.
__global__ __launch_bounds__(1024) void k_json_scan(int64_t *__restrict__ b, int64_t nb) {
    __shared__ long long wtot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t k = base + threadIdx.x;
        const long long v = k < nb ? (long long)b[k] : 0;
        long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        long long before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wtot[w];
            tot += wtot[w];
        }
        if (k < nb) b[k] = carry + before + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) b[nb] = carry;
}

__device__ __forceinline__ char *put(char *p, const char *s, int n) {
    for (int k = 0; k < n; ++k) p[k] = s[k];
    return p + n;
}

__global__ __launch_bounds__(kJsonBlock) void k_json_write(const uint64_t *__restrict__ tab,
                                                           const double *__restrict__ x,
                                                           const double *__restrict__ y,
                                                           const double *__restrict__ yaw, int64_t n, int depth,
                                                           const int64_t *__restrict__ boff, char *__restrict__ text) {
    extern __shared__ uint4 seg4[];                  // the segment, from the 16-byte line its first byte lies in
    __shared__ int wtot[kJsonBlock / 64];
    char *seg = reinterpret_cast<char *>(seg4);
    const JsonFmt f = json_fmt(depth);
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kJsonBlock + tid;
    JsonItem it;
    it.len = 0;
    if (i < n) it = json_item(tab, x, y, yaw, i, n, f);
    int total;
    const int off = json_block_scan(it.len, wtot, &total);
    const int64_t g0 = boff[blockIdx.x];             // the segment is text[g0, g0 + total)
    const int shift = (int)(g0 & 15);
    // the indents are most of the skeleton: fill with spaces, then write the rest
    const uint32_t sp = 0x20202020u;
    for (int k = tid; k < (shift + total + 15) / 16; k += kJsonBlock) seg4[k] = make_uint4(sp, sp, sp, sp);
    __syncthreads();
    if (i < n) {
        char *p = seg + shift + off;
        p = put(p, i == 0 ? "[\n" : ",\n", 2) + f.i1;
        p = put(p, "{\n", 2) + f.i2;
        p = put(p, "\"x\": ", 5);
        p += repr_write(it.x, p);
        p = put(p, ",\n", 2) + f.i2;
        p = put(p, "\"y\": ", 5);
        p += repr_write(it.y, p);
        p = put(p, ",\n", 2) + f.i2;
        p = put(p, "\"yaw\": ", 7);
        p += repr_write(it.w, p);
        p = put(p, "\n", 1) + f.i1;
        p = put(p, "}", 1);
        if (i == n - 1) {
            p = put(p, "\n", 1) + f.i0;
            p = put(p, "]", 1);
        }
    }
    __syncthreads();
    const int64_t g1 = g0 + total;
    const int64_t a0 = (g0 + 15) & ~(int64_t)15, a1 = g1 & ~(int64_t)15;   // the aligned body [a0, a1)
    if (a0 >= a1) {                                  // no whole line: bytes
        for (int k = tid; k < total; k += kJsonBlock) text[g0 + k] = seg[shift + k];
        return;
    }
    const int head = (int)(a0 - g0), tailb = (int)(g1 - a1);
    if (tid < head) text[g0 + tid] = seg[shift + tid];
    if (tid >= 64 && tid - 64 < tailb) text[a1 + (tid - 64)] = seg[(int)(a1 - (g0 - shift)) + (tid - 64)];
    uint4 *dst = reinterpret_cast<uint4 *>(text + a0);
    const int l0 = (int)((a0 - (g0 - shift)) >> 4), lines = (int)((a1 - a0) >> 4);
    for (int k = tid; k < lines; k += kJsonBlock) dst[k] = seg4[l0 + k];
}

__global__ __launch_bounds__(256) void k_repr_doubles(const uint64_t *__restrict__ tab, const double *__restrict__ v,
                                                      int64_t n, uint64_t *__restrict__ out,
                                                      uint8_t *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    char buf[kReprMax];
#pragma unroll
    for (int k = 0; k < kReprMax; ++k) buf[k] = 0;
    const int l = repr_double(v[i], tab, buf);
    uint64_t w[3];
    memcpy(w, buf, kReprMax);
    out[3 * i] = w[0];
    out[3 * i + 1] = w[1];
    out[3 * i + 2] = w[2];
    len[i] = (uint8_t)l;
}

}  // namespace

const uint64_t *json_host_table() {
    static const std::vector<uint64_t> tab = [] {
        std::vector<uint64_t> t(kReprTabWords);
        repr_build_table(t.data());
        return t;
    }();
    return tab.data();
}

hipError_t json_device_table(int device, const uint64_t **out) {
    static std::mutex mu;
    static uint64_t *dev[64] = {};
    if (device < 0 || device >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(mu);
    if (!dev[device]) {
        uint64_t *p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(uint64_t) * kReprTabWords);
        if (e != hipSuccess) return e;
        e = hipMemcpy(p, json_host_table(), sizeof(uint64_t) * kReprTabWords, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        dev[device] = p;
    }
    *out = dev[device];
    return hipSuccess;
}

int64_t json_max_bytes(int64_t n, int depth) {
    const JsonFmt f = json_fmt(depth);
    return n == 0 ? 2 : n * (int64_t)(f.fixed + 3 * kReprMax) + f.tail;
}

static size_t json_lds_bytes(int depth) {
    const JsonFmt f = json_fmt(depth);
    // the workgroup's items, the list's tail, the shift to the line (< 16) and the fill's rounding (< 16)
    return ((size_t)kJsonBlock * (size_t)(f.fixed + 3 * kReprMax) + (size_t)f.tail + 32 + 15) & ~(size_t)15;
}

hipError_t launch_json_sizes(const uint64_t *tab, const double *x, const double *y, const double *yaw, int64_t n,
                             int depth, int64_t *boff, hipStream_t s, hipEvent_t after_sizes) {
    const int64_t nb = (n + kJsonBlock - 1) / kJsonBlock;
    hipLaunchKernelGGL(k_json_sizes, dim3((unsigned)nb), dim3(kJsonBlock), 0, s, tab, x, y, yaw, n, depth, boff);
    if (after_sizes) (void)hipEventRecord(after_sizes, s);
    hipLaunchKernelGGL(k_json_scan, dim3(1), dim3(1024), 0, s, boff, nb);
    return hipGetLastError();
}

hipError_t launch_json_write(const uint64_t *tab, const double *x, const double *y, const double *yaw, int64_t n,
                             int depth, const int64_t *boff, char *text, hipStream_t s) {
    const int64_t nb = (n + kJsonBlock - 1) / kJsonBlock;
    hipLaunchKernelGGL(k_json_write, dim3((unsigned)nb), dim3(kJsonBlock), json_lds_bytes(depth), s, tab, x, y, yaw, n,
                       depth, boff, text);
    return hipGetLastError();
}

hipError_t launch_repr_doubles(const uint64_t *tab, const double *v, int64_t n, char *out, uint8_t *len,
                               hipStream_t s) {
    hipLaunchKernelGGL(k_repr_doubles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tab, v, n,
                       reinterpret_cast<uint64_t *>(out), len);
    return hipGetLastError();
}

}  // namespace fs2
