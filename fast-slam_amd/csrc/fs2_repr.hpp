// fs2_repr.hpp -- CPython's float.__repr__ (as json.dumps spells a float) as
// host/device arithmetic, for the viewer JSON's particle block
// (fast_slam_2/utils/serializer.py:39 of the reference: json.dump(..., indent=4)
// formats every pose coordinate with float.__repr__):
//   finite v: the shortest decimal digit string that reads back to v, the closest
//     to v among those of that length, an exact tie to the even digit; printed
//     d[.ddd]e±XX when the first digit's decimal exponent is < -4 or >= 16, else
//     positionally, with ".0" appended where no '.' would appear;
//   NaN (any sign, any payload) -> NaN, ±inf -> Infinity / -Infinity (json.dumps).
// The digits come from Ryu (Adams, "Ryu: fast float-to-string conversion", PLDI
// 2018): v's rounding interval [vm, vp] and v itself are scaled by a power of ten
// with one 64 x 128-bit multiplication by a tabulated 125-bit power of five (or of
// its reciprocal), then digits are removed while the interval still holds a shorter
// number.  The interval's lower half is narrower at a power of two (mm_shift), its
// ends belong to it when the mantissa is even (strtod rounds half to even).  The
// table (668 x 128 bit) is computed at start-up from 5^i in exact integer
// arithmetic (repr_build_table); the device reads its copy from global memory.
// The longest text is 24 bytes (-2.2250738585072014e-308).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace fs2 {

constexpr int kReprMax = 24;                 // longest text
constexpr int kReprInv = 342, kReprPow = 326;   // 5^-q for q < 342, 5^i for i < 326
constexpr int kReprTabWords = 2 * (kReprInv + kReprPow);   // uint64 words: (lo, hi) pairs
constexpr int kReprBits = 125;

// ---- the table, on the host: exact integers of up to 1024 bits ----
struct ReprBig {
    uint32_t w[32];
};
inline int repr_big_bits(const ReprBig &a) {
    for (int k = 31; k >= 0; --k)
        if (a.w[k]) {
            int b = 32;
            while (!(a.w[k] >> (b - 1))) --b;
            return 32 * k + b;
        }
    return 0;
}
inline void repr_big_mul_small(ReprBig &a, uint32_t m) {
    uint64_t c = 0;
    for (int k = 0; k < 32; ++k) {
        c += (uint64_t)a.w[k] * m;
        a.w[k] = (uint32_t)c;
        c >>= 32;
    }
}
inline void repr_big_shl1(ReprBig &a) {
    uint32_t c = 0;
    for (int k = 0; k < 32; ++k) {
        const uint32_t n = a.w[k] >> 31;
        a.w[k] = (a.w[k] << 1) | c;
        c = n;
    }
}
inline bool repr_big_ge(const ReprBig &a, const ReprBig &b) {
    for (int k = 31; k >= 0; --k)
        if (a.w[k] != b.w[k]) return a.w[k] > b.w[k];
    return true;
}
inline void repr_big_sub(ReprBig &a, const ReprBig &b) {
    uint64_t br = 0;
    for (int k = 0; k < 32; ++k) {
        const uint64_t d = (uint64_t)a.w[k] - b.w[k] - br;
        a.w[k] = (uint32_t)d;
        br = (d >> 32) & 1;
    }
}
// bits [lo, lo + 128) of a (lo may be negative: zeros below bit 0)
inline void repr_big_window(const ReprBig &a, int lo, uint64_t out[2]) {
    out[0] = out[1] = 0;
    for (int b = 0; b < 128; ++b) {
        const int s = lo + b;
        if (s < 0 || s >= 1024) continue;
        if ((a.w[s >> 5] >> (s & 31)) & 1u) out[b >> 6] |= 1ull << (b & 63);
    }
}
// tab[2 q], tab[2 q + 1]: floor(2^(bits(5^q) - 1 + 125) / 5^q) + 1, q < kReprInv;
// tab[2 (kReprInv + i)], ...: the top 125 bits of 5^i, i < kReprPow.
inline void repr_build_table(uint64_t *tab) {
    ReprBig p{};
    p.w[0] = 1;
    for (int i = 0; i < kReprInv; ++i) {
        const int bits = repr_big_bits(p);
        if (i < kReprPow) repr_big_window(p, bits - kReprBits, tab + 2 * (kReprInv + i));
        // long division of 2^(bits - 1) 2^125 by 5^i: the quotient has 126 bits at most
        uint64_t q[2] = {0, 0};
        if (i == 0) {
            q[1] = 1ull << (kReprBits - 64);
        } else {
            ReprBig r{};
            r.w[(bits - 1) >> 5] = 1u << ((bits - 1) & 31);      // < 5^i
            for (int s = 0; s < kReprBits; ++s) {
                repr_big_shl1(r);
                q[1] = (q[1] << 1) | (q[0] >> 63);
                q[0] <<= 1;
                if (repr_big_ge(r, p)) {
                    repr_big_sub(r, p);
                    q[0] |= 1;
                }
            }
        }
        q[0] += 1;
        if (q[0] == 0) q[1] += 1;
        tab[2 * i] = q[0];
        tab[2 * i + 1] = q[1];
        repr_big_mul_small(p, 5);
    }
}

// ---- digits ----
__host__ __device__ inline uint64_t repr_umulh(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// (m mul) >> j for a 128-bit mul = (mul[0], mul[1]), 64 < j < 128 + 64
__host__ __device__ inline uint64_t repr_mul_shift(uint64_t m, const uint64_t *mul, int j) {
    const uint64_t b0hi = repr_umulh(m, mul[0]);
    const uint64_t b2lo = m * mul[1], b2hi = repr_umulh(m, mul[1]);
    const uint64_t lo = b0hi + b2lo;
    const uint64_t hi = b2hi + (lo < b0hi ? 1u : 0u);
    const int s = j - 64;                            // 0 < s < 64 for every double
    return (hi << (64 - s)) | (lo >> s);
}
__host__ __device__ inline uint32_t repr_pow5_factor(uint64_t v) {
    uint32_t c = 0;
    while (v != 0 && v % 5 == 0) {
        v /= 5;
        ++c;
    }
    return c;
}
__host__ __device__ inline uint32_t repr_pow5bits(int32_t e) { return (uint32_t)(((e * 1217359) >> 19) + 1); }
__host__ __device__ inline uint32_t repr_log10_pow2(int32_t e) { return (uint32_t)((e * 78913) >> 18); }
__host__ __device__ inline uint32_t repr_log10_pow5(int32_t e) { return (uint32_t)((e * 732923) >> 20); }
__host__ __device__ inline int repr_declen(uint64_t v) {   // v < 10^17
    int n = 1;
    uint64_t p = 10;
    while (n < 17 && v >= p) {
        p *= 10;
        ++n;
    }
    return n;
}

// What is printed: kind 0 finite and non-zero (digits x 10^exp, olen digits), 1 zero,
// 2 NaN, 3 infinity.
struct ReprDec {
    uint64_t digits;
    int32_t exp;
    int32_t olen;
    int32_t kind;
    bool neg;
};

__host__ __device__ inline ReprDec repr_decompose(double v, const uint64_t *tab) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    ReprDec d;
    d.neg = (bits >> 63) != 0;
    d.digits = 0;
    d.exp = 0;
    d.olen = 1;
    const uint64_t mant = bits & 0x000fffffffffffffull;
    const uint32_t bexp = (uint32_t)((bits >> 52) & 0x7ff);
    if (bexp == 0x7ff) {
        d.kind = mant ? 2 : 3;
        return d;
    }
    if (bexp == 0 && mant == 0) {
        d.kind = 1;
        return d;
    }
    d.kind = 0;
    int32_t e2;
    uint64_t m2;
    if (bexp == 0) {
        e2 = 1 - 1023 - 52 - 2;
        m2 = mant;
    } else {
        e2 = (int32_t)bexp - 1023 - 52 - 2;
        m2 = (1ull << 52) | mant;
    }
    const bool accept = (m2 & 1) == 0;               // the interval's ends read back to v
    const uint64_t mv = 4 * m2;
    const uint32_t mm_shift = (mant != 0 || bexp <= 1) ? 1 : 0;   // 0 at a power of two: the lower half-gap is half as wide
    uint64_t vr, vp, vm;
    int32_t e10;
    bool vm_tz = false, vr_tz = false;               // the removed digits of vm / vr are all zero
    if (e2 >= 0) {
        const uint32_t q = repr_log10_pow2(e2) - (e2 > 3);
        e10 = (int32_t)q;
        const int32_t k = kReprBits + (int32_t)repr_pow5bits((int32_t)q) - 1;
        const int32_t j = -e2 + (int32_t)q + k;
        const uint64_t *mul = tab + 2 * q;
        vr = repr_mul_shift(mv, mul, j);
        vp = repr_mul_shift(mv + 2, mul, j);
        vm = repr_mul_shift(mv - 1 - mm_shift, mul, j);
        if (q <= 21) {
            if (mv % 5 == 0) vr_tz = repr_pow5_factor(mv) >= q;
            else if (accept) vm_tz = repr_pow5_factor(mv - 1 - mm_shift) >= q;
            else vp -= repr_pow5_factor(mv + 2) >= q ? 1 : 0;
        }
    } else {
        const uint32_t q = repr_log10_pow5(-e2) - (-e2 > 1);
        e10 = (int32_t)q + e2;
        const int32_t i = -e2 - (int32_t)q;
        const int32_t k = (int32_t)repr_pow5bits(i) - kReprBits;
        const int32_t j = (int32_t)q - k;
        const uint64_t *mul = tab + 2 * (kReprInv + i);
        vr = repr_mul_shift(mv, mul, j);
        vp = repr_mul_shift(mv + 2, mul, j);
        vm = repr_mul_shift(mv - 1 - mm_shift, mul, j);
        if (q <= 1) {
            vr_tz = true;
            if (accept) vm_tz = mm_shift == 1;
            else --vp;
        } else if (q < 63) {
            vr_tz = (mv & ((1ull << q) - 1)) == 0;
        }
    }
    int32_t removed = 0;
    uint32_t last = 0;                               // the last digit removed from vr
    while (vp / 10 > vm / 10) {
        vm_tz &= vm % 10 == 0;
        vr_tz &= last == 0;
        last = (uint32_t)(vr % 10);
        vr /= 10;
        vp /= 10;
        vm /= 10;
        ++removed;
    }
    if (vm_tz) {
        while (vm % 10 == 0) {
            vr_tz &= last == 0;
            last = (uint32_t)(vr % 10);
            vr /= 10;
            vp /= 10;
            vm /= 10;
            ++removed;
        }
    }
    if (vr_tz && last == 5 && vr % 2 == 0) last = 4;   // exactly ...5000: to the even digit
    d.digits = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5) ? 1 : 0);
    d.exp = e10 + removed;
    d.olen = repr_declen(d.digits);
    return d;
}

// Bytes of the text of d.
__host__ __device__ inline int repr_length(const ReprDec &d) {
    if (d.kind == 1) return d.neg ? 4 : 3;
    if (d.kind == 2) return 3;
    if (d.kind == 3) return d.neg ? 9 : 8;
    const int E = d.exp + d.olen - 1;                // decimal exponent of the first digit
    int n = d.neg ? 1 : 0;
    if (E < -4 || E >= 16) {
        const int a = E < 0 ? -E : E;
        return n + d.olen + (d.olen > 1 ? 1 : 0) + 2 + (a >= 100 ? 3 : 2);
    }
    if (E < 0) return n + 2 + (-E - 1) + d.olen;     // 0.000ddd
    return n + (d.olen > E + 1 ? d.olen + 1 : E + 1 + 2);   // dd.ddd / dd000.0
}

// Writes the text of d at out (no terminator); returns its length (repr_length).
__host__ __device__ inline int repr_write(const ReprDec &d, char *out) {
    int n = 0;
    if (d.kind == 2) {
        out[0] = 'N';
        out[1] = 'a';
        out[2] = 'N';
        return 3;
    }
    if (d.neg) out[n++] = '-';
    if (d.kind == 1) {
        out[n] = '0';
        out[n + 1] = '.';
        out[n + 2] = '0';
        return n + 3;
    }
    if (d.kind == 3) {
        const char *s = "Infinity";
        for (int k = 0; k < 8; ++k) out[n + k] = s[k];
        return n + 8;
    }
    const int E = d.exp + d.olen - 1, L = d.olen;
    uint64_t v = d.digits;
    if (E < -4 || E >= 16) {
        // d[.ddd]e±XX
        char *p = out + n;
        const int body = L > 1 ? L + 1 : 1;
        for (int k = L - 1; k >= 1; --k) {
            p[k + 1] = (char)('0' + v % 10);
            v /= 10;
        }
        p[0] = (char)('0' + v);
        if (L > 1) p[1] = '.';
        n += body;
        out[n++] = 'e';
        out[n++] = E < 0 ? '-' : '+';
        const int a = E < 0 ? -E : E;
        if (a >= 100) out[n++] = (char)('0' + a / 100);
        out[n++] = (char)('0' + (a / 10) % 10);
        out[n++] = (char)('0' + a % 10);
        return n;
    }
    if (E < 0) {
        out[n++] = '0';
        out[n++] = '.';
        for (int k = 0; k < -E - 1; ++k) out[n++] = '0';
        for (int k = L - 1; k >= 0; --k) {
            out[n + k] = (char)('0' + v % 10);
            v /= 10;
        }
        return n + L;
    }
    if (L > E + 1) {
        // E + 1 digits, '.', the rest
        char *p = out + n;
        for (int k = L - 1; k >= 0; --k) {
            p[k <= E ? k : k + 1] = (char)('0' + v % 10);
            v /= 10;
        }
        p[E + 1] = '.';
        return n + L + 1;
    }
    for (int k = L - 1; k >= 0; --k) {
        out[n + k] = (char)('0' + v % 10);
        v /= 10;
    }
    n += L;
    for (int k = L; k < E + 1; ++k) out[n++] = '0';
    out[n++] = '.';
    out[n++] = '0';
    return n;
}

// json.dumps(v) at out (kReprMax bytes of room); returns the length.
__host__ __device__ inline int repr_double(double v, const uint64_t *tab, char *out) {
    return repr_write(repr_decompose(v, tab), out);
}

}  // namespace fs2
