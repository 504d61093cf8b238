// dec_to_f64.h -- a decimal token -> the correctly rounded float64 (Python's float(token)), or "ask the host": the number
// parse of the ASCII PLY reader (csrc/ply_text.hip), the same code on the device and in its host twin.  Integer arithmetic
// only: no floating-point operation takes part, so the two agree by construction.
//
//   token   [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?  or  [+-]?(nan|inf|infinity) in any letter case; anything else is flagged
//   w, q    the first 19 significant digits as a uint64 and the decimal exponent: the value is w * 10^q, or -- when non-zero
//           digits were dropped -- lies in (w, w + 1) * 10^q
//   P       floor(5^q normalised to 128 bits) (dec_pow5_table.h): 5^q lies in [P, P + 1) * 2^e5, and is P * 2^e5 for 0 <= q <= 55
//   L, H    w * P and (w or w + 1) * (P or P + 1), 192-bit products: the value lies in [L, H] * 2^(e5 + q)
// Both ends are rounded to 53 bits, to nearest even.  Rounding is monotone, so when they agree that is the value's rounding.
// When they differ (a rounding boundary lies between them), when the result would be a subnormal double, or when the token is
// not of the grammar, the token is flagged and the host decides (float(), or the refusal).  w = 0 is +-0; q > 308 with w > 0
// is +-inf (10^309 > DBL_MAX); q < -342 is +-0 (w * 10^q < 10^19 * 10^-343 = 10^-324, below half the smallest subnormal).
#pragma once
#include <cstdint>

#include "dec_pow5_table.h"

#if defined(__HIPCC__)
#define GSX_DEC_HD __host__ __device__
#else
#define GSX_DEC_HD
#endif

namespace gsx {

constexpr int DEC_OK = 0, DEC_FLAG = 1;
constexpr int DEC_ROWS = GSX_DEC_QMAX - GSX_DEC_QMIN + 1;

static const uint64_t dec_pow5_host[DEC_ROWS][2] = {GSX_DEC_POW5_ROWS};
#if defined(__HIPCC__)
static __device__ const uint64_t dec_pow5_dev[DEC_ROWS][2] = {GSX_DEC_POW5_ROWS};
#endif

// floor(log2 5^q) - 127 for GSX_DEC_QMIN <= q <= GSX_DEC_QMAX (an arithmetic shift: q may be negative)
GSX_DEC_HD inline int dec_pow5_exp(int q) { return (int)(((int64_t)152170 * q) >> 16) - 127; }

GSX_DEC_HD inline void dec_pow5(int q, uint64_t &hi, uint64_t &lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    hi = dec_pow5_dev[q - GSX_DEC_QMIN][0];
    lo = dec_pow5_dev[q - GSX_DEC_QMIN][1];
#else
    hi = dec_pow5_host[q - GSX_DEC_QMIN][0];
    lo = dec_pow5_host[q - GSX_DEC_QMIN][1];
#endif
}

// a * b -> hi : lo, from 32-bit pieces (the same code on both sides)
GSX_DEC_HD inline void dec_mul64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo)
{
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
    lo = (p00 & 0xffffffffu) | (mid << 32);
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// w * (hi : lo) -> x2 : x1 : x0
GSX_DEC_HD inline void dec_mul192(uint64_t w, uint64_t hi, uint64_t lo, uint64_t &x2, uint64_t &x1, uint64_t &x0)
{
    uint64_t p0h, p1h, p1l;
    dec_mul64(w, lo, p0h, x0);
    dec_mul64(w, hi, p1h, p1l);
    x1 = p0h + p1l;
    x2 = p1h + (x1 < p0h ? 1u : 0u);
}

// (x2 : x1 : x0) * 2^e, at least 2^127 -> the float64 bits of its rounding to nearest even (overflow: infinity), or DEC_FLAG for
// a result below the smallest normal double
GSX_DEC_HD inline int dec_round192(uint64_t x2, uint64_t x1, uint64_t x0, int e, uint64_t *bits)
{
    if (x2 == 0) {
        x2 = x1;
        x1 = x0;
        x0 = 0;
        e -= 64;
    }
    const int lz = __builtin_clzll(x2);
    if (lz) {
        x2 = (x2 << lz) | (x1 >> (64 - lz));
        x1 = (x1 << lz) | (x0 >> (64 - lz));
        x0 <<= lz;
        e -= lz;
    }
    uint64_t mant = x2 >> 11;
    const uint64_t half = (x2 >> 10) & 1u, sticky = (x2 & 0x3ffu) | x1 | x0;
    if (half && (sticky || (mant & 1u))) ++mant;
    int ue = e + 191;
    if (mant >> 53) {
        mant >>= 1;
        ++ue;
    }
    if (ue > 1023) {
        *bits = 0x7ff0000000000000ull;
        return DEC_OK;
    }
    if (ue < -1022) return DEC_FLAG;
    *bits = ((uint64_t)(ue + 1023) << 52) | (mant & 0x000fffffffffffffull);
    return DEC_OK;
}

// w * 10^q (truncated: some value in (w, w + 1) * 10^q), w > 0, GSX_DEC_QMIN <= q <= GSX_DEC_QMAX -> the magnitude's bits
GSX_DEC_HD inline int dec_certify(uint64_t w, bool truncated, int q, uint64_t *bits)
{
    uint64_t mh, ml, l2, l1, l0;
    dec_pow5(q, mh, ml);
    const bool exact = q >= 0 && q <= GSX_DEC_EXACT_QMAX;
    const int e = dec_pow5_exp(q) + q;
    dec_mul192(w, mh, ml, l2, l1, l0);
    uint64_t lo_bits;
    if (dec_round192(l2, l1, l0, e, &lo_bits) != DEC_OK) return DEC_FLAG;
    if (exact && !truncated) {
        *bits = lo_bits;
        return DEC_OK;
    }
    const uint64_t wh = w + (truncated ? 1u : 0u);
    uint64_t h2, h1, h0;
    dec_mul192(wh, mh, ml, h2, h1, h0);
    if (!exact) {   // + wh * 1: the upper end of P's interval
        const uint64_t s0 = h0 + wh;
        const uint64_t c0 = s0 < h0 ? 1u : 0u;
        h0 = s0;
        const uint64_t s1 = h1 + c0;
        h2 += s1 < h1 ? 1u : 0u;
        h1 = s1;
    }
    uint64_t hi_bits;
    if (dec_round192(h2, h1, h0, e, &hi_bits) != DEC_OK || hi_bits != lo_bits) return DEC_FLAG;
    *bits = lo_bits;
    return DEC_OK;
}

GSX_DEC_HD inline bool dec_digit(unsigned c) { return c - (unsigned)'0' < 10u; }

// the n bytes byte(0) ... byte(n - 1) of a float token -> *bits (DEC_OK), or DEC_FLAG
template <class B>
GSX_DEC_HD inline int dec_to_f64(const B &byte, int n, uint64_t *bits)
{
    int i = 0;
    uint64_t sign = 0;
    if (n < 1) return DEC_FLAG;
    unsigned c = byte(0);
    if (c == '+' || c == '-') {
        sign = c == '-' ? 0x8000000000000000ull : 0;
        i = 1;
        if (n < 2) return DEC_FLAG;
    }
    c = byte(i) | 0x20u;
    if (c == 'n' || c == 'i') {
        const int len = n - i;
        const uint64_t word = c == 'n' ? 0x6e616eull : 0x7974696e69666e69ull;   // "nan" / "infinity", first letter lowest
        if (!(c == 'n' ? len == 3 : (len == 3 || len == 8))) return DEC_FLAG;
        for (int k = 0; k < len; ++k)
            if ((byte(i + k) | 0x20u) != ((word >> (8 * k)) & 0xffu)) return DEC_FLAG;
        *bits = sign | (c == 'n' ? 0x7ff8000000000000ull : 0x7ff0000000000000ull);
        return DEC_OK;
    }
    uint64_t w = 0;
    int nd = 0, dropped = 0, frac = 0;
    bool truncated = false, any = false;
    for (; i < n && dec_digit(c = byte(i)); ++i) {
        const unsigned d = c - '0';
        any = true;
        if (nd < 19) {
            if (w != 0 || d != 0) {
                w = w * 10 + d;
                ++nd;
            }
        } else {
            ++dropped;
            truncated |= d != 0;
        }
    }
    if (i < n && byte(i) == '.') {
        for (++i; i < n && dec_digit(c = byte(i)); ++i) {
            const unsigned d = c - '0';
            any = true;
            if (nd < 19) {
                if (w != 0 || d != 0) {
                    w = w * 10 + d;
                    ++nd;
                }
                ++frac;
            } else {
                truncated |= d != 0;
            }
        }
    }
    if (!any) return DEC_FLAG;
    int e10 = 0;
    if (i < n && (byte(i) | 0x20u) == 'e') {
        bool eneg = false;
        ++i;
        if (i < n && (byte(i) == '+' || byte(i) == '-')) eneg = byte(i++) == '-';
        if (i >= n || !dec_digit(byte(i))) return DEC_FLAG;
        for (; i < n && dec_digit(c = byte(i)); ++i)
            if (e10 < 100000000) e10 = e10 * 10 + (int)(c - '0');
        if (eneg) e10 = -e10;
    }
    if (i != n) return DEC_FLAG;
    if (w == 0) {
        *bits = sign;
        return DEC_OK;
    }
    const int q = e10 + dropped - frac;
    if (q > GSX_DEC_QMAX) {
        *bits = sign | 0x7ff0000000000000ull;
        return DEC_OK;
    }
    if (q < GSX_DEC_QMIN) {
        *bits = sign;
        return DEC_OK;
    }
    uint64_t mag;
    if (dec_certify(w, truncated, q, &mag) != DEC_OK) return DEC_FLAG;
    *bits = sign | mag;
    return DEC_OK;
}

// the n bytes of an integer token [+-]?D+ whose value lies in [lo, hi] -> *value (DEC_OK), or DEC_FLAG
template <class B>
GSX_DEC_HD inline int dec_to_int(const B &byte, int n, int64_t lo, int64_t hi, int64_t *value)
{
    int i = 0;
    bool neg = false;
    if (n < 1) return DEC_FLAG;
    unsigned c = byte(0);
    if (c == '+' || c == '-') {
        neg = c == '-';
        i = 1;
    }
    if (i >= n) return DEC_FLAG;
    int64_t v = 0;
    for (; i < n; ++i) {
        c = byte(i);
        if (!dec_digit(c)) return DEC_FLAG;
        if (v < ((int64_t)1 << 40)) v = v * 10 + (int64_t)(c - '0');
    }
    if (neg) v = -v;
    if (v < lo || v > hi) return DEC_FLAG;
    *value = v;
    return DEC_OK;
}

}  // namespace gsx
