// np_exp.h -- numpy's float32 exp (the AVX512F / AVX2+FMA3 SIMD routine of numpy/_core/src/umath/loops_exponent_log), bit
// for bit, as __host__ __device__ code.
//
// numpy's float32 exp is not correctly rounded (about 39 % of results differ from the nearest float32 by up to 2 ulp), so a
// writer that stores its raw bits (the ksplat scales, csrc/ksplat.hip) must repeat numpy's own steps:
//   Cody-Waite reduction by ln 2 in two fused steps, a [5/2] rational approximation in Horner form with fused steps, one IEEE
//   division, and an exact scaling by 2^q.
// Inputs numpy masks out: NaN -> +qNaN (0x7fc00000, whatever the input's sign or payload), x >= 0x1.62e430p+6 -> +inf,
// x <= -0x1.9fe368p+6 -> +0.  Proven against this numpy over all 2^32 inputs by tests/devtools/check_np_exp.py (host twin and
// device), and probed at run time against the running process's numpy (_lib.np_exp_probe).
//
// Every operation is written out: the library is built with -ffp-contract=off, and a host-only compile of this header must
// be too (tests/devtools/check_np_exp.py compiles it with -ffp-contract=off -mfma).
#pragma once

#include <stdint.h>
#include <string.h>
#include <math.h>

#if !defined(__HIPCC__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace gsx {

#if defined(__HIP_DEVICE_COMPILE__)
#define GSX_NPX_FMA(a, b, c) __fmaf_rn((a), (b), (c))
#define GSX_NPX_DIV(a, b) __fdiv_rn((a), (b))
#define GSX_NPX_MUL(a, b) __fmul_rn((a), (b))
#define GSX_NPX_RINT(a) __builtin_rintf(a)
#define GSX_NPX_LDEXP(a, e) __builtin_ldexpf((a), (e))
#else
#define GSX_NPX_FMA(a, b, c) fmaf((a), (b), (c))
#define GSX_NPX_DIV(a, b) ((a) / (b))
#define GSX_NPX_MUL(a, b) ((a) * (b))
#define GSX_NPX_RINT(a) rintf(a)            // round half to even (the default rounding mode)
#define GSX_NPX_LDEXP(a, e) ldexpf((a), (e))
#endif

__host__ __device__ inline uint32_t np_f32_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

__host__ __device__ inline float np_bits_f32(uint32_t u)
{
    float v;
    memcpy(&v, &u, 4);
    return v;
}

// np.exp(np.float32 x)
__host__ __device__ inline float np_expf(float x)
{
    const float xmax = 88.72283935546875f;          // 0x1.62e430p+6: at or above, numpy returns +inf
    const float xmin = -103.972084045410156f;       // -0x1.9fe368p+6: at or below, +0
    if (x != x) return np_bits_f32(0x7fc00000u);
    if (x >= xmax) return np_bits_f32(0x7f800000u);
    if (x <= xmin) return 0.0f;
    const float q = GSX_NPX_RINT(GSX_NPX_MUL(x, 1.44269504088896341f));   // x * log2(e), rounded to float32, then to an integer
    float y = GSX_NPX_FMA(q, -6.93145752e-1f, x);
    y = GSX_NPX_FMA(q, -1.42860677e-6f, y);
    float num = GSX_NPX_FMA(5.082762527590693718096e-04f, y, 6.757896990527504603057e-03f);
    num = GSX_NPX_FMA(num, y, 5.114512081637298353406e-02f);
    num = GSX_NPX_FMA(num, y, 2.473615434895520810817e-01f);
    num = GSX_NPX_FMA(num, y, 7.257664613233124478488e-01f);
    num = GSX_NPX_FMA(num, y, 9.999999999980870924916e-01f);
    float den = GSX_NPX_FMA(2.159509375685829852307e-02f, y, -2.742335390411667452936e-01f);
    den = GSX_NPX_FMA(den, y, 1.0f);
    return GSX_NPX_LDEXP(GSX_NPX_DIV(num, den), (int)q);   // one rounding, denormal results included (numpy: vscalefps)
}

}  // namespace gsx
