// np_log.h -- numpy's float32 log (the AVX512F / AVX2+FMA3 SIMD routine of numpy/_core/src/umath/loops_exponent_log), bit
// for bit, as __host__ __device__ code.
//
// numpy's float32 log is not correctly rounded, so a reader that stores its raw bits (the .splat scales, csrc/splat_read.hip)
// must repeat numpy's own steps:
//   x = m 2^e with m in [0.5, 1) (denormals normalised); m <= sqrt(1/2) is doubled and e lowered, so that m - 1 (exact) lies in
//   (sqrt(1/2) - 1, sqrt(2) - 1]; a [5/5] rational approximation of log(1 + t) in Horner form with fused steps, one IEEE division,
//   and one fused step that adds e ln 2.
// Inputs numpy masks out: NaN -> +qNaN (0x7fc00000, whatever the input's sign or payload), x < 0 (-inf included) -> -qNaN
// (0xffc00000), +-0 -> -inf, +inf -> +inf.  Proven against this numpy over all 2^32 inputs by tests/devtools/check_np_log.py
// (host twin and device), and probed at run time against the running process's numpy (_lib.np_log_probe).
//
// Every operation is written out: the library is built with -ffp-contract=off, and a host-only compile of this header must
// be too (tests/devtools/check_np_log.py compiles it with -ffp-contract=off -mfma).  frexp is integer work on the bits, the
// same on the host and on the device.
#pragma once

#include "np_exp.h"

namespace gsx {

// np.log(np.float32 x)
__host__ __device__ inline float np_logf(float x)
{
    const uint32_t u = np_f32_bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return np_bits_f32(0x7fc00000u);   // NaN
    if ((u << 1) == 0u) return np_bits_f32(0xff800000u);                     // +-0 -> -inf
    if (u >> 31) return np_bits_f32(0xffc00000u);                            // x < 0
    if (u == 0x7f800000u) return x;
    // frexp: x = m 2^e, m in [0.5, 1)
    uint32_t frac = u & 0x007fffffu;
    int e = (int)(u >> 23) - 126;
    if (u < 0x00800000u) {                                  // denormal: frac 2^-149, its top bit moved up to bit 23
        const int up = __builtin_clz(frac) - 8;
        frac = (frac << up) & 0x007fffffu;
        e = -125 - up;
    }
    float m = np_bits_f32(0x3f000000u | frac);
    if (m <= 0.70710678118654752440f) {
        m = m + m;
        e -= 1;
    }
    m = m - 1.0f;
    float num = GSX_NPX_FMA(2.589979117907922693523e-02f, m, 3.808837741388407920751e-01f);
    num = GSX_NPX_FMA(num, m, 1.480000633576506585156e+00f);
    num = GSX_NPX_FMA(num, m, 2.112677543073053063722e+00f);
    num = GSX_NPX_FMA(num, m, 9.999999999999998702752e-01f);
    num = GSX_NPX_FMA(num, m, 0.0f);
    float den = GSX_NPX_FMA(5.875095403124574342950e-03f, m, 1.546476374983906719538e-01f);
    den = GSX_NPX_FMA(den, m, 9.864942958519418960339e-01f);
    den = GSX_NPX_FMA(den, m, 2.453006071784736363091e+00f);
    den = GSX_NPX_FMA(den, m, 2.612677543073109236779e+00f);
    den = GSX_NPX_FMA(den, m, 1.0f);
    return GSX_NPX_FMA((float)e, 0.693147180559945309417f, GSX_NPX_DIV(num, den));
}

}  // namespace gsx
