// knn_mean_cert.h -- is the float32 mean of 16 APPROXIMATE float64 roots already the float32 the exact epilogue would store?
// Plain C++17 arithmetic on one number: no HIP header, so a host compiler can include it and a test can drive it without a
// GPU (tools/check_mean_cert_host.cpp, tests/test_mean_cert_host.py).  knn_brick's epilogue (knn_common.h:
// mean_from_net_cert) is the one caller on the device.
//
// What leaves knn_brick per query is one float32, (float)(sum of 16 float64 roots / 16).  The exact epilogue (mean_from_net)
// rounds every root correctly and adds them in numpy's order; its float64 mean is
//     m* = (sum_i sqrt(x_i)) (1 + t),   |t| <= 5.01 u,  u = 2^-53
// (u for each correctly rounded root, 4 u for the four additions any root passes through in the 8-accumulator shape; the
// division by 16 is exact).  The short epilogue takes roots with a relative error of at most E (sqrt_short_dist2) and adds them
// in whatever order the list is in:
//     m  = (sum_i sqrt(x_i) (1 + e_i)) (1 + t'),   |e_i| <= E,  |t'| <= 15.01 u  (16 non-negative terms, any order)
// so |m* - m| <= (E + 21 u) m to first order, the second-order terms below 2^-60 m for E < 2^-30.
//
// E is MEASURED, not derived: profiles/epilogue_cert_ab.txt has the largest relative error of the v_rsq_f64 seed and of the
// short root over every binade of the domain (tests/epilogue_cases.py: root_inputs, 4.3M values).  KNN_SHORT_ROOT_BOUND below is
// 64 times that maximum -- the factor covers mantissas the sample misses -- and tests/test_epilogue_cert_gpu.py holds the
// short root against it on whatever GPU runs the suite.
#pragma once

#if defined(__HIP__)
#define GSX_CERT_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GSX_CERT_HD inline
#endif

namespace gsx {

// measured on MI355X: seed e0 <= 5.22e-8 = 2^-24.19, short root <= 4.089e-15 = 2^-47.80 (1.5 e0^2 = 4.08e-15) -- times 64,
// rounded up to three hexadecimal digits: 2.62e-13 = 2^-41.8
constexpr double KNN_SHORT_ROOT_BOUND = 0x1.27p-42;
struct KnnMeanEps {
    static constexpr double value = KNN_SHORT_ROOT_BOUND + 32.0 * 0x1p-53;   // E + 21 u and the second-order terms, rounded up
};

struct MeanCert {
    float f;        // (float)(S / 16)
    bool certain;   // every real within EPS m of m = S / 16 rounds to f
};

// S: a float64 sum of 16 roots, >= 0 and either 0 or in [2^-149, 2^134) (roots of squared differences of float32 coordinates).
//
// certain is true when (float)lo == (float)hi for two doubles lo <= m (1 - EPS) and hi >= m (1 + EPS).  Rounding to float32 is
// monotone, so then every real in [lo, hi] -- m itself, and the exact epilogue's m* -- rounds to that one float, which is f.
// The directed slack: with e = EPS + 2^-50, the constants are CLO = (1 - e)(1 + d1) / 16 and CHI = (1 + e)(1 + d2) / 16 as
// the compiler folds them (forming e is exact or rounds once more, which the bound below leaves room for; the factor 1 / 16
// is exact) and the products round once more: lo = S CLO (1 + d3), hi = S CHI (1 + d4), every |d| <= u.  Hence
//     lo <= m (1 - e)(1 + u)^2 < m (1 - e + 2.01 u) < m (1 - EPS)      as 2^-50 = 8 u > 2.01 u,
//     hi >= m (1 + e)(1 - u)^2 > m (1 + e - 2.01 u - 2 e u) > m (1 + EPS).
// Nothing under- or overflows: S CLO and S CHI stay within [2^-154, 2^131).  S = 0 gives lo = hi = 0: certain, f = 0.
// Where the flag is false nothing is claimed; the caller recomputes exactly.  The interval tested is at most EPS + 2^-49 wide
// on either side, so the flag is false only when a float32 rounding boundary lies within that of m.
template <class EPS>
GSX_CERT_HD MeanCert mean_cert16(double S)
{
    static_assert(EPS::value > 0.0 && EPS::value < 0x1p-30, "relative bound out of the range the slack argument covers");
    constexpr double e = EPS::value + 0x1p-50;
    constexpr double CLO = 0.0625 * (1.0 - e), CHI = 0.0625 * (1.0 + e);
    MeanCert c;
    c.f = (float)(S * 0.0625);
    c.certain = (float)(S * CLO) == (float)(S * CHI);
    return c;
}

}  // namespace gsx
