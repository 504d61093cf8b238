// knn_probe.hip -- debug / tests: the device functions of the KNN epilogue (knn_common.h) on inputs the caller chooses.
//
// Every mean distance the library returns is (float)(sum of k float64 roots / k).  Through the KNN kernels the roots and
// the order of the additions are only ever seen after that rounding to float32, on clouds where a root one ulp off or a
// different order moves no result.  These entry points call the SAME inline functions the kernels call -- sqrt_rn_dist2,
// mean_from_net<L>, mean_from_list<KCAP>, pairwise_sum_le128, pairwise_sum_np<5>, mean_finish -- for every L and KCAP the
// kernels instantiate, so that tests/test_knn_epilogue_gpu.py can feed them roots next to a rounding boundary and rows
// whose float32 mean depends on the order of the float64 additions.  Nothing here is on a hot path.
#include <algorithm>

#include "gsx_common.h"
#include "knn_common.h"

namespace gsx {

constexpr int PROBE_THREADS = 64;      // one wave: a row per lane (net, list) or a row per wave (le128, np)
constexpr int PROBE_NP_MAX = 1000;     // longest row of the pairwise_sum_np form

template <int MODE>
__global__ __launch_bounds__(256) void probe_root_kernel(const double *__restrict__ in, int64_t n, double *__restrict__ out)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        out[i] = MODE == 0 ? sqrt_rn_dist2(in[i]) : __dsqrt_rn(in[i]);
}

// the short root of the certified epilogue (MODE 0) and the hardware seed it starts from (MODE 1: what sqrt_short_dist2 and
// sqrt_rn_dist2 both take v_rsq_f64 of)
template <int MODE>
__global__ __launch_bounds__(256) void probe_root_short_kernel(const double *__restrict__ in, int64_t n, double *__restrict__ out)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if constexpr (MODE == 0) {
            out[i] = sqrt_short_dist2(in[i]);
        } else {
            double xs;
            asm("v_max_f64 %0, %1, %2" : "=v"(xs) : "v"(in[i]), "v"(1e-300));
            out[i] = __builtin_amdgcn_rsq(xs);
        }
    }
}

// knn_brick / knn_leaf: the list holds the L nearest NEIGHBOURS' squared distances (entries past the row: +inf, as init() leaves them)
template <int L>
__global__ __launch_bounds__(PROBE_THREADS) void probe_net_kernel(const double *__restrict__ d2, int64_t m, int64_t stride, int k,
                                                                  float *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (r >= m) return;
    TopNet<L> lst;
    lst.init();
#pragma unroll
    for (int j = 0; j < L; ++j)
        if (j < stride) lst.a[j] = d2[r * stride + j];
    out[r] = mean_from_net(lst, k);
}

// knn_brick (phase2_net = 0) / knn_brute: entry 0 is the query itself, squared distance 0
template <int KCAP>
__global__ __launch_bounds__(PROBE_THREADS) void probe_list_kernel(const double *__restrict__ d2, int64_t m, int64_t stride, int k,
                                                                   float *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (r >= m) return;
    TopList<KCAP> lst;
    lst.init();
    lst.a[0] = 0.0;
#pragma unroll
    for (int j = 0; j < KCAP - 1; ++j)
        if (j < stride) lst.a[1 + j] = d2[r * stride + j];
    out[r] = mean_from_list<KCAP>(lst, k);
}

// knn_ring, knn_ring_fast, knn_heavy_merge, the tree's fallbacks (NP = false): the k+1 winners sit in LDS, the wave takes
// __dsqrt_rn of one each, lane 0 sums entries 1..k with pairwise_sum_le128.  knn_anyk (NP = true): sqrt_rn_dist2 and
// pairwise_sum_np<5>.  One wave per row.
template <bool NP>
__global__ __launch_bounds__(PROBE_THREADS) void probe_lds_kernel(const double *__restrict__ d2, int64_t m, int64_t stride, int k,
                                                                  float *__restrict__ out)
{
    __shared__ double s_out[1 + (NP ? PROBE_NP_MAX : 128)];
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    if (r >= m) return;   // block-uniform
    const int kk = k + 1;
    for (int i = lane; i < kk; i += 64) s_out[i] = i == 0 ? 0.0 : d2[r * stride + i - 1];
    __syncthreads();
    for (int i = lane; i < kk; i += 64) s_out[i] = NP ? sqrt_rn_dist2(s_out[i]) : __dsqrt_rn(s_out[i]);
    __syncthreads();
    if (lane == 0) {
        double sum;
        if constexpr (NP) sum = pairwise_sum_np<5>([&](int i) { return s_out[1 + i]; }, 0, k);
        else sum = pairwise_sum_le128([&](int i) { return s_out[1 + i]; }, k);
        out[r] = mean_finish(sum, k);
    }
}

template <int L>
static int launch_probe_net(gsx_ctx *ctx, const double *d2, int64_t m, int64_t stride, int k, float *out)
{
    hipLaunchKernelGGL((probe_net_kernel<L>), dim3(div_up(m, PROBE_THREADS)), dim3(PROBE_THREADS), 0, ctx->stream, d2, m, stride, k, out);
    GSX_HIP(hipGetLastError());
    return 0;
}

template <int KCAP>
static int launch_probe_list(gsx_ctx *ctx, const double *d2, int64_t m, int64_t stride, int k, float *out)
{
    hipLaunchKernelGGL((probe_list_kernel<KCAP>), dim3(div_up(m, PROBE_THREADS)), dim3(PROBE_THREADS), 0, ctx->stream, d2, m, stride, k, out);
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_knn_probe_root_dev(gsx_ctx *c, const double *in_dev, int64_t n, int mode, double *out_dev)
{
    if (!c || !in_dev || !out_dev || n <= 0) GSX_FAIL("gsx_knn_probe_root_dev: bad arguments");
    if (mode != GSX_PROBE_ROOT_DIST2 && mode != GSX_PROBE_ROOT_DSQRT) GSX_FAIL("gsx_knn_probe_root_dev: unknown mode %d", mode);
    GSX_HIP(hipSetDevice(c->device));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(div_up(n, 256), (int64_t)c->num_cu * 8));
    if (mode == GSX_PROBE_ROOT_DIST2) hipLaunchKernelGGL(probe_root_kernel<0>, dim3(blocks), dim3(256), 0, c->stream, in_dev, n, out_dev);
    else hipLaunchKernelGGL(probe_root_kernel<1>, dim3(blocks), dim3(256), 0, c->stream, in_dev, n, out_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_knn_probe_root_short_dev(gsx_ctx *c, const double *in_dev, int64_t n, int mode, double *out_dev)
{
    if (!c || !in_dev || !out_dev || n <= 0) GSX_FAIL("gsx_knn_probe_root_short_dev: bad arguments");
    if (mode != GSX_PROBE_SHORT_ROOT && mode != GSX_PROBE_SHORT_SEED) GSX_FAIL("gsx_knn_probe_root_short_dev: unknown mode %d", mode);
    GSX_HIP(hipSetDevice(c->device));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(div_up(n, 256), (int64_t)c->num_cu * 8));
    if (mode == GSX_PROBE_SHORT_ROOT) hipLaunchKernelGGL(probe_root_short_kernel<0>, dim3(blocks), dim3(256), 0, c->stream, in_dev, n, out_dev);
    else hipLaunchKernelGGL(probe_root_short_kernel<1>, dim3(blocks), dim3(256), 0, c->stream, in_dev, n, out_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_knn_probe_mean_dev(gsx_ctx *c, const double *d2_dev, int64_t m, int64_t stride, int k, int form, int cap, float *out_dev)
{
    if (!c || !d2_dev || !out_dev || m <= 0 || m > (int64_t)1 << 24) GSX_FAIL("gsx_knn_probe_mean_dev: bad arguments");
    if (k < 1 || stride < k) GSX_FAIL("gsx_knn_probe_mean_dev: need 1 <= k <= stride (k=%d, stride=%lld)", k, (long long)stride);
    GSX_HIP(hipSetDevice(c->device));
    switch (form) {
    case GSX_PROBE_MEAN_NET:   // the list lengths of dispatch_bricks (csrc/sor_grid.hip) and launch_knn_tree (csrc/sor_tree.hip)
        if (k > cap) GSX_FAIL("gsx_knn_probe_mean_dev: k=%d does not fit TopNet<%d>", k, cap);
        switch (cap) {
#define GSX_PROBE_NET(L) case L: return launch_probe_net<L>(c, d2_dev, m, stride, k, out_dev);
            GSX_PROBE_NET(8) GSX_PROBE_NET(16) GSX_PROBE_NET(24) GSX_PROBE_NET(32) GSX_PROBE_NET(40) GSX_PROBE_NET(48) GSX_PROBE_NET(56)
            GSX_PROBE_NET(64)
#if GSX_CAP4
            GSX_PROBE_NET(12) GSX_PROBE_NET(20) GSX_PROBE_NET(28) GSX_PROBE_NET(36) GSX_PROBE_NET(44) GSX_PROBE_NET(52)
#endif
#undef GSX_PROBE_NET
        }
        GSX_FAIL("gsx_knn_probe_mean_dev: no kernel instantiates TopNet<%d>", cap);
    case GSX_PROBE_MEAN_LIST:  // the capacities of dispatch_bricks with phase2_net = 0 and of launch_knn_brute (csrc/sor_brute.hip)
        if (k > cap - 1) GSX_FAIL("gsx_knn_probe_mean_dev: k=%d does not fit TopList<%d>", k, cap);
        switch (cap) {
#define GSX_PROBE_LIST(K) case K: return launch_probe_list<K>(c, d2_dev, m, stride, k, out_dev);
            GSX_PROBE_LIST(9) GSX_PROBE_LIST(17) GSX_PROBE_LIST(26) GSX_PROBE_LIST(33) GSX_PROBE_LIST(51) GSX_PROBE_LIST(65)
#undef GSX_PROBE_LIST
        }
        GSX_FAIL("gsx_knn_probe_mean_dev: no kernel instantiates TopList<%d>", cap);
    case GSX_PROBE_MEAN_LE128:
        if (k > 128) GSX_FAIL("gsx_knn_probe_mean_dev: pairwise_sum_le128 takes k <= 128 (k=%d)", k);
        hipLaunchKernelGGL(probe_lds_kernel<false>, dim3((unsigned)m), dim3(PROBE_THREADS), 0, c->stream, d2_dev, m, stride, k, out_dev);
        break;
    case GSX_PROBE_MEAN_NP:
        if (k > PROBE_NP_MAX) GSX_FAIL("gsx_knn_probe_mean_dev: the pairwise_sum_np form takes k <= %d (k=%d)", PROBE_NP_MAX, k);
        hipLaunchKernelGGL(probe_lds_kernel<true>, dim3((unsigned)m), dim3(PROBE_THREADS), 0, c->stream, d2_dev, m, stride, k, out_dev);
        break;
    default:
        GSX_FAIL("gsx_knn_probe_mean_dev: unknown form %d", form);
    }
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
