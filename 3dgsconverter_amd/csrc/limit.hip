// limit.hip -- the splat budget (--max_splats): keep the N most visible rows of a table, in input order.  No counterpart in the
// reference; "most visible" is the order of its .splat writer (gsconverter/formats/splat.py:92-98), so a budgeted table written
// as .splat is the head of the unbudgeted file.
//
//   gsx_limit_keys_dev     (s0, s1, s2, opacity) of every row -> the writer's u32 key (splat_metric.h: smallest = most visible,
//                          NaN = 0xffffffff)
//   gsx_limit_select_dev   mask[j] = row j is among the N smallest keys of the chain's n rows, equal keys by row index
//   gsx_limit_select_host  the same answer on host arrays, from the same decisions (limit_select.h)
//
// The select is a radix select, not a sort: it finds the threshold key T (the N-th smallest) one 8-bit digit at a time, most
// significant first.  Pass p reads the keys once and counts, per value of digit p, those that agree with T in the digits
// already found: a 256-bin histogram per wave in LDS, the waves' bins summed, and one integer atomicAdd per non-empty bin and
// workgroup into the pass's 256 global bins (Guideline 12: partial sums on chip, one atomic per block; integer adds, so the
// counts do not depend on arrival order).  A one-workgroup kernel walks the bins (limit_walk) and leaves the digit and the rank
// inside its bin in device memory for the next pass: the host is not asked between passes.  After four passes the bin is the
// rows with key == T, of which the first `remaining` in input order are kept: their ranks come from per-tile tie counts, the
// chain's one-workgroup scan (tile_scan.h) and a ballot inside the tile, the shape of the chain's compaction.  Five reads of the
// keys and one write of the mask; the workspace is 8 + 4 * 256 + n / 2048 words.
#include <algorithm>

#include "gsx_common.h"
#include "limit_select.h"
#include "row_tile.h"
#include "splat_metric.h"
#include "tile_scan.h"

namespace gsx {

constexpr int LIM_TILE = 2048;                       // rows per tile of the tie-rank passes: 8 per lane
enum { LIM_PREFIX = 0, LIM_REMAINING, LIM_KEPT, LIM_TIES, LIM_TIES_SCANNED, LIM_STATE_WORDS = 8 };

// row j of the chain -> its key (the convention of mask_ge_kernel)
__device__ __forceinline__ unsigned limit_key_of(const unsigned *__restrict__ keys, const unsigned *__restrict__ orig, int64_t j)
{
    return keys[orig ? orig[j] : (unsigned)j];
}

__global__ __launch_bounds__(256) void limit_keys_kernel(const float4 *__restrict__ cols, int64_t n, unsigned *__restrict__ keys)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 v = cols[i];
        keys[i] = splat_metric_key_of(v.x, v.y, v.z, v.w);
    }
}

__global__ __launch_bounds__(256) void limit_hist_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ orig, int64_t n, int pass,
                                                         const unsigned *__restrict__ state, unsigned *__restrict__ hist)
{
    __shared__ unsigned s_h[4][LIMIT_BINS];
    const int t = threadIdx.x, wv = t >> 6;
#pragma unroll
    for (int w = 0; w < 4; ++w) s_h[w][t] = 0u;
    __syncthreads();
    const unsigned prefix = pass ? state[LIM_PREFIX] : 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned k = limit_key_of(keys, orig, i);
        if (limit_matches(k, prefix, pass)) atomicAdd(&s_h[wv][limit_digit(k, pass)], 1u);
    }
    __syncthreads();
    const unsigned c = s_h[0][t] + s_h[1][t] + s_h[2][t] + s_h[3][t];
    if (c) atomicAdd(&hist[t], c);
}

// one workgroup: pass `pass`'s bins -> the next digit of the threshold and the rank inside its bin
__global__ __launch_bounds__(256) void limit_pick_kernel(const unsigned *__restrict__ hist, int pass, unsigned want, unsigned *__restrict__ state)
{
    __shared__ unsigned s_h[LIMIT_BINS];
    s_h[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned prefix = pass ? state[LIM_PREFIX] : 0u, remaining = pass ? state[LIM_REMAINING] : want;
        const unsigned bin = limit_walk(s_h, pass, &prefix, &remaining);
        state[LIM_PREFIX] = prefix;
        state[LIM_REMAINING] = remaining;
        state[LIM_KEPT] = want;
        state[LIM_TIES] = bin;
    }
}

__global__ __launch_bounds__(256) void limit_tie_count_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ orig, int64_t n,
                                                              const unsigned *__restrict__ state, unsigned *__restrict__ tile_cnt)
{
    __shared__ unsigned s[4];
    const unsigned T = state[LIM_PREFIX];
    const int64_t base = (int64_t)blockIdx.x * LIM_TILE;
    unsigned c = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t i = base + u * 256 + threadIdx.x;
        c += (i < n && limit_key_of(keys, orig, i) == T) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// tile_off: the exclusive scan of the tile tie counts.  Element order inside a tile is u-major (u * 256 + thread): input order
__global__ __launch_bounds__(256) void limit_mask_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ orig, int64_t n,
                                                         const unsigned *__restrict__ state, const unsigned *__restrict__ tile_off,
                                                         uint8_t *__restrict__ mask)
{
    __shared__ unsigned s_w[4];
    const unsigned T = state[LIM_PREFIX], ties_kept = state[LIM_REMAINING];
    const int64_t base = (int64_t)blockIdx.x * LIM_TILE;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned run = tile_off[blockIdx.x];
    for (int u = 0; u < 8; ++u) {
        const int64_t i = base + u * 256 + threadIdx.x;
        const unsigned k = i < n ? limit_key_of(keys, orig, i) : 0u;
        const bool tie = i < n && k == T;
        const unsigned long long bal = __ballot(tie);
        if (lane == 0) s_w[wv] = (unsigned)__builtin_popcountll(bal);
        __syncthreads();
        unsigned rank = run + (unsigned)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) rank += s_w[w];
        if (i < n) mask[i] = limit_keeps(k, T, rank, ties_kept) ? 1 : 0;
        run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_limit_keys_dev(gsx_ctx *c, const float *cols_dev, int64_t n0, uint32_t *keys_dev)
{
    if (!c || (n0 > 0 && (!cols_dev || !keys_dev))) GSX_FAIL("gsx_limit_keys_dev: null argument");
    if (n0 < 0 || n0 >= (1LL << 32)) GSX_FAIL("gsx_limit_keys_dev: 0 <= n0 < 2^32");
    if ((reinterpret_cast<uintptr_t>(cols_dev) & 15) || (reinterpret_cast<uintptr_t>(keys_dev) & 3))
        GSX_FAIL("gsx_limit_keys_dev: the columns must be 16-byte aligned, the keys 4-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    if (n0 == 0) return 0;
    hipLaunchKernelGGL(limit_keys_kernel, dim3(tile_blocks(c, n0, 1024, 8)), dim3(256), 0, c->stream, reinterpret_cast<const float4 *>(cols_dev), n0,
                       keys_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_limit_select_dev(gsx_ctx *c, const uint32_t *keys_dev, const uint32_t *orig_dev, int64_t n, int64_t max_count, uint8_t *mask_dev,
                         uint32_t *info_out)
{
    if (!c || !info_out || (n > 0 && (!keys_dev || !mask_dev))) GSX_FAIL("gsx_limit_select_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_limit_select_dev: 0 <= n < 2^32");
    if (max_count < 1) GSX_FAIL("gsx_limit_select_dev: a budget of %lld rows (at least 1)", (long long)max_count);
    if ((reinterpret_cast<uintptr_t>(keys_dev) & 3) || (reinterpret_cast<uintptr_t>(orig_dev) & 3))
        GSX_FAIL("gsx_limit_select_dev: keys and survivor list must be 4-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    info_out[0] = info_out[1] = info_out[2] = 0u;
    if (n == 0) return 0;
    const unsigned want = (unsigned)std::min<int64_t>(max_count, n);
    const int ntiles = div_up(n, LIM_TILE);
    GSX_CHECK(c->statspart.reserve(sizeof(unsigned) * (LIM_STATE_WORDS + (size_t)LIMIT_PASSES * LIMIT_BINS + (size_t)ntiles)));
    unsigned *state = c->statspart.as<unsigned>();
    unsigned *hist = state + LIM_STATE_WORDS;
    unsigned *tiles = hist + LIMIT_PASSES * LIMIT_BINS;
    GSX_HIP(hipMemsetAsync(state, 0, sizeof(unsigned) * (LIM_STATE_WORDS + (size_t)LIMIT_PASSES * LIMIT_BINS), c->stream));
    const unsigned blocks = tile_blocks(c, n, 4096, 4);
    for (int pass = 0; pass < LIMIT_PASSES; ++pass) {
        unsigned *h = hist + pass * LIMIT_BINS;
        hipLaunchKernelGGL(limit_hist_kernel, dim3(blocks), dim3(256), 0, c->stream, keys_dev, orig_dev, n, pass, state, h);
        hipLaunchKernelGGL(limit_pick_kernel, dim3(1), dim3(256), 0, c->stream, h, pass, want, state);
    }
    hipLaunchKernelGGL(limit_tie_count_kernel, dim3(ntiles), dim3(256), 0, c->stream, keys_dev, orig_dev, n, state, tiles);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, c->stream, tiles, ntiles, state + LIM_TIES_SCANNED);
    hipLaunchKernelGGL(limit_mask_kernel, dim3(ntiles), dim3(256), 0, c->stream, keys_dev, orig_dev, n, state, tiles, mask_dev);
    GSX_HIP(hipGetLastError());
    GSX_HIP(hipMemcpyAsync(info_out, state, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_limit_select_host(const uint32_t *keys, const uint32_t *orig, int64_t n, int64_t max_count, uint8_t *mask, uint32_t *info_out)
{
    if (!info_out || (n > 0 && (!keys || !mask))) GSX_FAIL("gsx_limit_select_host: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_limit_select_host: 0 <= n < 2^32");
    if (max_count < 1) GSX_FAIL("gsx_limit_select_host: a budget of %lld rows (at least 1)", (long long)max_count);
    info_out[0] = info_out[1] = info_out[2] = 0u;
    if (n == 0) return 0;
    const uint32_t want = (uint32_t)std::min<int64_t>(max_count, n);
    auto key_of = [&](int64_t j) { return keys[orig ? orig[j] : (uint32_t)j]; };
    uint32_t prefix = 0u, remaining = want;
    for (int pass = 0; pass < LIMIT_PASSES; ++pass) {
        uint32_t hist[LIMIT_BINS] = {0u};
        for (int64_t j = 0; j < n; ++j) {
            const uint32_t k = key_of(j);
            if (limit_matches(k, prefix, pass)) ++hist[limit_digit(k, pass)];
        }
        (void)limit_walk(hist, pass, &prefix, &remaining);
    }
    uint32_t rank = 0u;
    for (int64_t j = 0; j < n; ++j) {
        const uint32_t k = key_of(j);
        mask[j] = limit_keeps(k, prefix, rank, remaining) ? 1 : 0;
        rank += k == prefix ? 1u : 0u;
    }
    info_out[0] = prefix;
    info_out[1] = remaining;
    info_out[2] = want;
    return 0;
}

}  // extern "C"
