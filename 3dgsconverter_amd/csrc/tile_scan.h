// tile_scan.h -- the one-workgroup exclusive scan of per-tile counts between a count pass and a write pass: the chain's stable
// compaction (csrc/chain.hip) and the tie ranks of the splat budget's select (csrc/limit.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace gsx {

// exclusive scan of the tile counts in place (one workgroup of 1024 lanes); total -> *total_out.  static: both users compile
// their own copy
static __global__ __launch_bounds__(1024) void compact_scan_kernel(unsigned *__restrict__ tile_cnt, int ntiles, unsigned *__restrict__ total_out)
{
    __shared__ unsigned s_w[16];
    __shared__ unsigned s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int b = 0; b < ntiles; b += 1024) {
        const int i = b + threadIdx.x;
        const unsigned v = i < ntiles ? tile_cnt[i] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(inc, off);
            if ((int)(threadIdx.x & 63) >= off) inc += o;
        }
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        unsigned pre = s_carry;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += s_w[w];
        if (i < ntiles) tile_cnt[i] = pre + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = pre + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = s_carry;
}

}  // namespace gsx
