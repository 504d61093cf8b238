// limit_select.h -- the decisions of the splat budget's radix select, shared by the kernels of csrc/limit.hip and their host
// twin (gsx_limit_select_host): which digit of the u32 keys a pass looks at, which keys still take part, the walk over a pass's
// histogram that fixes one digit of the threshold key, and the rule that keeps a row.
//
// The select finds T, the N-th smallest key, most significant digit first: pass p counts, per value of digit p, the keys
// that agree with T in the digits found so far; the walk picks the digit whose bin holds the `remaining`-th of them and leaves
// `remaining` as a rank inside that bin.  After the last pass the bin is the keys equal to T and `remaining` >= 1 is how many
// of them are kept -- the first ones in input order.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace gsx {

constexpr int LIMIT_DIGIT_BITS = 8;
constexpr int LIMIT_BINS = 1 << LIMIT_DIGIT_BITS;
constexpr int LIMIT_PASSES = 32 / LIMIT_DIGIT_BITS;

__host__ __device__ inline int limit_shift(int pass) { return 32 - LIMIT_DIGIT_BITS * (pass + 1); }

__host__ __device__ inline uint32_t limit_digit(uint32_t key, int pass) { return (key >> limit_shift(pass)) & (uint32_t)(LIMIT_BINS - 1); }

// does `key` agree with `prefix` in the digits of the passes before `pass`?
__host__ __device__ inline bool limit_matches(uint32_t key, uint32_t prefix, int pass)
{
    return pass == 0 || ((key ^ prefix) >> (limit_shift(pass) + LIMIT_DIGIT_BITS)) == 0u;
}

// hist[LIMIT_BINS]: pass `pass`'s counts, 1 <= *remaining <= their sum.  The digit goes into *prefix; *remaining becomes the
// rank (from 1) inside the digit's bin; -> that bin's count
__host__ __device__ inline uint32_t limit_walk(const uint32_t *hist, int pass, uint32_t *prefix, uint32_t *remaining)
{
    uint32_t r = *remaining, d = 0;
    while (d + 1 < (uint32_t)LIMIT_BINS && hist[d] < r) r -= hist[d++];
    *prefix |= d << limit_shift(pass);
    *remaining = r;
    return hist[d];
}

// tie_rank: the row's rank (from 0, input order) among the rows whose key equals the threshold
__host__ __device__ inline bool limit_keeps(uint32_t key, uint32_t threshold, uint32_t tie_rank, uint32_t ties_kept)
{
    return key < threshold || (key == threshold && tie_rank < ties_kept);
}

}  // namespace gsx
