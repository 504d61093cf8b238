// view_key.h -- the ranking key of a row's summed view contribution, shared by the device kernel and its host twin.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GSX_VIEW_KEY_FN __host__ __device__ __forceinline__
#else
#define GSX_VIEW_KEY_FN inline
#endif

namespace gsx {

// 0xffffffff - fbits(total), fbits the bit pattern of `total` converted to float32 rounding toward zero, in integers: the
// most visible row has the smallest key, a row no view blended 0xffffffff.  fbits is monotone in total, so is the key.
GSX_VIEW_KEY_FN uint32_t view_key_of(uint64_t total)
{
    if (total == 0) return 0xffffffffu;
    const int e = 63 - __builtin_clzll((unsigned long long)total);       // bit_length(total) - 1
    const uint64_t m = e >= 23 ? total >> (e - 23) : total << (23 - e);
    return 0xffffffffu - ((uint32_t)(e + 127) << 23 | (uint32_t)(m & 0x7fffffull));
}

}  // namespace gsx
