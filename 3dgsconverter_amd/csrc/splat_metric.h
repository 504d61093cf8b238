// splat_metric.h -- the .splat writer's visibility metric (gsconverter/formats/splat.py:92-94) as the u32 key its order is
// sorted by, shared by the writer (csrc/splat.hip: splat_metric_key) and the splat budget filter (csrc/limit.hip): one
// implementation, so the rows a budget keeps are the rows the writer would have written first.
#pragma once

#include "np_exp.h"
#include "sog_math.h"

namespace gsx {

// exp((s0 + s1) + s2) * (1 / (1 + exp(-opacity))) in float32, numpy's order, exp = np_exp.h -> sort_key of its negative: the
// most visible row has the smallest key, a NaN metric 0xffffffff
__device__ __forceinline__ unsigned splat_metric_key_of(float s0, float s1, float s2, float opacity)
{
    const float ssum = __fadd_rn(__fadd_rn(s0, s1), s2);
    const float opa = __fdiv_rn(1.0f, __fadd_rn(1.0f, np_expf(-opacity)));
    return sort_key(-__fmul_rn(np_expf(ssum), opa));
}

}  // namespace gsx
