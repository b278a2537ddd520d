// mtq_glu.hpp — the gated-linear-unit activation, in one place: every kernel that gates (mtq_glu_combine, the fused wide kernels of
// mtq_packed.hip) calls glu_value and nothing else computes it, so the fused and the unfused route give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mtq.h"

namespace mtq {

// h = act(g) * u, every operation a separately rounded float32 one:
//   MTQ_ACT_SILU  t = expf(-g) (the accurate expf), d = 1 + t, s = g / d, h = s * u
//   MTQ_ACT_NONE  h = g * u
// Contraction is off inside (the __f*_rn forms are never fused), so no caller's surrounding code fuses into it or out of it.  Inf, NaN
// and -0 get no special case: what the sequence gives is the definition (silu(-inf) = -inf / inf = NaN, for one).  An `act` that is
// neither code is refused by the entries before a launch.
__device__ __forceinline__ float glu_value(float g, float u, int act)
{
#pragma clang fp contract(off)
    if (act == MTQ_ACT_NONE) return __fmul_rn(g, u);
    const float t = expf(-g);
    const float s = __fdiv_rn(g, __fadd_rn(1.0f, t));
    return __fmul_rn(s, u);
}

} // namespace mtq
