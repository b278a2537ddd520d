// mtq_hadamard_stages.hpp — the butterfly sequence of the block Hadamard rotation, for a wave whose lane l holds N consecutive columns
// from l · N of a run of 64 · N columns in VGPRs (mtq_hadamard.hip has the layout and the contract).  One sequence for every kernel that
// rotates: hadamard_rows_kernel and the X prologue of the packed skinny kernels (mtq_packed.hip) include it, so their bits cannot drift
// apart.  Every function needs EXEC all ones: the cross-lane stages read the partner's registers.
// The two files are built differently (mtq_hadamard.hip with the packed float32 forms off, mtq_packed.hip with them on, both with
// -ffp-contract=off) and must still agree to the bit: every operation here is ONE float32 add, subtract or multiply, which every
// form of the instruction rounds alike.  Keep it so - no multiply feeding an add or subtract that a compiler may contract, no
// fma, no reassociation; tests/test_packed_prologue_gpu.py compares the two builds' bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace mtq {
namespace had {

__device__ __forceinline__ float bits_f(uint32_t v) { return __uint_as_float(v); }

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v)
{
    return bits_f((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xF, 0xF, true));
}

// the value of lane ^ D, D inside a DPP row
template <int D>
__device__ __forceinline__ float partner(float v)
{
    if constexpr (D == 1) return dpp_f<0xB1>(v);                 // quad_perm [1, 0, 3, 2]
    else if constexpr (D == 2) return dpp_f<0x4E>(v);            // quad_perm [2, 3, 0, 1]
    else if constexpr (D == 4) return dpp_f<0x1B>(dpp_f<0x141>(v));   // row_half_mirror (i ^ 7), then quad_perm [3, 2, 1, 0] (i ^ 3)
    else return dpp_f<0x128>(v);                                 // row_ror:8 (i ^ 8 in a row of 16)
}

// lanes l and l ^ D, l & D == 0, hold a and b → a + b and a − b.  flip: the sign bit where lane & D.
template <int D, int N>
__device__ __forceinline__ void row_stage(float (&v)[N], uint32_t flip)
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = partner<D>(v[i]) + bits_f(__float_as_uint(v[i]) ^ flip);
}

// the same for D = 16 (HALF = false: the odd rows of the first operand change places with the even rows of the second) and D = 32
// (HALF = true: the upper half of the first with the lower half of the second), two registers at a time
template <bool HALF, int N>
__device__ __forceinline__ void swap_stage(float (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; i += 2) {
        const uint32_t a = __float_as_uint(v[i]), b = __float_as_uint(v[i + 1]);
        const auto r = HALF ? __builtin_amdgcn_permlane32_swap(a, b, false, false) : __builtin_amdgcn_permlane16_swap(a, b, false, false);
        // r[0]: the lower partners' a, then their b, in the upper partners' lanes; r[1]: the upper partners' a in the lower lanes, then b
        const float lo = bits_f(r[0]), hi = bits_f(r[1]);
        const uint32_t s = __float_as_uint(lo + hi), d = __float_as_uint(lo - hi);
        const auto q = HALF ? __builtin_amdgcn_permlane32_swap(s, d, false, false) : __builtin_amdgcn_permlane16_swap(s, d, false, false);
        v[i] = bits_f(q[0]);
        v[i + 1] = bits_f(q[1]);
    }
}

// The whole rotation of the wave's run: log2(N) register stages (stride 1 first), lane_stages = log2(B / N) in 1..6 cross-lane stages,
// then the one multiply by `scale`.  lane_stages is wave-uniform.
template <int N>
__device__ __forceinline__ void rotate_lanes(float (&v)[N], int lane, int lane_stages, float scale)
{
    const uint32_t flip1 = (uint32_t)(lane & 1) << 31, flip2 = (uint32_t)(lane & 2) << 30, flip4 = (uint32_t)(lane & 4) << 29,
                   flip8 = (uint32_t)(lane & 8) << 28;
#pragma unroll
    for (int h = 1; h < N; h <<= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (!(i & h)) {
                const float a = v[i], b = v[i + h];
                v[i] = a + b;
                v[i + h] = a - b;
            }
        }
    }
    row_stage<1, N>(v, flip1);
    if (lane_stages > 1) row_stage<2, N>(v, flip2);
    if (lane_stages > 2) row_stage<4, N>(v, flip4);
    if (lane_stages > 3) row_stage<8, N>(v, flip8);
    if (lane_stages > 4) swap_stage<false, N>(v);
    if (lane_stages > 5) swap_stage<true, N>(v);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] *= scale;
}

// float32(2^(−p/2)) for B = 2^p, and the number of cross-lane stages at N columns a lane (host)
inline float block_scale(int64_t block)
{
    int p = 0;
    while (((int64_t)1 << p) < block) ++p;
    return (float)std::ldexp((p & 1) ? std::sqrt(0.5) : 1.0, -(p / 2));
}

inline int lane_stages(int64_t block, int n)
{
    int s = 0;
    while (((int64_t)n << s) < block) ++s;
    return s;
}

} // namespace had
} // namespace mtq
