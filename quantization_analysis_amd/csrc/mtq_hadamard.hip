// mtq_hadamard.hip — block Hadamard rotation of matrix rows (quantization_analysis_amd/hadamard.py holds the contract).
//
// mtq_hadamard_rows: every aligned block of B = 2^p consecutive columns of every row becomes fl32(S · c_p), S = x_block · H_B with H_B
//   the Sylvester–Hadamard matrix in natural order, formed by p stages of float32 add/sub butterflies in a fixed order (stride 1 first),
//   c_p = float32(2^(−p/2)) applied as one float32 multiply after the last stage.  Output float32, or bf16 by RNE of that float32; an
//   optional second bf16 output yq = mtq_quantize_rows_bf16(y, fmt) of the bf16 y, bit for bit, from the same registers.
//   * No workgroup cooperation and no LDS: one wave owns one segment of 64 · N consecutive columns of one row, lane l the N consecutive
//     columns from l · N, in VGPRs.  N = 16 for B <= 1024 (a segment holds 1024 / B whole blocks), 32 for B = 2048, 64 for B = 4096 (a
//     segment is one block).  An in-place FWHT leaves output i where input i was, so a lane's registers are whole 16-groups of the BFP
//     twin: the twin needs no cross-lane work.
//   * Strides below N are register butterflies (one add or subtract per element and stage).
//   * Strides N · d, d = 1, 2, 4, 8 cross lanes inside a 16-lane DPP row: the lane flips its own sign where lane & d and adds the
//     partner's value, fetched by the add's DPP operand (quad_perm for d = 1, 2; row_ror:8 for d = 8; d = 4 is row_half_mirror followed
//     by a reversed quad_perm, one move more).
//   * d = 16 and d = 32 use v_permlane16_swap / v_permlane32_swap on a PAIR of a lane's registers: one swap brings the lower partners of
//     both registers into one and the upper partners into the other, one add and one subtract form all sums and differences, and a
//     second swap puts them back in place — two operations per element, no sign flip and no select.
//   * Stages with stride >= B are skipped (B = 32 runs one cross-lane stage, B >= 1024 all six); the count is wave-uniform.
//   A ragged last segment (k = 3 · B with B < 1024) masks whole lanes: k is a multiple of 32, so a lane's 16 columns are inside or
//   outside together, and a block is inside or outside as a whole; masked lanes compute on zeros (EXEC stays full for the DPP and swap
//   stages) and store nothing.  A wave loads its whole segment before it stores, so y == x is allowed.  No atomics: equal inputs give
//   equal bits.  The file is compiled with the packed float32 VALU forms off, as mtq_gptq_transpose.hip is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "mtq_device.hpp"
#include "mtq_error.hpp"
#include "mtq_hadamard_stages.hpp"

namespace mtq {
namespace {

constexpr int kHadWaves = 4;                      // independent waves per workgroup
constexpr int64_t kHadMaxBlocks = 1 << 20;        // waves walk the segments beyond that

using had::bits_f;

template <int N>
__device__ __forceinline__ void load_lane(const uint16_t *p, bool vec, float (&v)[N])
{
    if (vec) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int j = 0; j < N / 8; ++j) {
            const uint4 a = q[j];
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[8 * j + 2 * i] = bits_f(w[i] << 16); v[8 * j + 2 * i + 1] = bits_f(w[i] & 0xFFFF0000u); }
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = bits_f((uint32_t)p[i] << 16);
    }
}

template <int N>
__device__ __forceinline__ void load_lane(const float *p, bool vec, float (&v)[N])
{
    if (vec) {
        const float4 *q = reinterpret_cast<const float4 *>(p);
#pragma unroll
        for (int j = 0; j < N / 4; ++j) { const float4 a = q[j]; v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w; }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    }
}

// u: float32 words whose low 16 bits are zero
template <int N>
__device__ __forceinline__ void store_lane(uint16_t *p, bool vec, const uint32_t (&u)[N])
{
    if (vec) {
        uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
        for (int j = 0; j < N / 8; ++j)
            q[j] = make_uint4((u[8 * j] >> 16) | u[8 * j + 1], (u[8 * j + 2] >> 16) | u[8 * j + 3], (u[8 * j + 4] >> 16) | u[8 * j + 5],
                              (u[8 * j + 6] >> 16) | u[8 * j + 7]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = (uint16_t)(u[i] >> 16);
    }
}

template <int N>
__device__ __forceinline__ void store_lane(float *p, bool vec, const float (&v)[N])
{
    if (vec) {
        float4 *q = reinterpret_cast<float4 *>(p);
#pragma unroll
        for (int j = 0; j < N / 4; ++j) q[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}

// One 16-group of bf16 words → its BFP image of format F (1..3), the arithmetic of mtq_output_error.hip's quant_bits: the group's
// constants and the add-and-subtract rounding for a shared exponent in [80, 180], the literal uint32 route outside it.
template <int F>
__device__ __forceinline__ void quantize_group(const uint32_t *u, uint32_t *o)
{
    constexpr uint32_t M = F == 1 ? 7u : (F == 2 ? 3u : 1u);
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) m = max(m, u[i] & 0x7F800000u);
    const uint32_t E = m >> 23;
    if ((E - 80u) <= 100u) {
        const float k_align = bits_f((277u - E) << 23), k_back = bits_f((E - 23u) << 23);
        const float c = bits_f(((E + 24u - M) << 23) | 0x400000u);
        const float ymax = (float)((1u << M) - 1u) * bits_f((E - (M - 1u)) << 23);
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const float xs = __builtin_truncf(bits_f(u[i]) * k_align) * k_back;
            const float r = (xs + c) - c;
            o[i] = __float_as_uint(__builtin_amdgcn_fmed3f(r, -ymax, ymax));
        }
    } else {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) o[i] = bfp_elem_bits_rt(u[i], E, M);
    }
}

// TI, TO: uint16_t (bf16) or float.  N: columns per lane.  QF: 0, or the twin's format code (TO must be bf16).
// lane_stages: log2(B / N), 1..6.  vec bits: 1 x, 2 y, 4 yq may use 16-byte accesses.
template <typename TI, typename TO, int N, int QF>
__global__ __launch_bounds__(64 * kHadWaves) void hadamard_rows_kernel(const TI *x, int64_t k, int64_t ldx, int lane_stages, float scale, TO *y,
                                                                        int64_t ldy, uint16_t *yq, int64_t ldq, int vec, int64_t nseg,
                                                                        int64_t units)
{
    const int lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * kHadWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * kHadWaves;
    for (int64_t u = first; u < units; u += step) {
        const int64_t row = u / nseg, col = (u - row * nseg) * (64 * N) + (int64_t)lane * N;
        const bool live = col < k;
        float v[N];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = 0.0f;
        if (live) load_lane<N>(x + row * ldx + col, (vec & 1) != 0, v);
        had::rotate_lanes<N>(v, lane, lane_stages, scale);
        if constexpr (sizeof(TO) == 4) {
            if (live) store_lane<N>(y + row * ldy + col, (vec & 2) != 0, v);
        } else {
            uint32_t w[N];
#pragma unroll
            for (int i = 0; i < N; ++i) w[i] = bf16_round_bits(__float_as_uint(v[i]));
            if (live) store_lane<N>(y + row * ldy + col, (vec & 2) != 0, w);
            if constexpr (QF != 0) {
                uint32_t o[N];
#pragma unroll
                for (int g = 0; g < N / kGroup; ++g) quantize_group<QF>(w + g * kGroup, o + g * kGroup);
                if (live) store_lane<N>(yq + row * ldq + col, (vec & 4) != 0, o);
            }
        }
    }
}

struct HadArgs {
    const void *x;
    int64_t k, ldx;
    int lane_stages;
    float scale;
    void *y;
    int64_t ldy;
    uint16_t *yq;
    int64_t ldq;
    int vec;
    int64_t nseg, units;
    hipStream_t st;
};

template <typename TI, typename TO, int N, int QF>
void launch_one(const HadArgs &a)
{
    const int64_t blocks = std::min<int64_t>((a.units + kHadWaves - 1) / kHadWaves, kHadMaxBlocks);
    hipLaunchKernelGGL((hadamard_rows_kernel<TI, TO, N, QF>), dim3((unsigned)blocks), dim3(64 * kHadWaves), 0, a.st, static_cast<const TI *>(a.x),
                       a.k, a.ldx, a.lane_stages, a.scale, static_cast<TO *>(a.y), a.ldy, a.yq, a.ldq, a.vec, a.nseg, a.units);
}

template <typename TI, typename TO, int QF>
void launch_n(int n, const HadArgs &a)
{
    if (n == 16) launch_one<TI, TO, 16, QF>(a);
    else if (n == 32) launch_one<TI, TO, 32, QF>(a);
    else launch_one<TI, TO, 64, QF>(a);
}

template <typename TI>
void launch_out(bool y_f32, int qf, int n, const HadArgs &a)
{
    if (y_f32) return launch_n<TI, float, 0>(n, a);
    switch (qf) {
    case 0: return launch_n<TI, uint16_t, 0>(n, a);
    case MTQ_FMT_BFP8: return launch_n<TI, uint16_t, 1>(n, a);
    case MTQ_FMT_BFP4: return launch_n<TI, uint16_t, 2>(n, a);
    default: return launch_n<TI, uint16_t, 3>(n, a);
    }
}

bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}

bool vec16(const void *p, int64_t ld, int64_t esz) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * esz) % 16 == 0; }

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" int mtq_hadamard_rows(const void *x, int x_dtype, int64_t rows, int64_t k, int64_t ldx, int64_t block, void *y, int y_dtype,
                                 int64_t ldy, void *yq, int q_fmt, int64_t ldq, void *stream)
{
    if (!x || !y) return fail(MTQ_ERR_INVALID, "null argument");
    if (x_dtype != MTQ_DTYPE_BF16 && x_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "x_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (y_dtype != MTQ_DTYPE_BF16 && y_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "y_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (yq && (q_fmt < MTQ_FMT_BFP8 || q_fmt > MTQ_FMT_BFP2)) return fail(MTQ_ERR_UNSUPPORTED, "the twin's format code must be 1..3 (bfp8,bfp4,bfp2)");
    if (block < 32 || block > 4096 || (block & (block - 1)) != 0) return fail(MTQ_ERR_INVALID, "block must be a power of two in [32, 4096]");
    if (rows <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "rows and k must be positive (empty tensors are handled by the caller)");
    if (k % block != 0) return fail(MTQ_ERR_INVALID, "k is not a multiple of block");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldy < k) return fail(MTQ_ERR_INVALID, "ldy < k");
    if (yq && ldq < k) return fail(MTQ_ERR_INVALID, "ldq < k");
    if (yq && y_dtype != MTQ_DTYPE_BF16) return fail(MTQ_ERR_INVALID, "the quantised twin needs a bf16 y");
    if (rows > (int64_t)1 << 40 || k > (int64_t)1 << 30 || ldx > (int64_t)1 << 40 || ldy > (int64_t)1 << 40 || ldq > (int64_t)1 << 40)
        return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t xsz = x_dtype == MTQ_DTYPE_F32 ? 4 : 2, ysz = y_dtype == MTQ_DTYPE_F32 ? 4 : 2;
    const int64_t xb = ((rows - 1) * ldx + k) * xsz, yb = ((rows - 1) * ldy + k) * ysz, qb = ((rows - 1) * ldq + k) * 2;
    if (!(x == y && xsz == ysz && ldx == ldy) && overlap(x, xb, y, yb))
        return fail(MTQ_ERR_INVALID, "x and y overlap (only y == x with equal dtype and stride is allowed)");
    if (yq && (overlap(yq, qb, x, xb) || overlap(yq, qb, y, yb))) return fail(MTQ_ERR_INVALID, "yq overlaps x or y");
    if (int rc = require_device()) return rc;

    const int n = block <= 1024 ? 16 : (int)(block / 64);
    HadArgs a;
    a.x = x; a.k = k; a.ldx = ldx; a.lane_stages = had::lane_stages(block, n);
    a.scale = had::block_scale(block);
    a.y = y; a.ldy = ldy; a.yq = static_cast<uint16_t *>(yq); a.ldq = ldq;
    a.vec = (vec16(x, ldx, xsz) ? 1 : 0) | (vec16(y, ldy, ysz) ? 2 : 0) | (yq && vec16(yq, ldq, 2) ? 4 : 0);
    a.nseg = (k + 64 * n - 1) / (64 * n);
    a.units = rows * a.nseg;
    a.st = static_cast<hipStream_t>(stream);
    if (x_dtype == MTQ_DTYPE_F32) launch_out<float>(y_dtype == MTQ_DTYPE_F32, yq ? q_fmt : 0, n, a);
    else launch_out<uint16_t>(y_dtype == MTQ_DTYPE_F32, yq ? q_fmt : 0, n, a);
    return check_launch("mtq_hadamard_rows");
}
