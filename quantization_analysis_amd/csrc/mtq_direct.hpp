// mtq_direct.hpp — the exact (reduced-arithmetic) group sums of K1 on the row layout (mtq_direct.hip) and the column-group
// layout (mtq_transpose.hip): one shared-exponent group of 16 values → its float64 sums, bit for bit what the literal route
// (group_terms_literal, mtq_device.hpp) gives for every group whose shared exponent lies in [80,180].
//
// Same records as the literal route, bit for bit.  Per main-class element (within 14 binades of the group's shared
// exponent E; include/mtq.h's summation order) the literal route does, per BFP format: uint32 decode / align / round /
// re-encode (~25 ops), four float32 terms, four float64 accumulations and a float64 max.  Here:
//   * the aligned 24-bit mantissa is ONE multiply + truncating convert: a = trunc(|x|·2^(150−E)) (exact scaling);
//   * q = RNE of `a` to M bits with saturation in 5 integer ops; |y| = float(q)·2^(E−127−(M−1)) (exact, E ≥ 80);
//   * x and y share their sign, so x·y = |x|·|y| and |x−y| = ||x|−|y||: the float32 products / differences the
//     reference rounds are formed by the same float32 instructions on the magnitudes;
//   * Σy and Σy² of a BFP format are sums of ≤ 16 integers (|q| ≤ 127, q² ≤ 16129) times one power of two: exact
//     in float32, so they are accumulated with float32 add / fma and widened once per group;
//   * Σxy and Σ|x−y| keep their float64 accumulators and the element order of the literal route;
//   * tail-class elements are masked to +0 in the main pass (adding +0.0 changes no accumulator) and, when a lane
//     holds a non-zero one (rare), added afterwards in index order into separate tail sums: S = S_main + S_tail.
// A group whose E lies outside [80,180] (and is not all-zero) sets `bad`: the caller takes the literal route for its tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtq_device.hpp"

namespace mtq {

constexpr int kMaxSums = 2 + 4 * kNumFmt;                         // Σx, Σx², 4 × (Σy, Σy², Σxy, Σ|d|)

__host__ __device__ constexpr int popc4(uint32_t m) { return (int)((m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u)); }

__device__ __forceinline__ float u2f(uint32_t v) { return __uint_as_float(v); }
__device__ __forceinline__ uint32_t f2u(float v) { return __float_as_uint(v); }

typedef float f2 __attribute__((ext_vector_type(2)));

// m = max(m, |a|, |b|) in one instruction (inputs are never NaN on the exact route).
__device__ __forceinline__ void max3_abs(float &m, float a, float b) { asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b)); }

// One BFP format of two neighbouring main-class elements.  xs = the values truncated to the group's 24-bit window
// (±a·2^(E−150), 0 for masked elements), xm = the values themselves, C = 1.5·2^(E−103−M): adding and subtracting C
// rounds xs to the nearest multiple of the format's step 2^(E−126−M), ties to the even multiple — the reference's RNE on
// the truncated aligned mantissa (quantization_formats.py:133-140; C is an even multiple of the step and |xs| < C/3, so
// the sum stays inside one binade of C) — and the clamp is its saturating round-up (:141).  y carries x's sign.
__device__ __forceinline__ void bfp_pair(f2 xs, f2 xm, float C, float ymax, f2 &sy, f2 &sy2, double &sxy, double &sab, float &mx)
{
    const f2 r = (xs + C) - C;
    f2 ys;
    ys.x = __builtin_amdgcn_fmed3f(r.x, -ymax, ymax);
    ys.y = __builtin_amdgcn_fmed3f(r.y, -ymax, ymax);
    sy += ys;                                                    // exact: |Σ q| < 2^11 steps
    sy2 = __builtin_elementwise_fma(ys, ys, sy2);                // exact: Σ q² < 2^18 steps²
    const f2 p = xm * ys;                                        // float32 products (mixed_tile_greedy.py:161), ≥ 0
    sxy += (double)p.x;
    sxy += (double)p.y;
    const f2 d = xm - ys;                                        // :163
    sab += (double)fabsf(d.x);
    sab += (double)fabsf(d.y);
    max3_abs(mx, d.x, d.y);
}

// bf16 candidates of two float32 values: the hardware's RNE convert equals the integer form of
// quantization_formats.py:29-45 for every finite normal value (all a main-class element can be).
__device__ __forceinline__ f2 bf16_round_pair(f2 x)
{
    uint32_t pk;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(x.x), "v"(x.y));
    f2 y;
    y.x = u2f(pk << 16);
    y.y = u2f(pk & 0xFFFF0000u);
    return y;
}

// Group sums of one lane.  s[0..1] = Σx, Σx²; s[2+4j .. 5+4j] = Σy, Σy², Σxy, Σ|x−y| of the j-th requested format
// (ascending format code); mx[j] its max|x−y|.  `bad` = the exact route does not apply (the tile is redone).
template <uint32_t FM, bool kBf16Storage>
__device__ __forceinline__ void direct_group(const uint32_t (&u)[kGroup], double (&s)[kMaxSums], float (&mx)[kNumFmt], bool &bad)
{
    constexpr bool f0 = (FM & 1u) != 0, f8 = (FM & 2u) != 0, f4 = (FM & 4u) != 0, f2_ = (FM & 8u) != 0;
    constexpr int j0 = 0, j8 = popc4(FM & 1u), j4 = popc4(FM & 3u), j2 = popc4(FM & 7u);

    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) m = max(m, u[i] & 0x7FFFFFFFu);
    const uint32_t E = m >> 23;                                   // shared exponent (:118-119)
    const bool out_of_range = (E - 80u) > 100u;
    bad = out_of_range && m != 0u;
    const uint32_t Es = out_of_range ? 127u : E;                  // keeps the constants finite; results unused / all zero then
    const float k_align = u2f((277u - Es) << 23);                 // 2^(150−E): x → units of the window's last bit
    const float k_back = u2f((Es - 23u) << 23);                   // 2^(E−150)
    const float tail_thr = u2f((Es - 14u) << 23);                 // smallest main-class magnitude 2^(E−14−127)
    const float c8 = u2f(((Es + 17u) << 23) | 0x400000u), c4 = u2f(((Es + 21u) << 23) | 0x400000u), c2 = u2f(((Es + 23u) << 23) | 0x400000u);
    const float ymax8 = 127.0f * u2f((Es - 6u) << 23), ymax4 = 7.0f * u2f((Es - 2u) << 23), ymax2 = u2f(Es << 23);

    double sx = 0.0, sx2 = 0.0, y0 = 0.0, y02 = 0.0, xy0 = 0.0, ab0 = 0.0;
    double xy8 = 0.0, ab8 = 0.0, xy4 = 0.0, ab4 = 0.0, xy2 = 0.0, ab2 = 0.0;
    f2 sy8 = {0.0f, 0.0f}, sy82 = {0.0f, 0.0f}, sy4 = {0.0f, 0.0f}, sy42 = {0.0f, 0.0f}, sy2 = {0.0f, 0.0f}, sy22 = {0.0f, 0.0f};
    float m0 = 0.0f, m8 = 0.0f, m4 = 0.0f, m2 = 0.0f;
    uint32_t tail_or = 0u;
#pragma unroll
    for (int i = 0; i < kGroup; i += 2) {
        const uint32_t ua = fabsf(u2f(u[i])) < tail_thr ? 0u : u[i];          // tail class (zeros included) → +0 in the main pass
        const uint32_t ub = fabsf(u2f(u[i + 1])) < tail_thr ? 0u : u[i + 1];
        tail_or |= (u[i] ^ ua) | (u[i + 1] ^ ub);
        const f2 xm = {u2f(ua), u2f(ub)};
        sx += (double)xm.x;
        sx += (double)xm.y;
        const f2 xx = xm * xm;
        sx2 += (double)xx.x;
        sx2 += (double)xx.y;
        if (f0 && !kBf16Storage) {                                             // bf16 candidate of a float32 value (:29-45)
            const f2 yv = bf16_round_pair(xm);
            y0 += (double)yv.x;
            y0 += (double)yv.y;
            const f2 yy = yv * yv, xy = xm * yv, dd = xm - yv;
            y02 += (double)yy.x;
            y02 += (double)yy.y;
            xy0 += (double)xy.x;
            xy0 += (double)xy.y;
            ab0 += (double)fabsf(dd.x);
            ab0 += (double)fabsf(dd.y);
            max3_abs(m0, dd.x, dd.y);
        }
        if (f8 || f4 || f2_) {
            const f2 t = xm * k_align;                                         // exact scaling; integer part = aligned mantissa man >> d (:121-131)
            f2 at;
            at.x = __builtin_truncf(t.x);
            at.y = __builtin_truncf(t.y);
            const f2 xs = at * k_back;                                         // x truncated to the group's 24-bit window
            if (f8) bfp_pair(xs, xm, c8, ymax8, sy8, sy82, xy8, ab8, m8);
            if (f4) bfp_pair(xs, xm, c4, ymax4, sy4, sy42, xy4, ab4, m4);
            if (f2_) bfp_pair(xs, xm, c2, ymax2, sy2, sy22, xy2, ab2, m2);
        }
    }
    if (kBf16Storage) { y0 = sx; y02 = sx2; xy0 = sx2; }                       // y == x: the same float32 terms in the same order

    if ((tail_or << 1) != 0u) {                                                // a non-zero tail element in this lane (divergent, rare)
        double tx = 0.0, tx2 = 0.0, ty0 = 0.0, ty02 = 0.0, txy0 = 0.0, tab0 = 0.0, tab = 0.0;
        float tmx = 0.0f;
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const float xv = u2f(u[i]);
            if (fabsf(xv) < tail_thr) {                                        // zeros add +0.0 everywhere: harmless
                tx += (double)xv;
                const float xx = xv * xv;
                tx2 += (double)xx;
                const float ax = fabsf(xv);
                tab += (double)ax;                                             // every BFP format gives y = +0 this far below the maximum
                tmx = fmaxf(tmx, ax);
                if (f0 && !kBf16Storage) {
                    const float yv = u2f(bf16_round_bits(u[i]));
                    ty0 += (double)yv;
                    ty02 += (double)(yv * yv);
                    txy0 += (double)(xv * yv);
                    const float df = fabsf(xv - yv);
                    tab0 += (double)df;
                    m0 = fmaxf(m0, df);
                }
            }
        }
        sx = sx + tx; sx2 = sx2 + tx2;
        if (kBf16Storage) { y0 = sx; y02 = sx2; xy0 = sx2; }
        else { y0 = y0 + ty0; y02 = y02 + ty02; xy0 = xy0 + txy0; ab0 = ab0 + tab0; }
        ab8 = ab8 + tab; ab4 = ab4 + tab; ab2 = ab2 + tab;
        m8 = fmaxf(m8, tmx); m4 = fmaxf(m4, tmx); m2 = fmaxf(m2, tmx);
    }

    s[0] = sx; s[1] = sx2;
    if (f0) { s[2 + 4 * j0] = y0; s[3 + 4 * j0] = y02; s[4 + 4 * j0] = xy0; s[5 + 4 * j0] = ab0; mx[j0] = m0; }
    if (f8) { s[2 + 4 * j8] = (double)(sy8.x + sy8.y); s[3 + 4 * j8] = (double)(sy82.x + sy82.y); s[4 + 4 * j8] = xy8; s[5 + 4 * j8] = ab8; mx[j8] = m8; }
    if (f4) { s[2 + 4 * j4] = (double)(sy4.x + sy4.y); s[3 + 4 * j4] = (double)(sy42.x + sy42.y); s[4 + 4 * j4] = xy4; s[5 + 4 * j4] = ab4; mx[j4] = m4; }
    if (f2_) { s[2 + 4 * j2] = (double)(sy2.x + sy2.y); s[3 + 4 * j2] = (double)(sy22.x + sy22.y); s[4 + 4 * j2] = xy2; s[5 + 4 * j2] = ab2; mx[j2] = m2; }
}

} // namespace mtq
