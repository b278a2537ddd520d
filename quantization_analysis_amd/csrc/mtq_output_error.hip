// mtq_output_error.hip — LOE: the layer-output error of quantised weights on recorded activations.
//
// Y_f = X·Ŵ_fᵀ (+ b) for every candidate f against R = X·Wᵀ (+ b), in one pass over X and W, reduced to the seven float64 sums
// mtq_columns_from_sums takes; neither Ŵ nor Y is written.  X is bf16 (M × K), W is N × K (bf16 or float32) in the nn.Linear convention.
//
// Tiling: a workgroup of 4 waves owns a 128 (M) × 64 (N) output block and walks K in steps of 64.  Per step
//   * X: 128 × 64 bf16 → LDS;
//   * W: 64 rows × 64 = 256 groups of 16 → one lane per group computes the group's shared exponent once and writes a bf16 LDS image of
//     its 16 values for each candidate (bfp8 / bfp4 / bfp2 / map) and for the reference (hi = bf16(W); for float32 W also mid = bf16(W − hi)
//     and lo = bf16(W − hi − mid), which is exact: hi + mid + lo = W for |W| ≥ 2^-100).  Every BFP value has its low 16 bits zero, so each
//     image is exact in bf16 and the MFMA forms every product exactly; only the f32 accumulation rounds.
//   * each wave: 32 M rows × 64 N columns (2 subtiles of mfma_f32_32x32x16_bf16) per accumulator; one A fragment of X feeds them all.
// Accumulators: hi (the reference for bf16 W and the bf16 candidate for both: bf16(W) = hi), res (mid + lo, float32 W only), bfp8,
// bfp4, bfp2, map.  Epilogue: r = hi + res + b, q_f = acc_f + b, in f32; the sums of (r, q) in float64 per lane, then a fixed-order
// reduction over the workgroup into one partial record per workgroup, and a second kernel adds the records in index order into `sums`
// (no float atomics: the same inputs give the same bits).
//
// Activation formats (mtq_output_error_qx): the candidates see Q(X), a bf16 image of the BFP-quantised activations that the row pre-pass
// quantize_rows_bf16 writes once per chunk (exact: a BFP value has at most 8 significant bits), while R keeps X.  The QX instantiations
// stage the Q(X) tile beside X in LDS and take their A fragment for bfp8 / bfp4 / bfp2 / map from it; the bf16 candidate gets an
// accumulator of its own (Q(X)·hi), since hi is R's.  There the float32-W flag is a compile-time property of T, so the bf16-W
// instantiation holds no res accumulator.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kBM = 128, kBN = 64, kBK = 64, kThreads = 256;
constexpr int kLdk = kBK + 8;                      // LDS row pitch in bf16 (144 B: 16-B fragment reads of 32 rows spread over the banks)
constexpr int kImgHi = 0, kImgMid = 1, kImgLo = 2, kImgB8 = 3, kImgB4 = 4, kImgB2 = 5, kImgMap = 6, kNumImg = 7;
constexpr int kSlots = 7;                          // bf16, bfp8, bfp4, bfp2, map, fp0, recorded
constexpr int kRecord = 2 + 5 * kSlots;            // Σr, Σr², then Σq, Σq², Σrq, Σ|r−q|, max|r−q| per slot
constexpr int kLdsBytes = (kBM + kNumImg * kBN) * kLdk * 2;
constexpr int kLdsBytesQx = kLdsBytes + kBM * kLdk * 2;   // + the Q(X) tile

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bits_f(uint32_t v) { return __uint_as_float(v); }

// One BFP element by the group's constants (mtq_direct.hpp bfp_pair): xs = x truncated to the group's 24-bit window.
__device__ __forceinline__ uint32_t bfp_fast(float xs, float C, float ymax)
{
    const float r = (xs + C) - C;
    return __float_as_uint(__builtin_amdgcn_fmed3f(r, -ymax, ymax));
}

struct GroupConsts {
    float k_align, k_back, c[4], ymax[4];
};

__device__ __forceinline__ GroupConsts group_consts(uint32_t E)
{
    GroupConsts g;
    g.k_align = bits_f((277u - E) << 23);
    g.k_back = bits_f((E - 23u) << 23);
#pragma unroll
    for (int f = 1; f <= 3; ++f) {
        const uint32_t M = f == 1 ? 7u : (f == 2 ? 3u : 1u);
        g.c[f] = bits_f(((E + 24u - M) << 23) | 0x400000u);
        g.ymax[f] = (float)((1u << M) - 1u) * bits_f((E - (M - 1u)) << 23);
    }
    g.c[0] = g.ymax[0] = 0.0f;
    return g;
}

// y bits of format f (0..3; anything else → +0, as K3) for element u of a group with shared exponent E; fast = E in [80, 180].
__device__ __forceinline__ uint32_t quant_bits(int f, uint32_t u, uint32_t E, bool fast, const GroupConsts &g)
{
    if (f == 0) return bf16_round_bits(u);
    if (f < 1 || f > 3) return 0u;
    if (fast) {
        const float xs = __builtin_truncf(bits_f(u) * g.k_align) * g.k_back;
        return bfp_fast(xs, g.c[f], g.ymax[f]);
    }
    return bfp_elem_bits_rt(u, E, f == 1 ? 7u : (f == 2 ? 3u : 1u));
}

__device__ __forceinline__ void store_image(uint16_t *dst, const uint32_t (&y)[kGroup])
{
    uint32_t pk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pk[i] = (y[2 * i] >> 16) | (y[2 * i + 1] & 0xFFFF0000u);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    d[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    d[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
}

// One W group → every image the launch needs.  imask: bit i = image i is used.
__device__ __forceinline__ void stage_w_group(const uint32_t (&u)[kGroup], int64_t n, int64_t k, int64_t N, int64_t K,
                                              uint32_t imask, const int8_t *__restrict__ map, int64_t map_w, uint16_t *img0, int img_off)
{
    const uint32_t E = group_shared_exp(u);
    const bool fast = (E - 80u) <= 100u;
    const GroupConsts g = group_consts(fast ? E : 127u);
    uint32_t y[kGroup];
    constexpr int kImgElems = kBN * kLdk;
    {   // hi (and mid / lo for float32 storage)
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
        store_image(img0 + kImgHi * kImgElems + img_off, y);
        if (imask & (1u << kImgMid)) {
            uint32_t r1[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const float d1 = bits_f(u[i]) - bits_f(y[i]);            // exact
                r1[i] = bf16_round_bits(__float_as_uint(d1));
                y[i] = __float_as_uint(d1 - bits_f(r1[i]));              // exact, at most 8 significant bits
            }
            store_image(img0 + kImgMid * kImgElems + img_off, r1);
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(y[i]);
            store_image(img0 + kImgLo * kImgElems + img_off, y);
        }
    }
#pragma unroll
    for (int f = 1; f <= 3; ++f) {
        const int im = kImgB8 + f - 1;
        if (imask & (1u << im)) {                                        // launch-uniform
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = quant_bits(f, u[i], E, fast, g);
            store_image(img0 + im * kImgElems + img_off, y);
        }
    }
    if (imask & (1u << kImgMap)) {
        const int f = (n < N && k < K) ? (int)map[(n / kTile) * map_w + k / kTile] : 4;   // the zero padding of a ragged edge stays zero
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = quant_bits(f, u[i], E, fast, g);
        store_image(img0 + kImgMap * kImgElems + img_off, y);
    }
}

// ---- transposed layout (mtq_output_error_transposed): a group is 16 consecutive rows (N) of one column (k), aligned from row 0.
// The staging keeps the row kernel's ownership — lane tid holds row n0 + tid/4, columns 16·(tid%4) .. +15 — so wave w holds rows
// n0 + 16w .. +15 and element i's group is column k + i over the 16 lanes of the wave with equal lane & 3 (n0 is a multiple of 64).
// Its shared exponent is a max over lane bits 2..5; the constants become per element.  hi / mid / lo and the LDS images are untouched.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// E[i] = the max exponent field of element i over the 16 lanes of the wave with this lane's lane & 3 (EXEC must be full).  Two 8-bit
// fields per dword: the two in-row steps are DPP rotations (row_ror:4, row_ror:8 keep lane & 3), the two cross-row steps lane shuffles.
__device__ __forceinline__ void column_shared_exps(const uint32_t (&u)[kGroup], uint32_t (&E)[kGroup])
{
#pragma unroll
    for (int j = 0; j < kGroup / 2; ++j) {
        uint32_t v = ((u[2 * j] >> 23) & 0xFFu) | (((u[2 * j + 1] >> 23) & 0xFFu) << 16);
        v = pk_max_u16(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false));
        v = pk_max_u16(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false));
        v = pk_max_u16(v, (uint32_t)__shfl_xor((int)v, 16, 64));
        v = pk_max_u16(v, (uint32_t)__shfl_xor((int)v, 32, 64));
        E[2 * j] = v & 0xFFFFu;
        E[2 * j + 1] = v >> 16;
    }
}

// One element by bfp_fast with the constants of its own shared exponent E in [80, 180] (group_consts, per element).
__device__ __forceinline__ uint32_t bfp_fast_elem(uint32_t u, uint32_t E, uint32_t M)
{
    const float xs = __builtin_truncf(bits_f(u) * bits_f((277u - E) << 23)) * bits_f((E - 23u) << 23);
    const float c = bits_f(((E + 24u - M) << 23) | 0x400000u);
    const float ymax = (float)((1u << M) - 1u) * bits_f((E - (M - 1u)) << 23);
    return bfp_fast(xs, c, ymax);
}

// The lane's 16 elements (each of its own column group) → the images the launch needs; map: ceil(N/32) entries per tile row of Wᵀ.
__device__ __forceinline__ void stage_w_group_t(const uint32_t (&u)[kGroup], int64_t n, int64_t k, int64_t N, int64_t K,
                                                uint32_t imask, const int8_t *__restrict__ map, int64_t map_w, uint16_t *img0, int img_off)
{
    uint32_t E[kGroup];
    column_shared_exps(u, E);
    bool fast = true;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) fast = fast && (E[i] - 80u) <= 100u;
    uint32_t y[kGroup];
    constexpr int kImgElems = kBN * kLdk;
    {   // hi (and mid / lo for float32 storage): layout-free, as stage_w_group
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
        store_image(img0 + kImgHi * kImgElems + img_off, y);
        if (imask & (1u << kImgMid)) {
            uint32_t r1[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const float d1 = bits_f(u[i]) - bits_f(y[i]);
                r1[i] = bf16_round_bits(__float_as_uint(d1));
                y[i] = __float_as_uint(d1 - bits_f(r1[i]));
            }
            store_image(img0 + kImgMid * kImgElems + img_off, r1);
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(y[i]);
            store_image(img0 + kImgLo * kImgElems + img_off, y);
        }
    }
#pragma unroll
    for (int f = 1; f <= 3; ++f) {
        const int im = kImgB8 + f - 1;
        if (imask & (1u << im)) {                                        // launch-uniform
            const uint32_t M = f == 1 ? 7u : (f == 2 ? 3u : 1u);
            if (fast) {
#pragma unroll
                for (int i = 0; i < kGroup; ++i) y[i] = bfp_fast_elem(u[i], E[i], M);
            } else {
#pragma unroll
                for (int i = 0; i < kGroup; ++i) y[i] = bfp_elem_bits_rt(u[i], E[i], M);
            }
            store_image(img0 + im * kImgElems + img_off, y);
        }
    }
    if (imask & (1u << kImgMap)) {
        const int f = (n < N && k < K) ? (int)map[(k / kTile) * map_w + n / kTile] : 4;   // the zero padding of a ragged edge stays zero
        const uint32_t M = f == 1 ? 7u : (f == 2 ? 3u : 1u);
        if (f == 0) {
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
        } else if (f < 1 || f > 3) {
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = 0u;
        } else if (fast) {
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = bfp_fast_elem(u[i], E[i], M);
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i) y[i] = bfp_elem_bits_rt(u[i], E[i], M);
        }
        store_image(img0 + kImgMap * kImgElems + img_off, y);
    }
}

// max|r − q| with np.max semantics: a NaN on either side wins (fmax would drop it and report the largest finite difference).
__device__ __forceinline__ double nan_max(double a, double b) { return (a == a && b == b) ? fmax(a, b) : a + b; }

__device__ __forceinline__ void fold(double (&s)[kRecord], int slot, double r, double q)
{
    const double d = fabs(r - q);
    s[2 + 5 * slot] += q;
    s[3 + 5 * slot] += q * q;
    s[4 + 5 * slot] += r * q;
    s[5 + 5 * slot] += d;
    s[6 + 5 * slot] = nan_max(s[6 + 5 * slot], d);
}

// QX: the candidates take their A operand from xq (Q(X), bf16, ldxq) and the bf16 candidate accumulates in acc[6]; !QX ignores xq.
// TR: the transposed layout (stage_w_group_t; map over Wᵀ's grid); everything else is the row kernel's.
template <typename T, bool QX, bool TR>
__global__ __launch_bounds__(kThreads) void output_error_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec,
                                                                const T *__restrict__ w, int64_t N, int64_t ldw, int w_vec,
                                                                const float *__restrict__ bias, uint32_t imask, uint32_t smask,
                                                                const int8_t *__restrict__ map, int64_t map_w,
                                                                const void *__restrict__ rec, int rec_f32, int64_t ldr,
                                                                double *__restrict__ partials,
                                                                const uint16_t *__restrict__ xq, int64_t ldxq, int xq_vec)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[(QX ? kLdsBytesQx : kLdsBytes) / 2];
    __shared__ double red[4][kRecord];
    uint16_t *xs = lds;
    uint16_t *img0 = lds + kBM * kLdk;
    uint16_t *xqs = lds + (kBM + kNumImg * kBN) * kLdk;   // QX only
    constexpr int kImgElems = kBN * kLdk;
    constexpr int kAcc = QX ? 7 : 6;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nblocks = (N + kBN - 1) / kBN;
    const int64_t bm = blockIdx.x / nblocks, bn = blockIdx.x % nblocks;
    const int64_t m0 = bm * kBM, n0 = bn * kBN;
    const bool f32w = QX ? sizeof(T) == 4 : (imask & (1u << kImgMid)) != 0;

    f32x16 acc[kAcc][2];
#pragma unroll
    for (int a = 0; a < kAcc; ++a)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][s][r] = 0.0f;

    // global → registers one K-step ahead: the loads of step k0 + 64 are in flight while the MFMAs of step k0 run
    const int wrow = tid >> 2, wc16 = (tid & 3) * kGroup;
    uint4 xr[4], xqr[QX ? 4 : 1];
    uint32_t wu[kGroup];
    auto load_step = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // X: 128 rows × 64 columns = 1024 pieces of 8 bf16, 4 per thread
            const int p = tid + kThreads * i, row = p >> 3, c8 = (p & 7) * 8;
            const int64_t gm = m0 + row, gk = k0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < M) {
                const uint16_t *src = x + gm * ldx + gk;
                if (x_vec && gk + 8 <= K) {
                    v = *reinterpret_cast<const uint4 *>(src);
                } else {
                    uint32_t h[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) h[j] = gk + j < K ? (uint32_t)src[j] : 0u;
                    v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                }
            }
            xr[i] = v;
        }
        if constexpr (QX) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // Q(X): the same pieces
                const int p = tid + kThreads * i, row = p >> 3, c8 = (p & 7) * 8;
                const int64_t gm = m0 + row, gk = k0 + c8;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (gm < M) {
                    const uint16_t *src = xq + gm * ldxq + gk;
                    if (xq_vec && gk + 8 <= K) {
                        v = *reinterpret_cast<const uint4 *>(src);
                    } else {
                        uint32_t h[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) h[j] = gk + j < K ? (uint32_t)src[j] : 0u;
                        v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                    }
                }
                xqr[i] = v;
            }
        }
        Loader<T>::group(w, n0 + wrow, k0 + wc16, N, K, ldw, w_vec != 0, wu);   // W: lane tid owns group (row tid / 4, columns 16·(tid % 4) ..)
    };
    load_step(0);
    for (int64_t k0 = 0; k0 < K; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + kThreads * i;
            *reinterpret_cast<uint4 *>(xs + (p >> 3) * kLdk + (p & 7) * 8) = xr[i];
            if constexpr (QX) *reinterpret_cast<uint4 *>(xqs + (p >> 3) * kLdk + (p & 7) * 8) = xqr[i];
        }
        if constexpr (TR)
            stage_w_group_t(wu, n0 + wrow, k0 + wc16, N, K, imask, map, map_w, img0, wrow * kLdk + wc16);
        else
            stage_w_group(wu, n0 + wrow, k0 + wc16, N, K, imask, map, map_w, img0, wrow * kLdk + wc16);
        __syncthreads();
        if (k0 + kBK < K) load_step(k0 + kBK);
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) {
            const int koff = kk * 16 + 8 * (lane >> 5);
            const int aoff = (wave * 32 + (lane & 31)) * kLdk + koff;
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xs + aoff);
            const bf16x8 aq = QX ? *reinterpret_cast<const bf16x8 *>(xqs + aoff) : a;   // the candidates' A fragment
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int boff = (s * 32 + (lane & 31)) * kLdk + koff;
#define MTQ_OE_MFMA(ACC, A, IMG) acc[ACC][s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, *reinterpret_cast<const bf16x8 *>(img0 + (IMG) * kImgElems + boff), acc[ACC][s], 0, 0, 0)
                MTQ_OE_MFMA(0, a, kImgHi);
                if (f32w) { MTQ_OE_MFMA(1, a, kImgMid); MTQ_OE_MFMA(1, a, kImgLo); }
                if constexpr (QX) {
                    if (smask & 1u) MTQ_OE_MFMA(kAcc - 1, aq, kImgHi);
                }
                if (imask & (1u << kImgB8)) MTQ_OE_MFMA(2, aq, kImgB8);
                if (imask & (1u << kImgB4)) MTQ_OE_MFMA(3, aq, kImgB4);
                if (imask & (1u << kImgB2)) MTQ_OE_MFMA(4, aq, kImgB2);
                if (imask & (1u << kImgMap)) MTQ_OE_MFMA(5, aq, kImgMap);
#undef MTQ_OE_MFMA
            }
        }
        __syncthreads();
    }

    // epilogue: lane's outputs are (m0 + 32·wave + (r&3) + 8(r>>2) + 4(lane>>5), n0 + 32s + (lane&31))
    double sum[kRecord];
#pragma unroll
    for (int i = 0; i < kRecord; ++i) sum[i] = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t n = n0 + 32 * s + (lane & 31);
        if (n >= N) continue;
        const float b = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= M) continue;
            const float hi = acc[0][s][r];
            const float rf = (f32w ? hi + acc[1][s][r] : hi) + b;
            const double rd = (double)rf;
            sum[0] += rd;
            sum[1] += rd * rd;
            if (smask & 1u) fold(sum, 0, rd, (double)((QX ? acc[kAcc - 1][s][r] : hi) + b));
            if (smask & 2u) fold(sum, 1, rd, (double)(acc[2][s][r] + b));
            if (smask & 4u) fold(sum, 2, rd, (double)(acc[3][s][r] + b));
            if (smask & 8u) fold(sum, 3, rd, (double)(acc[4][s][r] + b));
            if (smask & 16u) fold(sum, 4, rd, (double)(acc[5][s][r] + b));
            if (smask & 32u) fold(sum, 5, rd, (double)b);
            if (smask & 64u) {
                const float q = rec_f32 ? static_cast<const float *>(rec)[m * ldr + n]
                                        : bits_f((uint32_t)static_cast<const uint16_t *>(rec)[m * ldr + n] << 16);
                fold(sum, 6, rd, (double)q);
            }
        }
    }
    // fixed-order reduction: butterfly within the wave (the same tree in every run), then the 4 waves in order
#pragma unroll
    for (int i = 0; i < kRecord; ++i) {
        const bool is_max = i >= 2 && (i - 2) % 5 == 4;
        double v = sum[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_xor(v, o, 64);
            v = is_max ? nan_max(v, t) : v + t;
        }
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (tid < kRecord) {
        const bool is_max = tid >= 2 && (tid - 2) % 5 == 4;
        double v = red[0][tid];
        for (int wv = 1; wv < 4; ++wv) v = is_max ? nan_max(v, red[wv][tid]) : v + red[wv][tid];
        partials[(int64_t)blockIdx.x * kRecord + tid] = v;
    }
}

// sums[slot][7] (+)= the workgroup records in index order: one workgroup per record entry, each thread a strided slice, then a fixed tree.
__global__ __launch_bounds__(256) void output_error_reduce(const double *__restrict__ partials, int64_t nblocks, double *__restrict__ sums,
                                                           uint32_t smask)
{
    __shared__ double buf[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const bool is_max = i >= 2 && (i - 2) % 5 == 4;
    double v = 0.0;
    for (int64_t b = tid; b < nblocks; b += 256) {
        const double p = partials[b * kRecord + i];
        v = is_max ? nan_max(v, p) : v + p;
    }
    buf[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) buf[tid] = is_max ? nan_max(buf[tid], buf[tid + s]) : buf[tid] + buf[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const double t = buf[0];
    if (i < 2) {                                   // Σr, Σr²: shared by every slot
        for (int slot = 0; slot < kSlots; ++slot)
            if (smask & (1u << slot)) sums[slot * 7 + i] += t;
    } else {
        const int slot = (i - 2) / 5, j = 2 + (i - 2) % 5;
        if (smask & (1u << slot)) sums[slot * 7 + j] = j == 6 ? nan_max(sums[slot * 7 + j], t) : sums[slot * 7 + j] + t;
    }
}

// The activation pre-pass: one lane per 16-element group of a bf16 row → Q(X) as bf16, the upper half of K2's float32 y (every BFP value,
// specials included, has its low 16 bits zero; fmt 0 is the identity on bf16 input).  Rows walk gridDim.y; a group past `cols` reads
// zero padding and stores only its live elements.  F is the format code (a template parameter: indexed at run time, the group
// constants would live in LDS).
template <int F>
__global__ __launch_bounds__(256) void quantize_rows_bf16(const uint16_t *__restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                          uint16_t *__restrict__ y, int64_t ldy, int vec_ok, int vec_ok_y)
{
    const int64_t col0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kGroup;
    if (col0 >= cols) return;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        uint32_t u[kGroup];
        Loader<uint16_t>::group(x, row, col0, rows, cols, ld, vec_ok != 0, u);
        const uint32_t E = group_shared_exp(u);
        const bool fast = (E - 80u) <= 100u;
        const GroupConsts g = group_consts(fast ? E : 127u);
        uint32_t o[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) o[i] = quant_bits(F, u[i], E, fast, g);
        uint16_t *yr = y + row * ldy + col0;
        if (col0 + kGroup <= cols && vec_ok_y) {
            store_image(yr, o);
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (col0 + i < cols) yr[i] = (uint16_t)(o[i] >> 16);
        }
    }
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_output_error_scratch_doubles(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0) return 0;
    return (size_t)(((m + kBM - 1) / kBM) * ((n + kBN - 1) / kBN)) * kRecord;
}

// One fused launch and its reduce; QX takes the candidates' A operand from xq, TR the transposed layout.
template <bool QX, bool TR>
static int launch_fused(bool f32w, int64_t blocks, hipStream_t st, const uint16_t *xp, int64_t m, int64_t k, int64_t ldx, int x_vec,
                        const void *w, int64_t n, int64_t ldw, int w_vec, const float *bias, uint32_t imask, uint32_t smask,
                        const int8_t *map, int64_t map_w, const void *recorded, int rec_f32, int64_t ldr, double *sums, double *scratch,
                        const uint16_t *xqp, int64_t ldxq, int xq_vec, const char *what, const char *what_reduce)
{
    const dim3 grid((unsigned)blocks);
    if (f32w)
        hipLaunchKernelGGL((output_error_kernel<float, QX, TR>), grid, dim3(kThreads), 0, st, xp, m, k, ldx, x_vec, static_cast<const float *>(w), n,
                           ldw, w_vec, bias, imask, smask, map, map_w, recorded, rec_f32, ldr, scratch, xqp, ldxq, xq_vec);
    else
        hipLaunchKernelGGL((output_error_kernel<uint16_t, QX, TR>), grid, dim3(kThreads), 0, st, xp, m, k, ldx, x_vec, static_cast<const uint16_t *>(w),
                           n, ldw, w_vec, bias, imask, smask, map, map_w, recorded, rec_f32, ldr, scratch, xqp, ldxq, xq_vec);
    if (int rc = check_launch(what)) return rc;
    hipLaunchKernelGGL(output_error_reduce, dim3(kRecord), dim3(256), 0, st, scratch, blocks, sums, smask);
    return check_launch(what_reduce);
}

// The checks and the launch of the LOE entries; qx = the candidates see xq (mtq_output_error_qx, or mtq_output_error_transposed with a
// non-null xq), tr = the transposed layout (the map over Wᵀ's grid, ceil(n/32) entries per row), otherwise mtq_output_error exactly.
static int launch_output_error(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                               const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                               double *sums, double *scratch, size_t scratch_doubles, void *stream, bool qx, const void *xq, int64_t ldxq,
                               bool tr = false)
{
    if (!x || !w || !sums || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (qx && !xq) return fail(MTQ_ERR_INVALID, "xq is null");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (recorded && rec_dtype != MTQ_DTYPE_BF16 && rec_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "rec_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if ((fmt_mask & ~MTQ_MASK_ALL) != 0) return fail(MTQ_ERR_UNSUPPORTED, "fmt_mask may name only bf16|bfp8|bfp4|bfp2 (bits 0..3)");
    if (m <= 0 || n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "m, n and k must be positive (empty operands are handled by the caller)");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (qx && ldxq < k) return fail(MTQ_ERR_INVALID, "ldxq < k");
    if (recorded && ldr < n) return fail(MTQ_ERR_INVALID, "ldr < n");
    if (m > (int64_t)1 << 40 || n > (int64_t)1 << 30 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t blocks = ((m + kBM - 1) / kBM) * ((n + kBN - 1) / kBN);
    if (blocks > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many workgroups for one launch: pass M in chunks");
    if (scratch_doubles < mtq_output_error_scratch_doubles(m, n)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_output_error_scratch_doubles(m, n)");
    if (int rc = require_device()) return rc;

    const int f32w = w_dtype == MTQ_DTYPE_F32;
    uint32_t imask = 1u << kImgHi;
    if (f32w) imask |= (1u << kImgMid) | (1u << kImgLo);
    for (int f = 1; f <= 3; ++f)
        if (fmt_mask & (1u << f)) imask |= 1u << (kImgB8 + f - 1);
    if (map) imask |= 1u << kImgMap;
    const uint32_t smask = (fmt_mask & MTQ_MASK_ALL) | (map ? 16u : 0u) | 32u | (recorded ? 64u : 0u);
    const int64_t esz = f32w ? 4 : 2;
    const int x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * esz) % 16 == 0;
    const int64_t map_w = tr ? (n + kTile - 1) / kTile : (k + kTile - 1) / kTile;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *xp = static_cast<const uint16_t *>(x), *xqp = static_cast<const uint16_t *>(xq);
    const int rec_f32 = rec_dtype == MTQ_DTYPE_F32;
    const int xq_vec = qx && reinterpret_cast<uintptr_t>(xq) % 16 == 0 && ldxq % 8 == 0;
    if (tr) {
        if (qx)
            return launch_fused<true, true>(f32w, blocks, st, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, bias, imask, smask, map, map_w, recorded,
                                            rec_f32, ldr, sums, scratch, xqp, ldxq, xq_vec, "mtq_output_error_transposed",
                                            "mtq_output_error_transposed (reduce)");
        return launch_fused<false, true>(f32w, blocks, st, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, bias, imask, smask, map, map_w, recorded,
                                         rec_f32, ldr, sums, scratch, nullptr, 0, 0, "mtq_output_error_transposed",
                                         "mtq_output_error_transposed (reduce)");
    }
    if (qx)
        return launch_fused<true, false>(f32w, blocks, st, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, bias, imask, smask, map, map_w, recorded,
                                         rec_f32, ldr, sums, scratch, xqp, ldxq, xq_vec, "mtq_output_error_qx", "mtq_output_error_qx (reduce)");
    return launch_fused<false, false>(f32w, blocks, st, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, bias, imask, smask, map, map_w, recorded,
                                      rec_f32, ldr, sums, scratch, nullptr, 0, 0, "mtq_output_error", "mtq_output_error (reduce)");
}

extern "C" int mtq_output_error(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                                const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                                double *sums, double *scratch, size_t scratch_doubles, void *stream)
{
    return launch_output_error(x, m, k, ldx, w, w_dtype, n, ldw, bias, fmt_mask, map, recorded, rec_dtype, ldr, sums, scratch, scratch_doubles,
                               stream, false, nullptr, 0);
}

extern "C" int mtq_output_error_qx(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                                   const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                                   double *sums, double *scratch, size_t scratch_doubles, void *stream, const void *xq, int64_t ldxq)
{
    return launch_output_error(x, m, k, ldx, w, w_dtype, n, ldw, bias, fmt_mask, map, recorded, rec_dtype, ldr, sums, scratch, scratch_doubles,
                               stream, true, xq, ldxq);
}

extern "C" int mtq_output_error_transposed(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                                           const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype,
                                           int64_t ldr, double *sums, double *scratch, size_t scratch_doubles, void *stream, const void *xq,
                                           int64_t ldxq)
{
    return launch_output_error(x, m, k, ldx, w, w_dtype, n, ldw, bias, fmt_mask, map, recorded, rec_dtype, ldr, sums, scratch, scratch_doubles,
                               stream, xq != nullptr, xq, ldxq, true);
}

extern "C" int mtq_quantize_rows_bf16(const void *x, int64_t rows, int64_t cols, int64_t ld, int fmt, void *y, int64_t ldy, void *stream)
{
    if (!x || !y) return fail(MTQ_ERR_INVALID, "null argument");
    if (fmt < MTQ_FMT_BF16 || fmt > MTQ_FMT_BFP2) return fail(MTQ_ERR_UNSUPPORTED, "activation format code must be 0..3 (bf16,bfp8,bfp4,bfp2)");
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty tensors are handled by the caller)");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (ldy < cols) return fail(MTQ_ERR_INVALID, "ldy < cols");
    if (rows > (int64_t)1 << 40 || cols > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (int rc = require_device()) return rc;
    const int vec_ok = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ld % 8 == 0;
    const int vec_ok_y = reinterpret_cast<uintptr_t>(y) % 16 == 0 && ldy % 8 == 0;
    const int64_t gw = (cols + kGroup - 1) / kGroup;
    const dim3 grid((unsigned)((gw + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535));
    const uint16_t *xp = static_cast<const uint16_t *>(x);
    uint16_t *yp = static_cast<uint16_t *>(y);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (fmt) {
    case MTQ_FMT_BF16: hipLaunchKernelGGL(quantize_rows_bf16<0>, grid, dim3(256), 0, st, xp, rows, cols, ld, yp, ldy, vec_ok, vec_ok_y); break;
    case MTQ_FMT_BFP8: hipLaunchKernelGGL(quantize_rows_bf16<1>, grid, dim3(256), 0, st, xp, rows, cols, ld, yp, ldy, vec_ok, vec_ok_y); break;
    case MTQ_FMT_BFP4: hipLaunchKernelGGL(quantize_rows_bf16<2>, grid, dim3(256), 0, st, xp, rows, cols, ld, yp, ldy, vec_ok, vec_ok_y); break;
    default: hipLaunchKernelGGL(quantize_rows_bf16<3>, grid, dim3(256), 0, st, xp, rows, cols, ld, yp, ldy, vec_ok, vec_ok_y); break;
    }
    return check_launch("mtq_quantize_rows_bf16");
}
