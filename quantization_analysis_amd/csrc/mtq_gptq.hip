// mtq_gptq.hip — the two device halves of GPTQ's error-compensated BFP weights (quantization_analysis_amd/gptq.py holds the contract).
//
// mtq_gram_full: all of H = XᵀX as k × k float64, ADDED into h.  A workgroup of 4 waves owns a pair (I, J), I ≤ J, of 128-column super
//   blocks and a span of tokens.  Per step it stages 64 tokens × 128 columns of X for I and for J in LDS (row-major, as read); wave w reads
//   32-column block 4I + w of the I image transposed (ds_read_b64_tr_b16) as the A fragment and blocks 4J + c of the J image as the B
//   fragments of mfma_f32_32x32x16_bf16, skipping the blocks below the diagonal.  The numerics are those of mtq_gram_blocks: bf16
//   products exact in f32, f32 folded into float64 every kFold tokens (an entry within 2⁻¹⁶·(|X|ᵀ|X|)_ab).  Each entry of a block pair is
//   formed once and written to (a, b) and (b, a), so h stays bitwise symmetric.  With one span per pair the kernel adds into h directly;
//   with several, spans go to scratch and a second kernel adds them in index order (no float atomics).
// mtq_gptq_sweep: the column sweep, rows independent.  A workgroup of 4 waves owns a strip of 32 rows (one tile row) and walks its
//   32-column blocks left to right.  Per block, the waves first form Σ_{i < b0} e_i · U[i, block] for the strip (the GEMM-shaped part,
//   float64 VALU fma from LDS-staged 16-column chunks of Eᵀ and U, the chunks dealt round-robin over the 4 waves and the 4 partials added
//   in wave order); then wave 0 holds the block in registers, lane = (row, 16-column half), so a BFP group and the tile's code are
//   lane-local, and runs the 32 sequential steps with U's diagonal block in LDS.  e goes to scratch (Eᵀ, k_pad × n_pad doubles).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kFCols = 128;            // columns per super block: 4 waves × one 32-column block
constexpr int kFStep = 64;             // tokens staged per step
constexpr int kFFold = 256;            // f32 → f64 fold interval in tokens (a multiple of kFStep)
constexpr int kFPitch = 160;           // LDS row pitch in bf16 (as mtq_gram_blocks)
constexpr int64_t kFTargetGroups = 1024;
constexpr int kBlock = kTile * kTile;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int64_t super_pairs(int64_t k)
{
    const int64_t sb = (k + kFCols - 1) / kFCols;
    return sb * (sb + 1) / 2;
}

// Tokens per workgroup (a multiple of kFFold) and the number of spans: about kFTargetGroups workgroups, one span once the pairs alone
// reach that (no scratch then).
__host__ void gram_full_split(int64_t m, int64_t k, int64_t *span, int64_t *spans)
{
    const int64_t pairs = super_pairs(k);
    const int64_t folds = (m + kFFold - 1) / kFFold;
    const int64_t want = std::min<int64_t>(std::max<int64_t>((kFTargetGroups + pairs - 1) / pairs, 1), folds);
    *span = ((folds + want - 1) / want) * kFFold;
    *spans = (m + *span - 1) / *span;
}

// super pair index p = J(J+1)/2 + I, I ≤ J
__device__ __forceinline__ void pair_of(int64_t p, int64_t *si, int64_t *sj)
{
    int64_t j = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > p) --j;
    while ((j + 1) * (j + 2) / 2 <= p) ++j;
    *sj = j;
    *si = p - j * (j + 1) / 2;
}

__device__ __forceinline__ i16x4 read_tr(const uint16_t *p)
{
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4 *)(p));
}

// Entry (a, b) of block pair (bi, bj), bi ≤ bj: added at (a, b) and, off the diagonal, at (b, a); on a diagonal block only a ≤ b is
// used (the MFMA forms both triangles, not necessarily equal bit for bit).
__device__ __forceinline__ void add_entry(double *__restrict__ h, int64_t K, int64_t bi, int64_t bj, int a, int b, double v)
{
    const int64_t ga = bi * kTile + a, gb = bj * kTile + b;
    if (ga >= K || gb >= K) return;
    if (bi == bj && a > b) return;
    h[ga * K + gb] += v;
    if (ga != gb) h[gb * K + ga] += v;
}

__global__ __launch_bounds__(256) void gram_full_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec, int64_t span,
                                                        int64_t pairs, double *__restrict__ h, double *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) uint16_t xs[2][kFStep * kFPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    int64_t si, sj;
    pair_of(p, &si, &sj);
    const int64_t c0[2] = {si * kFCols, sj * kFCols};
    const int64_t t0 = (int64_t)blockIdx.y * span, t1 = std::min<int64_t>(M, t0 + span);
    const int64_t bi = si * 4 + wave;
    const bool diag = si == sj;

    // global → registers one step ahead: 2 × 64 tokens × 128 columns = 2048 pieces of 8 bf16, 8 per thread; zeros past M and K
    uint4 xr[8];
    auto load_step = [&](int64_t tk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pc = tid + 256 * i, s = pc >> 10, q = pc & 1023, row = q >> 4, c8 = (q & 15) * 8;
            const int64_t gm = tk + row, gk = c0[s] + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < t1) {
                const uint16_t *src = x + gm * ldx + gk;
                if (x_vec && gk + 8 <= K) {
                    v = *reinterpret_cast<const uint4 *>(src);
                } else {
                    uint32_t hh[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) hh[j] = gk + j < K ? (uint32_t)src[j] : 0u;
                    v = make_uint4(hh[0] | (hh[1] << 16), hh[2] | (hh[3] << 16), hh[4] | (hh[5] << 16), hh[6] | (hh[7] << 16));
                }
            }
            xr[i] = v;
        }
    };

    // the transposed read of mtq_gram_blocks: lane l receives column l & 31 of the block, tokens 8(l>>5) .. +7 of the 16 (two reads)
    const int g = lane >> 4;
    const int rd = (8 * (g >> 1) + ((lane & 15) >> 2)) * kFPitch + 16 * (g & 1) + 4 * (lane & 3);
    bool live[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) live[c] = !(diag && c < wave) && bi * kTile < K && (sj * 4 + c) * kTile < K;   // wave-uniform

    f32x16 acc[4];
    double acc64[4][16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[c][r] = 0.0f; acc64[c][r] = 0.0; }
    load_step(t0);
    for (int64_t tk = t0; tk < t1; tk += kFStep) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pc = tid + 256 * i, s = pc >> 10, q = pc & 1023;
            *reinterpret_cast<uint4 *>(&xs[s][(q >> 4) * kFPitch + (q & 15) * 8]) = xr[i];
        }
        __syncthreads();
        if (tk + kFStep < t1) load_step(tk + kFStep);
#pragma unroll
        for (int kk = 0; kk < kFStep / 16; ++kk) {
            const i16x4 alo = read_tr(&xs[0][rd + 32 * wave + 16 * kk * kFPitch]);
            const i16x4 ahi = read_tr(&xs[0][rd + 32 * wave + (16 * kk + 4) * kFPitch]);
            const bf16x8 a = __builtin_bit_cast(bf16x8, (i16x8)__builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!live[c]) continue;
                const i16x4 blo = read_tr(&xs[1][rd + 32 * c + 16 * kk * kFPitch]);
                const i16x4 bhi = read_tr(&xs[1][rd + 32 * c + (16 * kk + 4) * kFPitch]);
                const bf16x8 b = __builtin_bit_cast(bf16x8, (i16x8)__builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[c], 0, 0, 0);
            }
        }
        __syncthreads();
        if ((tk + kFStep - t0) % kFFold == 0 || tk + kFStep >= t1) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc64[c][r] += (double)acc[c][r]; acc[c][r] = 0.0f; }
        }
    }
    // lane holds entry (a, b) = ((r&3) + 8(r>>2) + 4(lane>>5), lane&31) of block pair (bi, 4J + c) in register r
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!live[c]) continue;
        const int64_t bj = sj * 4 + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), b = lane & 31;
            if (partials)
                partials[(((int64_t)blockIdx.y * pairs + p) * 16 + wave * 4 + c) * kBlock + a * kTile + b] = acc64[c][r];
            else
                add_entry(h, K, bi, bj, a, b, acc64[c][r]);
        }
    }
}

// h += Σ_s partials[s], s in index order, each entry once and mirrored.
__global__ __launch_bounds__(256) void gram_full_reduce(const double *__restrict__ partials, int64_t spans, int64_t pairs, int64_t K,
                                                        double *__restrict__ h)
{
    const int64_t entries = pairs * 16 * kBlock;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= entries) return;
    const int64_t slot = i / kBlock, p = slot / 16;
    const int wave = (int)((slot / 4) % 4), c = (int)(slot % 4), a = (int)((i % kBlock) / kTile), b = (int)(i % kTile);
    int64_t si, sj;
    pair_of(p, &si, &sj);
    if (si == sj && c < wave) return;
    double v = 0.0;
    for (int64_t s = 0; s < spans; ++s) v += partials[s * entries + i];
    add_entry(h, K, si * 4 + wave, sj * 4 + c, a, b, v);
}

// ----------------------------------------------------------------------------- the sweep

constexpr int kSChunk = 16;            // earlier columns per LDS-staged chunk of the GEMM-shaped part

__device__ __forceinline__ double2 ld2(const double *p) { return *reinterpret_cast<const double2 *>(p); }

template <typename T>
__global__ __launch_bounds__(256) void gptq_sweep_kernel(const T *__restrict__ w, int64_t N, int64_t K, int64_t ldw, int w_vec,
                                                         const double *__restrict__ u, int u_vec, const int8_t *__restrict__ codes, int64_t tw,
                                                         float *__restrict__ out, int64_t ldo, double *__restrict__ loss,
                                                         double *__restrict__ et, int64_t lde)
{
    // per wave: Eᵀ chunk [16][32] then U chunk [16][32] (8 KB); after the GEMM part the same 8 KB hold the wave's 32 × 32 partial
    __shared__ __attribute__((aligned(16))) double stage[4][2 * kSChunk * kTile];
    __shared__ __attribute__((aligned(16))) double ud[kTile][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int64_t tr = blockIdx.x;
    double *es = stage[wave], *us = stage[wave] + kSChunk * kTile;
    const int rg = lane >> 3, cg = lane & 7;                   // GEMM part: rows 4rg .. +3, columns 4cg .. +3 of the block
    const int row = lane >> 1, half = lane & 1;                // sweep (wave 0): row, 16-column half
    const int64_t grow = r0 + row;
    double lsum = 0.0;

    for (int64_t b0 = 0; b0 < K; b0 += kTile) {
        // ---- Σ_{i < b0} e_i · U[i, b0 + col] for the strip: chunk ch = 4t + wave of the b0 / 16 earlier chunks
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        const int64_t nch = b0 / kSChunk, trips = (nch + 3) / 4;
        double2 er[4], ur[4];
        auto load_chunk = [&](int64_t ch) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int pc = lane + 64 * s, ii = pc >> 4, c2 = (pc & 15) * 2;
                const int64_t gi = ch * kSChunk + ii;
                er[s] = ld2(et + gi * lde + r0 + c2);
                const int64_t gc = b0 + c2;
                if (u_vec && gc + 1 < K) {
                    ur[s] = ld2(u + gi * K + gc);
                } else {
                    ur[s].x = gc < K ? u[gi * K + gc] : 0.0;
                    ur[s].y = gc + 1 < K ? u[gi * K + gc + 1] : 0.0;
                }
            }
        };
        if (wave < nch) load_chunk(wave);
        for (int64_t t = 0; t < trips; ++t) {
            const int64_t ch = 4 * t + wave;
            __syncthreads();
            if (ch < nch) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int pc = lane + 64 * s, ii = pc >> 4, c2 = (pc & 15) * 2;
                    *reinterpret_cast<double2 *>(es + ii * kTile + c2) = er[s];
                    *reinterpret_cast<double2 *>(us + ii * kTile + c2) = ur[s];
                }
            }
            __syncthreads();
            if (ch + 4 < nch) load_chunk(ch + 4);
            if (ch < nch) {
#pragma unroll 4
                for (int ii = 0; ii < kSChunk; ++ii) {
                    const double2 e01 = ld2(es + ii * kTile + 4 * rg), e23 = ld2(es + ii * kTile + 4 * rg + 2);
                    const double2 u01 = ld2(us + ii * kTile + 4 * cg), u23 = ld2(us + ii * kTile + 4 * cg + 2);
                    const double ev[4] = {e01.x, e01.y, e23.x, e23.y}, uv[4] = {u01.x, u01.y, u23.x, u23.y};
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[r][c] = fma(ev[r], uv[c], acc[r][c]);
                }
            }
        }
        __syncthreads();
        {   // the wave's partial into its own stage region; U's diagonal block (upper triangle only) into ud
            double *red = stage[wave];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) red[(4 * rg + r) * kTile + 4 * cg + c] = acc[r][c];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int idx = tid + 256 * s, i = idx >> 5, c = idx & 31;
                const int64_t gi = b0 + i, gc = b0 + c;
                ud[i][c] = (gi < K && gc < K && c >= i) ? u[gi * K + gc] : 0.0;
            }
        }
        __syncthreads();
        if (wave == 0) {
            // ---- the 32 sequential steps of the block: lane (row, half) holds columns b0 + 16·half .. + 15 of its row
            const int code = (int)codes[tr * tw + b0 / kTile];
            const bool is_bf16 = code == 0;
            const uint32_t M = code == 1 ? 7u : (code == 2 ? 3u : 1u);
            uint32_t wu[kGroup];
            Loader<T>::group(w, grow, b0 + 16 * half, N, K, ldw, w_vec != 0, wu);
            double cur[kGroup], eo[kGroup];
            uint32_t qo[kGroup];
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                const int a = row * kTile + 16 * half + c;
                const double v = ((stage[0][a] + stage[1][a]) + stage[2][a]) + stage[3][a];
                cur[c] = (double)__uint_as_float(wu[c]) - v;
                eo[c] = 0.0;
                qo[c] = 0u;
            }
            uint32_t E = 0u;
#pragma unroll
            for (int j = 0; j < kTile; ++j) {
                const int gsel = j >> 4, c = j & 15;
                const bool col_ok = b0 + j < K;
                double e = 0.0;
                if (half == gsel) {
                    if (c == 0) {
                        uint32_t mx = 0u;
#pragma unroll
                        for (int i = 0; i < kGroup; ++i) mx = max(mx, __float_as_uint((float)cur[i]) & 0x7F800000u);
                        E = mx >> 23;
                    }
                    if (col_ok) {
                        const uint32_t xu = __float_as_uint((float)cur[c]);
                        const uint32_t qb = is_bf16 ? bf16_round_bits(xu) : bfp_elem_bits_sat(xu, E, M);
                        e = (cur[c] - (double)__uint_as_float(qb)) / ud[j][j];
                        qo[c] = qb;
                        eo[c] = e;
                    }
                }
                e = __shfl(e, (lane & ~1) | gsel, 64);
                lsum = lsum + e * e;
#pragma unroll
                for (int cc = 0; cc < kGroup; ++cc) {
                    const int col = 16 * half + cc;
                    if (col > j) cur[cc] = cur[cc] - e * ud[j][col];
                }
            }
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                const int64_t col = b0 + 16 * half + c;
                et[col * lde + grow] = eo[c];
                if (grow < N && col < K) out[grow * ldo + col] = __uint_as_float(qo[c]);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && half == 0 && grow < N) loss[grow] = lsum;
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_gram_full_scratch_doubles(int64_t m, int64_t k)
{
    if (m <= 0 || k <= 0 || k > (int64_t)1 << 30) return 0;
    int64_t span, spans;
    gram_full_split(m, k, &span, &spans);
    return spans > 1 ? (size_t)spans * (size_t)super_pairs(k) * 16 * kBlock : 0;
}

extern "C" int mtq_gram_full(const void *x, int64_t m, int64_t k, int64_t ldx, double *h, size_t h_doubles, double *scratch, size_t scratch_doubles,
                             void *stream)
{
    if (!x || !h || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (m <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "m and k must be positive (empty chunks are handled by the caller)");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (m > (int64_t)1 << 40 || k > (int64_t)1 << 20) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (h_doubles != (size_t)k * (size_t)k) return fail(MTQ_ERR_INVALID, "h_doubles != k * k");
    if (scratch_doubles < mtq_gram_full_scratch_doubles(m, k)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_gram_full_scratch_doubles(m, k)");
    int64_t span, spans;
    gram_full_split(m, k, &span, &spans);
    if (spans > 65535) return fail(MTQ_ERR_INVALID, "too many token spans for one launch: pass m in chunks");
    const int64_t pairs = super_pairs(k);
    if (pairs > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many column blocks for one launch");
    if (int rc = require_device()) return rc;
    const int x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)pairs, (unsigned)spans);
    hipLaunchKernelGGL(gram_full_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), m, k, ldx, x_vec, span, pairs, h,
                       spans > 1 ? scratch : nullptr);
    if (int rc = check_launch("mtq_gram_full")) return rc;
    if (spans == 1) return MTQ_OK;
    const int64_t entries = pairs * 16 * kBlock;
    hipLaunchKernelGGL(gram_full_reduce, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, scratch, spans, pairs, k, h);
    return check_launch("mtq_gram_full (reduce)");
}

extern "C" size_t mtq_gptq_sweep_scratch_doubles(int64_t n, int64_t k)
{
    if (n <= 0 || k <= 0 || n > (int64_t)1 << 30 || k > (int64_t)1 << 20) return 0;
    return (size_t)((n + kTile - 1) / kTile * kTile) * (size_t)((k + kTile - 1) / kTile * kTile);
}

extern "C" int mtq_gptq_sweep(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *u, size_t u_doubles, const int8_t *codes,
                              size_t code_count, float *out, int64_t ldo, double *loss, double *scratch, size_t scratch_doubles, void *stream)
{
    if (!w || !u || !codes || !out || !loss || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "n and k must be positive");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (ldo < k) return fail(MTQ_ERR_INVALID, "ldo < k");
    if (n > (int64_t)1 << 30 || k > (int64_t)1 << 20) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (u_doubles != (size_t)k * (size_t)k) return fail(MTQ_ERR_INVALID, "u_doubles != k * k");
    const int64_t th = (n + kTile - 1) / kTile, tw = (k + kTile - 1) / kTile;
    if (code_count != (size_t)(th * tw)) return fail(MTQ_ERR_INVALID, "code_count != ceil(n / 32) * ceil(k / 32)");
    if (scratch_doubles < mtq_gptq_sweep_scratch_doubles(n, k)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_gptq_sweep_scratch_doubles(n, k)");
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(MTQ_ERR_INVALID, "scratch must be 16-byte aligned");
    if (th > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many row strips for one launch");
    if (int rc = require_device()) return rc;
    const int64_t esz = w_dtype == MTQ_DTYPE_F32 ? 4 : 2;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * esz) % 16 == 0;
    const int u_vec = reinterpret_cast<uintptr_t>(u) % 16 == 0 && k % 2 == 0;
    const int64_t lde = th * kTile;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (w_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(gptq_sweep_kernel<float>, dim3((unsigned)th), dim3(256), 0, st, static_cast<const float *>(w), n, k, ldw, w_vec, u, u_vec,
                           codes, tw, out, ldo, loss, scratch, lde);
    else
        hipLaunchKernelGGL(gptq_sweep_kernel<uint16_t>, dim3((unsigned)th), dim3(256), 0, st, static_cast<const uint16_t *>(w), n, k, ldw, w_vec, u,
                           u_vec, codes, tw, out, ldo, loss, scratch, lde);
    return check_launch("mtq_gptq_sweep");
}
