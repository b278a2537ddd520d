// mtq_budget.hip — the two device halves of the activation-aware budget maps (budget_maps.py).
//
// mtq_gram_blocks: the diagonal 32 × 32 blocks of XᵀX, H_c = X[:, 32c : 32c+32]ᵀ · X[:, 32c : 32c+32] in float64, ADDED into h.
//   A workgroup of 4 waves owns 128 columns (one column block per wave) and a span of tokens.  Per step it stages 64 tokens × 128
//   columns of X in LDS (row-major, as read); each wave reads its block back transposed with ds_read_b64_tr_b16, so lane l holds tokens
//   8(l>>5) .. +7 of column l & 31 — for H = X_cᵀX_c that is both the A and the B fragment of mfma_f32_32x32x16_bf16.  bf16 × bf16
//   products are exact in f32; the f32 accumulator is folded into float64 every kFold tokens, which bounds the error of an entry by
//   2⁻¹⁶·(|X|ᵀ|X|)_ab.  Each workgroup writes its blocks to scratch; a second kernel adds the spans in index order (no float atomics:
//   the same inputs give the same bits).
// mtq_tile_error_tables: for every 32 × 32 tile t = (r, c) of W and format f, Δ = K2_f(W) − W in float64 (the literal helpers of
//   mtq_device.hpp, so Δ is the one K2 / K3 build) and e_out[t, f] = Σ_i δ_iᵀ H_c δ_i, e_w[t, f] = Σ δ², both in a fixed order.
//   One wave per workgroup walks a column of tiles with H_c's rows in registers.
// mtq_tile_error_tables_transposed: the same tables in the transposed layout (Δ from column groups, tiles over Wᵀ's grid).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kGCols = 128;            // columns per workgroup: 4 waves × one 32-column block
constexpr int kGStep = 64;             // tokens staged per step
constexpr int kGFold = 256;            // f32 → f64 fold interval in tokens (a multiple of kGStep)
constexpr int kGPitch = 160;           // LDS row pitch in bf16 (320 B: the 4 rows of a transposed read land on distinct banks)
constexpr int64_t kGTargetGroups = 1024;
constexpr int kBlock = kTile * kTile;  // doubles per Gram block

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Tokens per workgroup (a multiple of kGFold) and the number of spans: about kGTargetGroups workgroups, fewer when m is short.
__host__ void gram_split(int64_t m, int64_t k, int64_t *span, int64_t *spans)
{
    const int64_t groups = (k + kGCols - 1) / kGCols;
    const int64_t folds = (m + kGFold - 1) / kGFold;
    const int64_t want = std::min<int64_t>(std::max<int64_t>((kGTargetGroups + groups - 1) / groups, 1), folds);
    *span = ((folds + want - 1) / want) * kGFold;
    *spans = (m + *span - 1) / *span;
}

__device__ __forceinline__ i16x4 read_tr(const uint16_t *p)
{
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4 *)(p));
}

__global__ __launch_bounds__(256) void gram_blocks_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec,
                                                          int64_t span, int64_t nb, double *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) uint16_t xs[kGStep * kGPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kGCols;
    const int64_t t0 = (int64_t)blockIdx.y * span, t1 = std::min<int64_t>(M, t0 + span);

    // global → registers one step ahead: 64 tokens × 128 columns = 1024 pieces of 8 bf16, 4 per thread; zeros past M and K
    uint4 xr[4];
    auto load_step = [&](int64_t tk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * i, row = p >> 4, c8 = (p & 15) * 8;
            const int64_t gm = tk + row, gk = c0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < t1) {
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
    };

    // transposed read (T10): lane 4q + p of 16-lane group g supplies row 8(g>>1) + q, columns 16(g&1) + 4p of the wave's block and
    // receives column 16(g&1) + (lane&15) = lane&31 of those 4 rows; the second read takes rows + 4.  Every lane reads (EXEC full).
    const int g = lane >> 4;
    const int rd = (8 * (g >> 1) + ((lane & 15) >> 2)) * kGPitch + 32 * wave + 16 * (g & 1) + 4 * (lane & 3);

    f32x16 acc;
    double acc64[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; acc64[r] = 0.0; }
    load_step(t0);
    for (int64_t tk = t0; tk < t1; tk += kGStep) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * i;
            *reinterpret_cast<uint4 *>(xs + (p >> 4) * kGPitch + (p & 15) * 8) = xr[i];
        }
        __syncthreads();
        if (tk + kGStep < t1) load_step(tk + kGStep);
#pragma unroll
        for (int kk = 0; kk < kGStep / 16; ++kk) {
            const i16x4 lo = read_tr(xs + rd + 16 * kk * kGPitch);
            const i16x4 hi = read_tr(xs + rd + (16 * kk + 4) * kGPitch);
            const bf16x8 a = __builtin_bit_cast(bf16x8, (i16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, a, acc, 0, 0, 0);
        }
        __syncthreads();
        if ((tk + kGStep - t0) % kGFold == 0 || tk + kGStep >= t1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc64[r] += (double)acc[r]; acc[r] = 0.0f; }
        }
    }
    // lane holds H[(r&3) + 8(r>>2) + 4(lane>>5)][lane&31] of its block in register r
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= nb) return;
    double *dst = partials + ((int64_t)blockIdx.y * nb + b) * kBlock;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * kTile + (lane & 31)] = acc64[r];
}

// h[i] += Σ_s partials[s][i], s in index order.
__global__ __launch_bounds__(256) void gram_blocks_reduce(const double *__restrict__ partials, int64_t spans, int64_t entries, double *__restrict__ h)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= entries) return;
    double v = 0.0;
    for (int64_t s = 0; s < spans; ++s) v += partials[s * entries + i];
    h[i] += v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per workgroup: tile column c = blockIdx.x, tile rows blockIdx.y, + gridDim.y, ...  Lane l loads the group (row l>>1,
// columns 16(l&1) ..) and keeps row a = l&31 of H_c; per format it writes its δ to LDS and forms Σ_{i ≡ l>>5 (mod 2)} δ_i[a]·(H_c δ_i)[a].
template <typename T>
__global__ __launch_bounds__(64) void tile_error_tables_kernel(const T *__restrict__ w, int64_t N, int64_t K, int64_t ldw, int w_vec,
                                                               const double *__restrict__ h, int64_t th, int64_t tw,
                                                               double *__restrict__ e_out, double *__restrict__ e_w)
{
    __shared__ __attribute__((aligned(16))) double dl[kTile][kTile];
    const int lane = threadIdx.x, a = lane & 31, half = lane >> 5;
    const int64_t c = blockIdx.x;
    double hrow[kTile];
#pragma unroll
    for (int b = 0; b < kTile; ++b) hrow[b] = h[c * kBlock + a * kTile + b];
    const int lrow = lane >> 1, lcol = 16 * (lane & 1);
    for (int64_t r = blockIdx.y; r < th; r += gridDim.y) {
        uint32_t u[kGroup];
        Loader<T>::group(w, r * kTile + lrow, c * kTile + lcol, N, K, ldw, w_vec != 0, u);
        const uint32_t E = group_shared_exp(u);
        const int64_t t = r * tw + c;
#pragma unroll 1
        for (int f = 0; f < kNumFmt; ++f) {
            double sq = 0.0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const double d = (double)__uint_as_float(quant_elem_bits(f, u[i], E)) - (double)__uint_as_float(u[i]);
                dl[lrow][lcol + i] = d;
                sq += d * d;
            }
            __syncthreads();
            double part = 0.0;
#pragma unroll 4
            for (int j = 0; j < kTile / 2; ++j) {
                const int i = 2 * j + half;
                double gsum = 0.0;
#pragma unroll
                for (int b = 0; b < kTile; ++b) gsum = fma(hrow[b], dl[i][b], gsum);
                part = fma(dl[i][a], gsum, part);
            }
            __syncthreads();
            part = wave_sum(part);
            if (e_w) sq = wave_sum(sq);
            if (lane == 0) {
                e_out[t * kNumFmt + f] = part;
                if (e_w) e_w[t * kNumFmt + f] = sq;
            }
        }
    }
}

// The transposed layout: Δ = K2_f(Wᵀ)ᵀ − W, groups of 16 consecutive rows of one column, and tiles over Wᵀ's grid (t = kb · tn + nb,
// tn = ceil(N/32)).  Tile (kb, nb) pairs rows nb of W with column block kb, so H_kb is the one it needs.  One wave per workgroup: tile
// row kb = blockIdx.x of Wᵀ (H_kb's rows in registers), tile columns blockIdx.y, + gridDim.y, ...  Lane l loads the column group
// (column 32kb + (l>>1), rows 32nb + 16(l&1) ..) and writes its δ transposed into dl, so that dl[i] is again row i of W over the
// block's 32 columns; the rest is tile_error_tables_kernel's.
template <typename T>
__global__ __launch_bounds__(64) void tile_error_tables_t_kernel(const T *__restrict__ w, int64_t N, int64_t K, int64_t ldw,
                                                                 const double *__restrict__ h, int64_t tk, int64_t tn,
                                                                 double *__restrict__ e_out, double *__restrict__ e_w)
{
    __shared__ __attribute__((aligned(16))) double dl[kTile][kTile];
    const int lane = threadIdx.x, a = lane & 31, half = lane >> 5;
    const int64_t kb = blockIdx.x;
    double hrow[kTile];
#pragma unroll
    for (int b = 0; b < kTile; ++b) hrow[b] = h[kb * kBlock + a * kTile + b];
    const int lcol = lane >> 1, lrow = 16 * (lane & 1);
    const int64_t col = kb * kTile + lcol;
    for (int64_t nb = blockIdx.y; nb < tn; nb += gridDim.y) {
        const int64_t row0 = nb * kTile + lrow;
        uint32_t u[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int64_t row = row0 + i;
            u[i] = (row < N && col < K) ? (sizeof(T) == 4 ? __float_as_uint((float)w[row * ldw + col])
                                                          : (uint32_t)w[row * ldw + col] << 16)
                                        : 0u;
        }
        const uint32_t E = group_shared_exp(u);
        const int64_t t = kb * tn + nb;
#pragma unroll 1
        for (int f = 0; f < kNumFmt; ++f) {
            double sq = 0.0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const double d = (double)__uint_as_float(quant_elem_bits(f, u[i], E)) - (double)__uint_as_float(u[i]);
                dl[lrow + i][lcol] = d;
                sq += d * d;
            }
            __syncthreads();
            double part = 0.0;
#pragma unroll 4
            for (int j = 0; j < kTile / 2; ++j) {
                const int i = 2 * j + half;
                double gsum = 0.0;
#pragma unroll
                for (int b = 0; b < kTile; ++b) gsum = fma(hrow[b], dl[i][b], gsum);
                part = fma(dl[i][a], gsum, part);
            }
            __syncthreads();
            part = wave_sum(part);
            if (e_w) sq = wave_sum(sq);
            if (lane == 0) {
                e_out[t * kNumFmt + f] = part;
                if (e_w) e_w[t * kNumFmt + f] = sq;
            }
        }
    }
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_gram_blocks_scratch_doubles(int64_t m, int64_t k)
{
    if (m <= 0 || k <= 0) return 0;
    int64_t span, spans;
    gram_split(m, k, &span, &spans);
    return (size_t)spans * (size_t)((k + kTile - 1) / kTile) * kBlock;
}

extern "C" int mtq_gram_blocks(const void *x, int64_t m, int64_t k, int64_t ldx, double *h, size_t h_doubles, double *scratch,
                               size_t scratch_doubles, void *stream)
{
    if (!x || !h || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (m <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "m and k must be positive (empty chunks are handled by the caller)");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (m > (int64_t)1 << 40 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t nb = (k + kTile - 1) / kTile;
    if (h_doubles != (size_t)nb * kBlock) return fail(MTQ_ERR_INVALID, "h_doubles != ceil(k / 32) * 1024");
    if (scratch_doubles < mtq_gram_blocks_scratch_doubles(m, k)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_gram_blocks_scratch_doubles(m, k)");
    int64_t span, spans;
    gram_split(m, k, &span, &spans);
    if (spans > 65535) return fail(MTQ_ERR_INVALID, "too many token spans for one launch: pass m in chunks");
    if (int rc = require_device()) return rc;
    const int x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((k + kGCols - 1) / kGCols), (unsigned)spans);
    hipLaunchKernelGGL(gram_blocks_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), m, k, ldx, x_vec, span, nb, scratch);
    if (int rc = check_launch("mtq_gram_blocks")) return rc;
    const int64_t entries = nb * kBlock;
    hipLaunchKernelGGL(gram_blocks_reduce, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, scratch, spans, entries, h);
    return check_launch("mtq_gram_blocks (reduce)");
}

extern "C" int mtq_tile_error_tables(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *h, size_t h_doubles,
                                     double *e_out, double *e_w, size_t table_doubles, void *stream)
{
    if (!w || !h || !e_out) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "n and k must be positive");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (n > (int64_t)1 << 30 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t th = (n + kTile - 1) / kTile, tw = (k + kTile - 1) / kTile;
    if (h_doubles != (size_t)tw * kBlock) return fail(MTQ_ERR_INVALID, "h_doubles != ceil(k / 32) * 1024");
    if (table_doubles != (size_t)(th * tw) * kNumFmt) return fail(MTQ_ERR_INVALID, "table_doubles != tiles * 4");
    if (tw > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many tile columns for one launch");
    if (int rc = require_device()) return rc;
    const int64_t esz = w_dtype == MTQ_DTYPE_F32 ? 4 : 2;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * esz) % 16 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)tw, (unsigned)std::min<int64_t>(th, std::max<int64_t>(1, 16384 / tw)));
    if (w_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(tile_error_tables_kernel<float>, grid, dim3(64), 0, st, static_cast<const float *>(w), n, k, ldw, w_vec, h, th, tw, e_out, e_w);
    else
        hipLaunchKernelGGL(tile_error_tables_kernel<uint16_t>, grid, dim3(64), 0, st, static_cast<const uint16_t *>(w), n, k, ldw, w_vec, h, th, tw,
                           e_out, e_w);
    return check_launch("mtq_tile_error_tables");
}

extern "C" int mtq_tile_error_tables_transposed(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *h,
                                                size_t h_doubles, double *e_out, double *e_w, size_t table_doubles, void *stream)
{
    if (!w || !h || !e_out) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "n and k must be positive");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (n > (int64_t)1 << 30 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t tk = (k + kTile - 1) / kTile, tn = (n + kTile - 1) / kTile;   // Wᵀ's grid: tk × tn
    if (h_doubles != (size_t)tk * kBlock) return fail(MTQ_ERR_INVALID, "h_doubles != ceil(k / 32) * 1024");
    if (table_doubles != (size_t)(tk * tn) * kNumFmt) return fail(MTQ_ERR_INVALID, "table_doubles != tiles * 4");
    if (tk > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many tile rows for one launch");
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)tk, (unsigned)std::min<int64_t>(tn, std::max<int64_t>(1, 16384 / tk)));
    if (w_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(tile_error_tables_t_kernel<float>, grid, dim3(64), 0, st, static_cast<const float *>(w), n, k, ldw, h, tk, tn, e_out, e_w);
    else
        hipLaunchKernelGGL(tile_error_tables_t_kernel<uint16_t>, grid, dim3(64), 0, st, static_cast<const uint16_t *>(w), n, k, ldw, h, tk, tn,
                           e_out, e_w);
    return check_launch("mtq_tile_error_tables_transposed");
}
