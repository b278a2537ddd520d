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
// mtq_tile_sq_error_batched: e_w alone for every tile of `count` equally shaped matrices in one launch, a wave per tile: the group
//   load, the shared exponent, the 16 squared differences of a lane in index order and wave_sum are mtq_tile_error_tables', so the
//   bits are its e_w; no Gram block is read.
// mtq_budget_allocate_device: budget_maps.allocate on the device, for n_seg segments of one table at once.
//   hull     a thread per tile walks the tile's lower convex hull with hull_segments' float64 operations (no contraction in this
//            library, IEEE divide) and keeps up to three steps: the clamped key's bit pattern and the point each step reaches;
//   select   the scan's cut is the first position in (key descending, tile ascending, step ascending) order whose running size
//            exceeds the budget.  The size is allocate's expression over integer counts per format, and "size > budget" is monotone
//            along the order, so the cut is found by bisection: 63 passes on the key's bit pattern (keys are >= +0: their patterns
//            order as integers), then bit_length(4 T + 1) passes on 4 · tile + step inside the group of equal keys at the cut.  A pass
//            is one count kernel (every tile's format under the tried threshold, counted per segment with integer atomics) and one
//            decide kernel of a thread per segment; nothing is read back between passes;
//   final    the map and the counts under the found threshold, and the status.
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


// ----------------------------------------------------------------------------- e_w alone, batched

// One wave per tile, four tiles per workgroup, tiles g = b · tiles + t taken grid-stride.  Lane l loads the group (row l>>1, columns
// 16(l&1) ..) as tile_error_tables_kernel does, and sums its 16 squared differences in the same order.
template <typename T>
__global__ __launch_bounds__(256) void tile_sq_error_kernel(const T *__restrict__ x, int64_t count, int64_t stride, int64_t N, int64_t K,
                                                            int64_t ld, int x_vec, int64_t tw, int64_t tiles, double *__restrict__ e_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lrow = lane >> 1, lcol = 16 * (lane & 1);
    const int64_t total = count * tiles;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < total; g += (int64_t)gridDim.x * 4) {
        const int64_t b = g / tiles, t = g - b * tiles, r = t / tw, c = t - r * tw;
        uint32_t u[kGroup];
        Loader<T>::group(x + b * stride, r * kTile + lrow, c * kTile + lcol, N, K, ld, x_vec != 0, u);
        const uint32_t E = group_shared_exp(u);
        double mine = 0.0;
#pragma unroll
        for (int f = 0; f < kNumFmt; ++f) {                // unrolled: f is a constant in quant_elem_bits; the sums are the rolled loop's
            double sq = 0.0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const double d = (double)__uint_as_float(quant_elem_bits(f, u[i], E)) - (double)__uint_as_float(u[i]);
                sq += d * d;
            }
            sq = wave_sum(sq);
            if (lane == f) mine = sq;
        }
        if (lane < kNumFmt) e_w[g * kNumFmt + lane] = mine;
    }
}

// ----------------------------------------------------------------------------- budget allocation

// The candidates in allocate's order (ascending bytes, then code), P of them: order index p ↔ format code[p], bytes[p] = 1024 ·
// bytes per element as the host forms it; bpe by format code for the size expression.
struct BudgetFormats {
    int P;
    int code[kNumFmt];
    double bytes[kNumFmt];
    double bpe[kNumFmt];
};

constexpr int kBThreads = 256;
constexpr int kBPer = 8;                                   // tiles per thread of a count pass
constexpr int64_t kBKeyTop = 0x7FF0000000000001ll;         // above every key's pattern (+inf included)
constexpr int64_t kBAll = INT64_MAX;

// Per-segment selection state in scratch.
struct BudgetSeg {
    unsigned long long cnt[kNumFmt];   // tiles per order index under the tried threshold
    int64_t lo, hi;                    // key bisection: taking every key >= hi fits, every key >= lo does not (lo = -1: untested)
    int64_t clo, chi;                  // (tile, step) bisection inside the group key == g: through clo fits, through chi does not
    uint64_t g;                        // a step is taken when key > g, or key == g and 4 · tile + step <= c
    int64_t c;
    int32_t bad;                       // a non-finite table entry in the segment
    int32_t pad;
};

// The segment of tile t: the j with first[j] <= t < first[j + 1], or -1.  first is non-decreasing.
__device__ __forceinline__ int budget_segment(const int64_t *__restrict__ first, int n_seg, int64_t t)
{
    int lo = 0, hi = n_seg + 1;                            // entries of first[0 .. n_seg] that are <= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const int j = lo - 1;
    return j >= 0 && j < n_seg ? j : -1;
}

// allocate's size of a segment from its counts per order index: ((cnt · 1024) · bytes per element), summed in format-code order.
__device__ __forceinline__ double budget_size(const unsigned long long cnt[kNumFmt], const BudgetFormats &F)
{
    double by_code[kNumFmt] = {0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < F.P; ++p) by_code[F.code[p]] = ((double)(int64_t)cnt[p] * 1024.0) * F.bpe[F.code[p]];
    double total = 0.0;
#pragma unroll
    for (int f = 0; f < kNumFmt; ++f) total = total + by_code[f];
    return total;
}

// hull_segments for one tile per thread.  keys[t][s]: the clamped slope of step s; steps[t]: the step count in bits 0-1 and the order
// index step s reaches in bits 2(s+1) ..
__global__ __launch_bounds__(kBThreads) void budget_hull_kernel(const double *__restrict__ table, int64_t T, const int64_t *__restrict__ first,
                                                                int n_seg, BudgetFormats F, uint64_t *__restrict__ keys,
                                                                uint8_t *__restrict__ steps, BudgetSeg *__restrict__ seg)
{
    const int64_t t = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (t >= T) return;
    double e[kNumFmt];
    bool finite = true;
#pragma unroll
    for (int f = 0; f < kNumFmt; ++f) {
        e[f] = table[t * kNumFmt + f];
        finite = finite && (__double_as_longlong(e[f]) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll;
    }
    if (!finite) {
        const int j = budget_segment(first, n_seg, t);
        if (j >= 0) atomicOr(&seg[j].bad, 1);
    }
    double pe[kNumFmt];
    for (int p = 0; p < kNumFmt; ++p) pe[p] = p < F.P ? e[F.code[p]] : 0.0;
    int cur = 0, n = 0;
    unsigned packed = 0u;
    double key_prev = __longlong_as_double(0x7FF0000000000000ll);
    uint64_t k[3] = {0ull, 0ull, 0ull};
    for (int step = 0; step < F.P - 1; ++step) {
        const double e_cur = pe[cur], b_cur = F.bytes[cur];
        double best = 0.0;
        int nxt = -1;
        for (int q = 0; q < F.P; ++q) {                    // ascending bytes: a strict > keeps the cheaper point on a tie
            const double gain = e_cur - pe[q], db = F.bytes[q] - b_cur;
            if (db > 0.0 && gain > 0.0) {
                const double slope = __ddiv_rn(gain, db);
                if (nxt < 0 || slope > best) { best = slope; nxt = q; }
            }
        }
        if (nxt < 0) break;
        const double key = best < key_prev ? best : key_prev;
        k[step] = (uint64_t)__double_as_longlong(key);
        packed |= (unsigned)nxt << (2 * (step + 1));
        key_prev = key;
        cur = nxt;
        n = step + 1;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) keys[t * 3 + s] = k[s];
    steps[t] = (uint8_t)(packed | (unsigned)n);
}

// The order index tile t ends at under the threshold (g, c): its taken steps are a prefix (keys do not rise along a tile's steps, and on
// equal keys 4t + s does).
__device__ __forceinline__ int budget_tile_point(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ steps, int64_t t, uint64_t g,
                                                 int64_t c)
{
    const unsigned st = steps[t];
    const int n = (int)(st & 3u);
    int taken = 0;
    for (int s = 0; s < n; ++s) {
        const uint64_t key = keys[t * 3 + s];
        taken += (key > g || (key == g && t * 4 + s <= c)) ? 1 : 0;
    }
    return taken ? (int)((st >> (2 * taken)) & 3u) : 0;
}

// One pass: counts per (segment, order index) under every segment's tried threshold.  A workgroup owns kBThreads · kBPer consecutive
// tiles; when they lie in one segment it adds its four counts once, otherwise every tile adds its own.  With map != null it is the final
// pass: the map's codes and counts by format code.
__global__ __launch_bounds__(kBThreads) void budget_count_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ steps, int64_t T,
                                                                 const int64_t *__restrict__ first, int n_seg, BudgetFormats F,
                                                                 BudgetSeg *__restrict__ seg, int8_t *__restrict__ map,
                                                                 unsigned long long *__restrict__ counts)
{
    __shared__ unsigned block_cnt[kNumFmt];
    const int64_t t0 = (int64_t)blockIdx.x * (kBThreads * kBPer);
    const int64_t t1 = t0 + kBThreads * kBPer < T ? t0 + kBThreads * kBPer : T;
    const int j0 = budget_segment(first, n_seg, t0), j1 = budget_segment(first, n_seg, t1 - 1);
    if (j0 >= 0 && j0 == j1) {
        if (threadIdx.x < kNumFmt) block_cnt[threadIdx.x] = 0u;
        __syncthreads();
        const uint64_t g = seg[j0].g;
        const int64_t c = seg[j0].c;
        unsigned mine[kNumFmt] = {0u, 0u, 0u, 0u};
        for (int64_t t = t0 + threadIdx.x; t < t1; t += kBThreads) {
            const int p = budget_tile_point(keys, steps, t, g, c);
#pragma unroll
            for (int q = 0; q < kNumFmt; ++q) mine[q] += p == q ? 1u : 0u;
            if (map) map[t] = (int8_t)F.code[p];
        }
#pragma unroll
        for (int q = 0; q < kNumFmt; ++q) {
            unsigned v = mine[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&block_cnt[q], v);
        }
        __syncthreads();
        if ((int)threadIdx.x < F.P && block_cnt[threadIdx.x]) {
            unsigned long long *dst = map ? counts + (int64_t)j0 * kNumFmt + F.code[threadIdx.x] : &seg[j0].cnt[threadIdx.x];
            atomicAdd(dst, (unsigned long long)block_cnt[threadIdx.x]);
        }
        return;
    }
    // several segments in the chunk: a wave's 64 consecutive tiles usually still share one, and then add their counts once
    const int lane = threadIdx.x & 63;
    for (int64_t base = t0; base < t1; base += kBThreads) {
        const int64_t t = base + threadIdx.x;
        const int j = t < t1 ? budget_segment(first, n_seg, t) : -1;
        const int p = j >= 0 ? budget_tile_point(keys, steps, t, seg[j].g, seg[j].c) : -1;
        if (map && j >= 0) map[t] = (int8_t)F.code[p];
        const int jw = __shfl(j, 0, 64);
        if (__ballot(j != jw) == 0ull) {
            if (jw < 0) continue;
            for (int q = 0; q < F.P; ++q) {
                const unsigned long long n = (unsigned long long)__popcll(__ballot(p == q));
                if (lane == q && n) atomicAdd(map ? counts + (int64_t)jw * kNumFmt + F.code[q] : &seg[jw].cnt[q], n);
            }
        } else if (j >= 0) {
            atomicAdd(map ? counts + (int64_t)j * kNumFmt + F.code[p] : &seg[j].cnt[p], 1ull);
        }
    }
}

enum { kBInit = 0, kBKey = 1, kBKeyLast = 2, kBTile = 3 };

// A thread per segment: what the pass just counted moves one end of the bisection, and the next threshold to try is set.
__global__ __launch_bounds__(kBThreads) void budget_decide_kernel(BudgetSeg *__restrict__ seg, const int64_t *__restrict__ first, int n_seg,
                                                                  const double *__restrict__ budget, BudgetFormats F, int mode)
{
    const int j = blockIdx.x * kBThreads + threadIdx.x;
    if (j >= n_seg) return;
    BudgetSeg s = seg[j];
    const bool fits = !(budget_size(s.cnt, F) > budget[j]);
    if (mode == kBInit) {
        s.lo = -1;
        s.hi = kBKeyTop;
    } else if (mode == kBTile) {
        if (s.chi - s.clo > 1) { if (fits) s.clo = s.c; else s.chi = s.c; }
    } else if (s.hi - s.lo > 1) {
        if (fits) s.hi = (int64_t)s.g; else s.lo = (int64_t)s.g;
    }
    if (mode == kBInit || mode == kBKey) {
        s.g = (uint64_t)(s.hi - s.lo > 1 ? s.lo + (s.hi - s.lo) / 2 : s.hi);
        s.c = kBAll;
    } else {
        if (mode == kBKeyLast) {
            if (s.lo < 0) {                                // every step fits
                s.g = 0ull;
                s.clo = s.chi = kBAll;
            } else {                                       // the group key == lo holds the cut
                s.g = (uint64_t)s.lo;
                s.clo = first[j] * 4 - 1;
                s.chi = first[j + 1] * 4;
            }
        }
        s.c = s.chi - s.clo > 1 ? s.clo + (s.chi - s.clo) / 2 : s.clo;
    }
#pragma unroll
    for (int p = 0; p < kNumFmt; ++p) s.cnt[p] = 0ull;
    seg[j] = s;
}

// status: 2 a non-finite entry, else 1 the budget below the all-cheapest size, else 0.
__global__ __launch_bounds__(kBThreads) void budget_status_kernel(const BudgetSeg *__restrict__ seg, const int64_t *__restrict__ first, int n_seg,
                                                                  const double *__restrict__ budget, BudgetFormats F, int32_t *__restrict__ status)
{
    const int j = blockIdx.x * kBThreads + threadIdx.x;
    if (j >= n_seg) return;
    unsigned long long cnt[kNumFmt] = {(unsigned long long)(first[j + 1] - first[j]), 0ull, 0ull, 0ull};
    status[j] = seg[j].bad ? 2 : (budget_size(cnt, F) > budget[j] ? 1 : 0);
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

extern "C" int mtq_tile_sq_error_batched(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols,
                                         int64_t ld, double *e_w, void *stream)
{
    if (!x || !e_w) return fail(MTQ_ERR_INVALID, "null argument");
    if (in_dtype != MTQ_DTYPE_BF16 && in_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "in_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (count <= 0 || rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "count, rows and cols must be positive");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (stride_elems < 0 || (count > 1 && stride_elems < (rows - 1) * ld + cols)) return fail(MTQ_ERR_INVALID, "stride_elems shorter than a matrix");
    if (rows > (int64_t)1 << 30 || cols > (int64_t)1 << 30 || count > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "batch too large");
    const int64_t th = (rows + kTile - 1) / kTile, tw = (cols + kTile - 1) / kTile, tiles = th * tw;
    if (tiles > ((int64_t)1 << 40) / count) return fail(MTQ_ERR_INVALID, "batch too large");
    if (int rc = require_device()) return rc;
    const int64_t esz = in_dtype == MTQ_DTYPE_F32 ? 4 : 2;
    const int x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && (ld * esz) % 16 == 0 && (stride_elems * esz) % 16 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)std::min<int64_t>((count * tiles + 3) / 4, 16384));
    if (in_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(tile_sq_error_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(x), count, stride_elems, rows, cols, ld,
                           x_vec, tw, tiles, e_w);
    else
        hipLaunchKernelGGL(tile_sq_error_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), count, stride_elems, rows,
                           cols, ld, x_vec, tw, tiles, e_w);
    return check_launch("mtq_tile_sq_error_batched");
}

// scratch: BudgetSeg [n_seg] | keys uint64 [T][3] | steps uint8 [T]
extern "C" size_t mtq_budget_allocate_scratch_bytes(int64_t tiles, int64_t n_seg)
{
    if (tiles <= 0 || n_seg <= 0 || tiles > (int64_t)1 << 31 || n_seg > INT32_MAX) return 0;
    return (size_t)n_seg * sizeof(BudgetSeg) + (size_t)tiles * 25;
}

extern "C" int mtq_budget_allocate_device(const double *table, int64_t tiles, const int64_t *seg_first, int n_seg, uint32_t fmt_mask,
                                          const double *budget_bytes, int8_t *map, int64_t *counts, int32_t *status, void *scratch,
                                          size_t scratch_bytes, void *stream)
{
    if (!table || !seg_first || !budget_bytes || !map || !counts || !status || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (tiles <= 0 || tiles > (int64_t)1 << 31) return fail(MTQ_ERR_INVALID, "tiles must be in 1 .. 2^31");
    if (n_seg <= 0) return fail(MTQ_ERR_INVALID, "n_seg must be positive");
    if ((fmt_mask & 0xFu) == 0u) return fail(MTQ_ERR_INVALID, "fmt_mask names no tile format");
    if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(MTQ_ERR_INVALID, "scratch must be 8-byte aligned");
    if (scratch_bytes < mtq_budget_allocate_scratch_bytes(tiles, n_seg)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_budget_allocate_scratch_bytes(tiles, n_seg)");
    if (int rc = require_device()) return rc;
    // MIXED_TILE_BYTES_PER_ELEM; a dearer format has the lower code, so ascending (bytes, code) is descending code
    static const double kBpe[kNumFmt] = {2.0, 1.088, 0.50097, 0.25097};
    BudgetFormats F{};
    for (int f = kNumFmt - 1; f >= 0; --f)
        if (fmt_mask & (1u << f)) { F.code[F.P] = f; F.bytes[F.P] = 1024.0 * kBpe[f]; ++F.P; }
    for (int f = 0; f < kNumFmt; ++f) F.bpe[f] = kBpe[f];
    BudgetSeg *seg = static_cast<BudgetSeg *>(scratch);
    uint64_t *keys = reinterpret_cast<uint64_t *>(seg + n_seg);
    uint8_t *steps = reinterpret_cast<uint8_t *>(keys + tiles * 3);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(seg, 0, (size_t)n_seg * sizeof(BudgetSeg), st) != hipSuccess || hipMemsetAsync(counts, 0, (size_t)n_seg * kNumFmt * sizeof(int64_t), st) != hipSuccess)
        return fail(MTQ_ERR_HIP, "mtq_budget_allocate_device: hipMemsetAsync failed");
    const dim3 per_tile((unsigned)((tiles + kBThreads - 1) / kBThreads)), per_seg((unsigned)((n_seg + kBThreads - 1) / kBThreads));
    const dim3 per_chunk((unsigned)((tiles + kBThreads * kBPer - 1) / (kBThreads * kBPer)));
    hipLaunchKernelGGL(budget_hull_kernel, per_tile, dim3(kBThreads), 0, st, table, tiles, seg_first, n_seg, F, keys, steps, seg);
    if (int rc = check_launch("mtq_budget_allocate_device (hull)")) return rc;
    int tile_passes = 0;
    while (((int64_t)1 << tile_passes) < 4 * tiles + 2) ++tile_passes;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
    hipLaunchKernelGGL(budget_decide_kernel, per_seg, dim3(kBThreads), 0, st, seg, seg_first, n_seg, budget_bytes, F, (int)kBInit);
    for (int pass = 0; pass < 63 + tile_passes; ++pass) {
        hipLaunchKernelGGL(budget_count_kernel, per_chunk, dim3(kBThreads), 0, st, keys, steps, tiles, seg_first, n_seg, F, seg, (int8_t *)nullptr, cnt);
        hipLaunchKernelGGL(budget_decide_kernel, per_seg, dim3(kBThreads), 0, st, seg, seg_first, n_seg, budget_bytes, F,
                           pass < 62 ? (int)kBKey : pass == 62 ? (int)kBKeyLast : (int)kBTile);
    }
    if (int rc = check_launch("mtq_budget_allocate_device (select)")) return rc;
    hipLaunchKernelGGL(budget_count_kernel, per_chunk, dim3(kBThreads), 0, st, keys, steps, tiles, seg_first, n_seg, F, seg, map, cnt);
    hipLaunchKernelGGL(budget_status_kernel, per_seg, dim3(kBThreads), 0, st, seg, seg_first, n_seg, budget_bytes, F, status);
    return check_launch("mtq_budget_allocate_device");
}
