// mtq_transpose.hip — K1T / K2T: K1 and K2 of Xᵀ read straight from a row-major X (include/mtq.h, mtq_tile_stats_transposed and
// mtq_quantize_transposed).  The reference's `transpose` algorithm (compression_algorithms/transpose.py:13-33) quantises np.transpose(x),
// so a shared exponent covers 16 consecutive ROWS of one column of X: no transposed copy of X is ever made.
//
// K1T: one wave64 per unit of 32 rows × 128 columns of X = four 32×32 tiles of Xᵀ.  Lane 16s + j owns the columns c, c+1
// (c = 32·(4u + s) + 2j) over the unit's 32 rows: Xᵀ rows 2j, 2j+1 of tile s, i.e. the four groups of one row pair, which the lane sums
// sequentially in the documented order (column c rows 0-15, column c rows 16-31, column c+1 rows 0-15, column c+1 rows 16-31); the 16
// lanes of a tile then add their row pairs by the balanced tree (xor butterfly, lane 0's operand first, as tile_terms_literal does).
// Every load instruction of a wave reads one row of X over 128 consecutive columns (256 B of bf16, 512 B of float32): no cross-lane
// exponent reduction and no LDS.  The group arithmetic is the exact route of mtq_direct.hpp; a tile with a group outside its exponent
// range carries kRedoMagic in Σx and tile_stats_transposed_redo recomputes it by the literal route (group_terms_literal), one wave per
// tile, lane ℓ holding the group (Xᵀ row ℓ>>1, half ℓ&1) — the mapping and order of tile_terms_literal.
//
// K2T: one thread per (column, group of 16 rows); a wave's loads and stores are row segments of 64 consecutive columns.
//
// K3T: K2T's layout with a format per group read from a map over Xᵀ's grid (the mixed-tile searches with params["layout"] = "transpose").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mtq.h"
#include "mtq_device.hpp"
#include "mtq_direct.hpp"
#include "mtq_error.hpp"

namespace mtq {

constexpr unsigned long long kRedoMagicT = 0x7FF8C0DE5EED0001ull; // same pattern as the row-layout kernels
constexpr int kTUnitCols = 128;                                   // X columns per K1T wave (4 tiles of Xᵀ)

// The 32 rows × 2 columns a K1T lane owns, as raw fp32 words; elements outside the matrix read as +0.0.  pair_ok: the two columns
// of a row can be read as one 4-byte (bf16) / 8-byte (float32) word.
template <typename T> struct ColPair;

template <> struct ColPair<uint16_t> {
    uint32_t w[kTile];   // column c in the low half, c + 1 in the high half
    __device__ __forceinline__ void load(const uint16_t *__restrict__ p, int64_t r0, int64_t c, int64_t rows, int64_t cols, int64_t ld, bool pair_ok)
    {
        const bool both = pair_ok && c + 1 < cols;
#pragma unroll
        for (int i = 0; i < kTile; ++i) {
            const int64_t r = r0 + i;
            uint32_t v = 0u;
            if (r < rows) {
                if (both) v = *reinterpret_cast<const uint32_t *>(p + r * ld + c);
                else {
                    if (c < cols) v = p[r * ld + c];
                    if (c + 1 < cols) v |= (uint32_t)p[r * ld + c + 1] << 16;
                }
            }
            w[i] = v;
        }
    }
    // group g: (column c + (g >> 1), rows 16·(g & 1) .. +15)
    __device__ __forceinline__ void group(int g, uint32_t (&u)[kGroup]) const
    {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const uint32_t v = w[16 * (g & 1) + i];
            u[i] = (g >> 1) ? (v & 0xFFFF0000u) : (v << 16);
        }
    }
};

template <> struct ColPair<float> {
    uint32_t a[kTile], b[kTile];   // columns c and c + 1
    __device__ __forceinline__ void load(const float *__restrict__ p, int64_t r0, int64_t c, int64_t rows, int64_t cols, int64_t ld, bool pair_ok)
    {
        const bool both = pair_ok && c + 1 < cols;
#pragma unroll
        for (int i = 0; i < kTile; ++i) {
            const int64_t r = r0 + i;
            uint32_t va = 0u, vb = 0u;
            if (r < rows) {
                if (both) {
                    const uint2 v = *reinterpret_cast<const uint2 *>(p + r * ld + c);
                    va = v.x;
                    vb = v.y;
                } else {
                    if (c < cols) va = __float_as_uint(p[r * ld + c]);
                    if (c + 1 < cols) vb = __float_as_uint(p[r * ld + c + 1]);
                }
            }
            a[i] = va;
            b[i] = vb;
        }
    }
    __device__ __forceinline__ void group(int g, uint32_t (&u)[kGroup]) const
    {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) u[i] = (g >> 1) ? b[16 * (g & 1) + i] : a[16 * (g & 1) + i];
    }
};

// Units are numbered (matrix, 32-row block rb, 128-column block cu), cu fastest: neighbouring waves read neighbouring columns of the
// same rows.  Record of Xᵀ tile (cb, rb), cb = 4·cu + s: matrix·tiles + cb·tiles_h + rb, tiles_h = ceil(rows / 32).
template <typename T, uint32_t FM>
__global__ __launch_bounds__(256) void tile_stats_transposed(const T *__restrict__ x, int64_t stride, int64_t rows, int64_t cols, int64_t ld,
                                                            uint32_t tiles_h, uint32_t tiles_w, uint32_t units_c, int64_t units,
                                                            double *__restrict__ stats, int pair_ok, unsigned *__restrict__ work, unsigned launch_id)
{
    constexpr int nf = popc4(FM), rec = 2 + 5 * nf;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= units) return;                                               // wave-uniform
    const int lane = threadIdx.x & 63, seg = lane >> 4, j = lane & 15;
    const int64_t per = (int64_t)tiles_h * units_c;
    const int64_t b = unit / per, rem = unit - b * per;
    const uint32_t rb = (uint32_t)(rem / units_c), cu = (uint32_t)(rem - (int64_t)rb * units_c);
    const uint32_t cb = 4u * cu + (uint32_t)seg;                             // this lane's tile row of Xᵀ (column block of X)
    const int64_t c = (int64_t)cb * kTile + 2 * j;

    ColPair<T> cp;
    cp.load(x + b * stride, (int64_t)rb * kTile, c, rows, cols, ld, pair_ok != 0);

    double acc[rec];
    bool bad = false;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                            // the row pair's four groups, sequentially
        uint32_t u[kGroup];
        cp.group(g, u);
        double s[kMaxSums];
        float mx[kNumFmt];
        bool bg;
        direct_group<FM, sizeof(T) == 2>(u, s, mx, bg);
        bad = bad || bg;
        if (g == 0) {
            acc[0] = s[0];
            acc[1] = s[1];
#pragma unroll
            for (int f = 0; f < nf; ++f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[2 + 5 * f + k] = s[2 + 4 * f + k];
                acc[2 + 5 * f + 4] = (double)mx[f];
            }
        } else {
            acc[0] = acc[0] + s[0];
            acc[1] = acc[1] + s[1];
#pragma unroll
            for (int f = 0; f < nf; ++f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[2 + 5 * f + k] = acc[2 + 5 * f + k] + s[2 + 4 * f + k];
                acc[2 + 5 * f + 4] = fmax(acc[2 + 5 * f + 4], (double)mx[f]);   // never NaN on the exact route
            }
        }
    }
#pragma unroll
    for (int k = 0; k < rec; ++k) {                                          // 16 row pairs: balanced tree inside the 16 lanes of a tile
        const bool is_max = k >= 2 && ((k - 2) % 5) == 4;
        double v = acc[k];
#pragma unroll
        for (int sft = 1; sft < 16; sft <<= 1) {
            const double o = __shfl_xor(v, sft, 64);
            v = is_max ? fmax(v, o) : v + o;
        }
        acc[k] = v;
    }
    const bool tile_bad = ((__ballot(bad) >> (16 * seg)) & 0xFFFFull) != 0ull;
    if (j == 0 && cb < tiles_w) {
        double *out = stats + (b * tiles_w + cb) * (int64_t)tiles_h * rec + (int64_t)rb * rec;
        if (tile_bad) {
            acc[0] = __longlong_as_double((long long)kRedoMagicT);
            work[kWorkStamp] = launch_id;                                    // tells the follow-up kernel there is something to redo
        }
#pragma unroll
        for (int k = 0; k < rec; ++k) out[k] = acc[k];
    }
}

// Follow-up of K1T: records whose Σx carries kRedoMagic are recomputed by the literal route (non-finite values, denormal-only groups,
// exponent spreads the exact route does not take).  Returns at once unless K1T stamped this launch's id.
template <typename T>
__global__ __launch_bounds__(256) void tile_stats_transposed_redo(const T *__restrict__ x, int64_t count, int64_t stride, int64_t rows, int64_t cols,
                                                                 int64_t ld, uint32_t tiles_h, int64_t tiles, uint32_t fmt_mask, int rec,
                                                                 double *__restrict__ stats, const unsigned *__restrict__ work, unsigned launch_id)
{
    if (work[kWorkStamp] != launch_id) return;
    const int lane = threadIdx.x & 63;
    const int64_t total = count * tiles;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; first < total; first += (int64_t)gridDim.x * 4 * 64) {
        const int64_t mine = first + lane;
        bool flagged = false;
        if (mine < total) flagged = (unsigned long long)__double_as_longlong(stats[mine * rec]) == kRedoMagicT;
        unsigned long long todo = __ballot(flagged);
        while (todo) {                                                       // wave-uniform loop over the flagged tiles
            const int64_t gt = first + __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t b = gt / tiles, t = gt - b * tiles;
            const int64_t cb = t / tiles_h, rb = t - cb * tiles_h;
            // lane ℓ: Xᵀ row ℓ>>1 of the tile = column cb·32 + (ℓ>>1) of X, half ℓ&1 = rows rb·32 + 16·(ℓ&1) .. +15
            const int64_t c = cb * kTile + (lane >> 1), r0 = rb * kTile + (lane & 1) * kGroup;
            const T *p = x + b * stride;
            uint32_t u[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                uint32_t v = 0u;
                if (c < cols && r0 + i < rows) {
                    if constexpr (sizeof(T) == 2) v = (uint32_t)p[(r0 + i) * ld + c] << 16;
                    else v = __float_as_uint(p[(r0 + i) * ld + c]);
                }
                u[i] = v;
            }
            double acc[2 + 5 * kNumFmt];
            tile_terms_literal(u, fmt_mask, acc);
            if (lane == 0) {
                double *out = stats + gt * rec;
                out[0] = acc[0];
                out[1] = acc[1];
                int o = 2;
#pragma unroll
                for (int f = 0; f < kNumFmt; ++f)
                    if (fmt_mask & (1u << f)) {
#pragma unroll
                        for (int k = 0; k < 5; ++k) out[o + k] = acc[2 + 5 * f + k];
                        o += 5;
                    }
            }
        }
    }
}

// K2T: y[r][c] = the element (c, r) of quantize(Xᵀ): the group is rows 16g .. 16g+15 of column c.
template <typename T>
__global__ __launch_bounds__(256) void quantize_transposed(const T *__restrict__ x, int64_t rows, int64_t cols, int64_t ld, int64_t row_groups, int fmt,
                                                          float *__restrict__ y, int64_t ldy)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    for (int64_t g = blockIdx.y; g < row_groups; g += gridDim.y) {
        const int64_t r0 = g * kGroup;
        uint32_t u[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            uint32_t v = 0u;
            if (r0 + i < rows) {
                if constexpr (sizeof(T) == 2) v = (uint32_t)x[(r0 + i) * ld + c] << 16;
                else v = __float_as_uint(x[(r0 + i) * ld + c]);
            }
            u[i] = v;
        }
        const uint32_t shared = group_shared_exp(u);
#pragma unroll
        for (int i = 0; i < kGroup; ++i)
            if (r0 + i < rows) y[(r0 + i) * ldy + c] = __uint_as_float(quant_elem_bits(fmt, u[i], shared));
    }
}

// K3T: y[r][c] = the element (c, r) of K3 of Xᵀ with `map` (Xᵀ's grid, row-major): the group is rows 16g .. 16g+15 of column c and
// lies in Xᵀ tile (c / 32, r0 / 32).  The thread layout of K2T; blockIdx.z walks the matrices of a batch.
template <typename T>
__global__ __launch_bounds__(256) void apply_assignment_transposed(const T *__restrict__ x, int64_t count, int64_t stride, int64_t rows, int64_t cols,
                                                                  int64_t ld, int64_t row_groups, int64_t tiles_w, int64_t tiles,
                                                                  const int8_t *__restrict__ map, float *__restrict__ y, int64_t ldy)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    for (int64_t b = blockIdx.z; b < count; b += gridDim.z) {
        const T *xb = x + b * stride;
        float *yb = y + b * rows * ldy;
        const int8_t *mb = map + b * tiles + (c / kTile) * tiles_w;
        for (int64_t g = blockIdx.y; g < row_groups; g += gridDim.y) {
            const int64_t r0 = g * kGroup;
            uint32_t u[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                uint32_t v = 0u;
                if (r0 + i < rows) {
                    if constexpr (sizeof(T) == 2) v = (uint32_t)xb[(r0 + i) * ld + c] << 16;
                    else v = __float_as_uint(xb[(r0 + i) * ld + c]);
                }
                u[i] = v;
            }
            const uint32_t shared = group_shared_exp(u);
            const int f = mb[r0 / kTile];
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (r0 + i < rows) yb[(r0 + i) * ldy + c] = __uint_as_float(quant_elem_bits(f, u[i], shared));
        }
    }
}

// K3T, vector form (cols % 4 == 0, rows of X and y aligned for 4-element words): a thread owns four adjacent columns, so a wave's load
// is 512 B (bf16) / 1 KiB (float32) of one row and its store 1 KiB.  The four columns lie in one Xᵀ tile row and share a map entry.
template <typename T>
__global__ __launch_bounds__(256) void apply_assignment_transposed_quad(const T *__restrict__ x, int64_t count, int64_t stride, int64_t rows,
                                                                       int64_t cols, int64_t ld, int64_t row_groups, int64_t tiles_w, int64_t tiles,
                                                                       const int8_t *__restrict__ map, float *__restrict__ y, int64_t ldy)
{
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= cols) return;                                                   // cols % 4 == 0: c .. c + 3 are all inside
    for (int64_t b = blockIdx.z; b < count; b += gridDim.z) {
        const T *xb = x + b * stride;
        float *yb = y + b * rows * ldy;
        const int8_t *mb = map + b * tiles + (c / kTile) * tiles_w;
        for (int64_t g = blockIdx.y; g < row_groups; g += gridDim.y) {
            const int64_t r0 = g * kGroup;
            uint32_t u[4][kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                uint32_t v[4] = {0u, 0u, 0u, 0u};
                if (r0 + i < rows) {
                    if constexpr (sizeof(T) == 2) {
                        const uint2 w = *reinterpret_cast<const uint2 *>(xb + (r0 + i) * ld + c);
                        v[0] = w.x << 16; v[1] = w.x & 0xFFFF0000u; v[2] = w.y << 16; v[3] = w.y & 0xFFFF0000u;
                    } else {
                        const uint4 w = *reinterpret_cast<const uint4 *>(xb + (r0 + i) * ld + c);
                        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) u[k][i] = v[k];
            }
            uint32_t shared[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) shared[k] = group_shared_exp(u[k]);
            const int f = mb[r0 / kTile];
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (r0 + i < rows)
                    *reinterpret_cast<uint4 *>(yb + (r0 + i) * ldy + c) = make_uint4(quant_elem_bits(f, u[0][i], shared[0]), quant_elem_bits(f, u[1][i], shared[1]),
                                                                                     quant_elem_bits(f, u[2][i], shared[2]), quant_elem_bits(f, u[3][i], shared[3]));
        }
    }
}

template <typename T>
static void launch_transposed(uint32_t fm, dim3 grid, hipStream_t st, const T *x, int64_t stride, int64_t rows, int64_t cols, int64_t ld,
                              uint32_t tiles_h, uint32_t tiles_w, uint32_t units_c, int64_t units, double *stats, int pair_ok, unsigned *work,
                              unsigned launch_id)
{
#define MTQ_LAUNCH_T(M) \
    case M: hipLaunchKernelGGL((tile_stats_transposed<T, M>), grid, dim3(256), 0, st, x, stride, rows, cols, ld, tiles_h, tiles_w, units_c, units, \
                               stats, pair_ok, work, launch_id); break;
    switch (fm) { // one instantiation per requested format subset, as the row-layout direct kernel
        MTQ_LAUNCH_T(1u) MTQ_LAUNCH_T(2u) MTQ_LAUNCH_T(3u) MTQ_LAUNCH_T(4u) MTQ_LAUNCH_T(5u) MTQ_LAUNCH_T(6u) MTQ_LAUNCH_T(7u) MTQ_LAUNCH_T(8u)
        MTQ_LAUNCH_T(9u) MTQ_LAUNCH_T(10u) MTQ_LAUNCH_T(11u) MTQ_LAUNCH_T(12u) MTQ_LAUNCH_T(13u) MTQ_LAUNCH_T(14u) MTQ_LAUNCH_T(15u)
    default: break;
    }
#undef MTQ_LAUNCH_T
}

} // namespace mtq

using namespace mtq;

extern "C" int mtq_tile_stats_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                         uint32_t fmt_mask, double *stats, void *stream)
{
    if (!x || !stats) return fail(MTQ_ERR_INVALID, "null argument");
    if (in_dtype != MTQ_DTYPE_BF16 && in_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "in_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (count < 1) return fail(MTQ_ERR_INVALID, "count must be positive");
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty tensors are handled by the caller)");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (count > 1 && stride_elems < 0) return fail(MTQ_ERR_INVALID, "stride_elems must not be negative");
    if ((fmt_mask & MTQ_MASK_ALL) == 0 || (fmt_mask & ~MTQ_MASK_ALL) != 0) return fail(MTQ_ERR_INVALID, "fmt_mask must name 1..4 of bf16|bfp8|bfp4|bfp2 and nothing else");
    if (rows > (int64_t)1 << 30 || cols > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t th = (rows + kTile - 1) / kTile, tw = (cols + kTile - 1) / kTile, tiles = th * tw;
    const int64_t units_c = (cols + kTUnitCols - 1) / kTUnitCols, units = count * th * units_c;
    if (count * tiles >= ((int64_t)1 << 33) || (units + 3) / 4 > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many tiles for one launch");
    if (int rc = require_device()) return rc;
    const int64_t esz = in_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    const int pair_ok = (reinterpret_cast<uintptr_t>(x) % (uintptr_t)(2 * esz)) == 0 && ld % 2 == 0 && (count == 1 || stride_elems % 2 == 0);
    const int rec = 2 + 5 * popc4(fmt_mask);
    hipStream_t st = static_cast<hipStream_t>(stream);
    WorkSlot work;
    if (int rc = work_counter_acquire(stream, &work)) return rc;
    const unsigned launch_id = next_launch_id();
    const dim3 grid((unsigned)((units + 3) / 4));
    if (in_dtype == MTQ_DTYPE_BF16)
        launch_transposed<uint16_t>(fmt_mask, grid, st, static_cast<const uint16_t *>(x), stride_elems, rows, cols, ld, (uint32_t)th, (uint32_t)tw,
                                    (uint32_t)units_c, units, stats, pair_ok, work.counters, launch_id);
    else
        launch_transposed<float>(fmt_mask, grid, st, static_cast<const float *>(x), stride_elems, rows, cols, ld, (uint32_t)th, (uint32_t)tw,
                                 (uint32_t)units_c, units, stats, pair_ok, work.counters, launch_id);
    if (int rc = check_launch("mtq_tile_stats_transposed")) {
        work_counter_abandon(work);
        return rc;
    }
    const dim3 rgrid((unsigned)std::min<int64_t>(((count * tiles + 63) / 64 + 3) / 4, 512));
    if (in_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(tile_stats_transposed_redo<uint16_t>, rgrid, dim3(256), 0, st, static_cast<const uint16_t *>(x), count, stride_elems, rows, cols,
                           ld, (uint32_t)th, tiles, fmt_mask, rec, stats, work.counters, launch_id);
    else
        hipLaunchKernelGGL(tile_stats_transposed_redo<float>, rgrid, dim3(256), 0, st, static_cast<const float *>(x), count, stride_elems, rows, cols, ld,
                           (uint32_t)th, tiles, fmt_mask, rec, stats, work.counters, launch_id);
    const int rc = check_launch("mtq_tile_stats_transposed (redo flagged)");
    work_counter_release(work, stream);   // K1T leaves the slot's unit counters untouched (zero): only its stamp word is written
    return rc;
}

extern "C" int mtq_quantize_transposed(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld, int fmt, float *y, int64_t ldy, void *stream)
{
    if (!x || !y) return fail(MTQ_ERR_INVALID, "null argument");
    if (in_dtype != MTQ_DTYPE_BF16 && in_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "in_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty tensors are handled by the caller)");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (ldy < cols) return fail(MTQ_ERR_INVALID, "ldy < cols");
    if (fmt < MTQ_FMT_BF16 || fmt > MTQ_FMT_FP0) return fail(MTQ_ERR_UNSUPPORTED, "format code must be 0..4 (bf16,bfp8,bfp4,bfp2,fp0)");
    if (rows > (int64_t)1 << 40 || cols > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (int rc = require_device()) return rc;
    const int64_t row_groups = (rows + kGroup - 1) / kGroup;
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)std::min<int64_t>(row_groups, 65535));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (in_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(quantize_transposed<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), rows, cols, ld, row_groups, fmt, y, ldy);
    else
        hipLaunchKernelGGL(quantize_transposed<float>, grid, dim3(256), 0, st, static_cast<const float *>(x), rows, cols, ld, row_groups, fmt, y, ldy);
    return check_launch("mtq_quantize_transposed");
}

extern "C" int mtq_apply_assignment_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                               const int8_t *map, float *y, int64_t ldy, void *stream)
{
    if (!x || !y || !map) return fail(MTQ_ERR_INVALID, "null argument");
    if (in_dtype != MTQ_DTYPE_BF16 && in_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "in_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (count < 1) return fail(MTQ_ERR_INVALID, "count must be positive");
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty tensors are handled by the caller)");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (ldy < cols) return fail(MTQ_ERR_INVALID, "ldy < cols");
    if (count > 1 && stride_elems < 0) return fail(MTQ_ERR_INVALID, "stride_elems must not be negative");
    if (rows > (int64_t)1 << 30 || cols > (int64_t)1 << 30 || count * rows * ldy > ((int64_t)1 << 40)) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (int rc = require_device()) return rc;
    const int64_t row_groups = (rows + kGroup - 1) / kGroup, tw = (rows + kTile - 1) / kTile, tiles = tw * ((cols + kTile - 1) / kTile);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t esz = in_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    const bool quad = cols % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (uintptr_t)(4 * esz) == 0 && ld % 4 == 0 && (count == 1 || stride_elems % 4 == 0) &&
                      reinterpret_cast<uintptr_t>(y) % 16 == 0 && ldy % 4 == 0;
    if (quad) {
        const dim3 qgrid((unsigned)((cols / 4 + 255) / 256), (unsigned)std::min<int64_t>(row_groups, 65535), (unsigned)std::min<int64_t>(count, 65535));
        if (in_dtype == MTQ_DTYPE_BF16)
            hipLaunchKernelGGL(apply_assignment_transposed_quad<uint16_t>, qgrid, dim3(256), 0, st, static_cast<const uint16_t *>(x), count, stride_elems, rows,
                               cols, ld, row_groups, tw, tiles, map, y, ldy);
        else
            hipLaunchKernelGGL(apply_assignment_transposed_quad<float>, qgrid, dim3(256), 0, st, static_cast<const float *>(x), count, stride_elems, rows, cols,
                               ld, row_groups, tw, tiles, map, y, ldy);
        return check_launch("mtq_apply_assignment_transposed");
    }
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)std::min<int64_t>(row_groups, 65535), (unsigned)std::min<int64_t>(count, 65535));
    if (in_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(apply_assignment_transposed<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), count, stride_elems, rows, cols,
                           ld, row_groups, tw, tiles, map, y, ldy);
    else
        hipLaunchKernelGGL(apply_assignment_transposed<float>, grid, dim3(256), 0, st, static_cast<const float *>(x), count, stride_elems, rows, cols, ld,
                           row_groups, tw, tiles, map, y, ldy);
    return check_launch("mtq_apply_assignment_transposed");
}
