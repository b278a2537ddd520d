// mtq_packed.hip — the packed mixed-tile weight: the bytes a tile map promises, and a linear layer that multiplies with them.
//
// Format (include/mtq.h, DESIGN.md "Packed mixed-tile weights"): row layout only.  Tile t = tr * tiles_w + tc of the zero-padded 2-D
// flatten is one blob at packed + 64 * offsets[t], of 2048 / 1088 / 576 / 320 bytes for the map codes 0..3 (bf16, bfp8, bfp4, bfp2).
// A BFP blob is 64 shared-exponent bytes (group g = 2 * row + half, 16 consecutive columns of one row) and then the element codes
// (sign << M) | man in row-major order e = 32 * row + col: one byte each (bfp8), two per byte with even e in the low nibble (bfp4), four
// per byte with e at bits 2(e % 4) (bfp2).  A bf16 blob is 1024 little-endian uint16, the upper halves of bf16_round_bits.  Group g's
// codes are therefore the 16 / 8 / 4 (or, bf16, 32) contiguous bytes at 64 + 16g / 8g / 4g (32g): one lane, one vector access.
//
//   pack_tiles_kernel / unpack_tiles_kernel   one wave per tile, one lane per group; the format is uniform across the wave.
//   packed_offsets_batched_kernel, packed_bases_kernel, pack_tiles_batched_kernel / unpack_tiles_batched_kernel
//                                             a batch of equal-shaped tensors into one arena: the offsets of every map and the tensors'
//       bases by block scans on the device (plain stores, no atomics, no waiting between workgroups), then one wave per (tensor, tile)
//       through the same per-tile bodies as the single-tensor kernels.
//   packed_linear_kernel                      Y = X·Ŵᵀ + b in the shape of mtq_output_error.hip: a workgroup of 4 waves owns a
//       128 (M) × 64 (N) block and walks K in steps of 64; per step each of the 256 lanes takes one group of the 64 × 64 W block, reads
//       its exponent byte and its code bytes and decodes them into the bf16 LDS image (every BFP value has its low 16 bits zero: the
//       image is exact), X goes to LDS beside it, mfma_f32_32x32x16_bf16 accumulates in f32.  One accumulator, one K order per output,
//       no atomics: the same inputs give the same bits.
//   packed_linear_skinny_kernel               the same product for m <= 32: one wave per (K slice, tile row), W straight to registers.
//   packed_linear_skinny_grouped_kernel       that wave's work for every expert of an arena over the expert's own rows of X, one launch:
//       for decode-sized groups (a group above 32 rows is walked in chunks and re-reads W; the block kernel is the route for large m).
//   packed_grouped_plan_kernel<32>, packed_linear_skinny_grouped_chunked_kernel
//                                             the same product and bits with a wave per 32-row chunk of a group, for hot experts: the
//       groups' chunk counts are prefix-summed on the device before the launch and each wave finds its group by a search of that prefix.
//   packed_wide_kernel<.., WT = false>        the block kernel's bits from a 128 × 128 block whose waves decode whole tiles: for m >= 64.
//   packed_grouped_plan_kernel<128>, packed_wide_grouped_kernel<.., WT = false>
//                                             that block for every expert of an arena over the expert's own rows, one launch: the groups'
//       128-row block counts are prefix-summed on the device and each workgroup finds its group by the chunked kernel's search.
//   packed_glu_wide_kernel<.., WT = false>, packed_glu_wide_grouped_kernel<.., WT = false>, glu_combine_kernel
//                                             the gated MLP's first half, glu_value(X·Ŵgᵀ + bg, X·Ŵuᵀ + bu): the wide kernel's step on a
//       128 × 64 block whose four tile-row slots alternate between the gate and the up stream, so a lane holds both projections of its
//       outputs; the same block in the grouped wide frame; and the element-wise combine that finishes the unfused route with the same
//       function (mtq_glu.hpp) and so the same bits.
//   pack_tiles_transposed_kernel / unpack_tiles_transposed_kernel
//                                             the stream of the TRANSPOSE of a stored matrix, read / written in the stored orientation: a
//       map over the transposed layout of W is a row-layout map of Wᵀ, so this is the same format (no new bytes, no new layout value).
//   pack_tiles_transposed_batched_kernel / unpack_tiles_transposed_batched_kernel
//                                             that pair for a batch and its arena, one wave per (tensor, tile); the pack reads each tile's
//       region of w by rows into a wave-private LDS image and gathers the column groups from it.
//   packed_matmul_kernel                      Y = X·P̂ + b for a packed k × n matrix: the block kernel's frame over a [k][n] LDS image
//       that is read with the transposed LDS read (ds_read_b64_tr_b16); bit for bit the block kernel on the transposed weight.
//   packed_matmul_skinny_kernel               that product for m <= 32: one wave per (K slice, tile column), each tile through a
//       wave-private [32 k][32 n] LDS image and the transposed read; bit for bit the skinny linear kernel on the transposed weight.
//   packed_wide_kernel<.., WT = true>         that product for m >= 64: the wide block with its W side fed from the k × n stream, four
//       [64 k][32 n] sub-images read through the transposed LDS read; bit for bit packed_matmul_kernel.  packed_wide_grouped_kernel<..,
//       WT = true> is that block for every (k, n) expert of an arena.
//   packed_glu_wide_kernel<.., WT = true>, packed_glu_wide_grouped_kernel<.., WT = true>, packed_glu_matmul_skinny_kernel,
//   packed_glu_matmul_skinny_grouped_kernel   the gated product for packed k × n gate and up matrices: the four gated frames with the
//       matmul kernels' feed (the wide block's [64 k][32 n] sub-images alternating between the two streams; the skinny wave's two
//       images on the projection axis); bit for bit two matmul calls into f32 and the combine.
//   packed_glu_skinny_grouped_kernel<GATHER = true>, packed_glu_matmul_skinny_grouped_kernel<GATHER = true>, skinny_grouped_combine_kernel
//                                             an MoE layer's decode route without its staging copies (include/mtq_moe_decode.h): the two
//       grouped skinny GLU waves reading their X groups from the token's own row through the plan's src (mtq_moe_dispatch's rule, its
//       bits), and the grouped skinny down projection's reduce with mtq_moe_combine's weighted sum in it.
//   packed_glu_skinny_grouped_chunked_kernel<GATHER>, packed_glu_matmul_skinny_grouped_chunked_kernel<GATHER>,
//   glu_skinny_grouped_chunked_reduce_kernel  the grouped skinny GLU waves with a wave per 32-row chunk of a group, on the chunked linear
//       kernels' plan and search (include/mtq_glu_chunked.h): the walking kernels' bits, for routings with hot experts; the reduce
//       takes a workgroup per chunk slot.  The down projection with the combine uses the chunked linear kernels as they stand.
//
// The wide kernels are frames around one block function, wide_block; the skinny kernels around one wave's run, skinny_run, and one
// epilogue, store_lane_rows; all of them read a tensor through a PackedStream and guard a blob with stream_at.
//
// Every blob is checked against the buffer's length on the device before it is touched (offsets come from the caller): a tile whose
// blob does not fit is not written (pack), not stored (unpack) or read as zeros (linear).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "mtq_device.hpp"
#include "mtq_error.hpp"
#include "mtq_glu.hpp"

namespace mtq {
namespace {

constexpr int kUnit = 64;                           // offsets count units of 64 bytes
constexpr int kExpBytes = 64;                       // shared exponents at the head of a BFP blob

__host__ __device__ constexpr uint32_t packed_tile_bytes(int f)
{
    return f == 0 ? 2048u : (f == 1 ? 1088u : (f == 2 ? 576u : (f == 3 ? 320u : 0u)));
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 16 float32 words with zero low halves → 16 bf16, 32 bytes
__device__ __forceinline__ void pack_halves(const uint32_t (&y)[kGroup], uint4 &lo, uint4 &hi)
{
    uint32_t pk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pk[i] = (y[2 * i] >> 16) | (y[2 * i + 1] & 0xFFFF0000u);
    lo = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    hi = make_uint4(pk[4], pk[5], pk[6], pk[7]);
}

// The raw bytes of one group as a lane holds them: w[0..7] little-endian (32 bytes for bf16, 16 / 8 / 4 for bfp8 / bfp4 / bfp2).
struct GroupRaw {
    uint32_t w[8];
    uint32_t E;
    int f;                                           // 0..3, anything else: zeros
};

template <int F>
__device__ __forceinline__ void decode_as(const GroupRaw &g, uint32_t (&y)[kGroup])
{
    constexpr uint32_t M = F == 1 ? 7u : (F == 2 ? 3u : 1u);
    constexpr uint32_t B = M + 1u;                  // bits per code
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const uint32_t code = (g.w[(i * B) >> 5] >> ((i * B) & 31u)) & ((1u << B) - 1u);
        y[i] = bfp_code_bits_rt(code, g.E, M);
    }
}

__device__ __forceinline__ void decode_group(const GroupRaw &g, uint32_t (&y)[kGroup])
{
    if (g.f == 0) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = (i & 1) ? (g.w[i >> 1] & 0xFFFF0000u) : (g.w[i >> 1] << 16);
    } else if (g.f == 1) {
        decode_as<1>(g, y);
    } else if (g.f == 2) {
        decode_as<2>(g, y);
    } else if (g.f == 3) {
        decode_as<3>(g, y);
    } else {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = 0u;
    }
}

// Where tile t's blob is and what it holds: f < 0 when the tile's code is no format or its blob passes the end of the buffer.
struct TileAt {
    uint64_t off;
    int f;
};

__device__ __forceinline__ TileAt tile_at(uint64_t packed_bytes, const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets, int64_t t,
                                          uint64_t base = 0)   // base: where the tensor's stream starts in an arena, in units
{
    TileAt a;
    const int f = map[t];
    a.off = (base + offsets[t]) * kUnit;
    const uint32_t size = packed_tile_bytes(f);
    a.f = (size == 0u || a.off + size > packed_bytes) ? -1 : f;
    return a;
}

// Group gi (0..63) of the blob at `a`.
__device__ __forceinline__ void load_group(const uint8_t *__restrict__ packed, const TileAt &a, int gi, GroupRaw &g)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) g.w[i] = 0u;
    g.E = 0u;
    g.f = a.f;
    if (a.f < 0) return;
    const int f = a.f;
    const uint8_t *blob = packed + a.off;
    if (f == 0) {
        const uint4 *q = reinterpret_cast<const uint4 *>(blob + gi * 32);
        const uint4 lo = q[0], hi = q[1];
        g.w[0] = lo.x; g.w[1] = lo.y; g.w[2] = lo.z; g.w[3] = lo.w;
        g.w[4] = hi.x; g.w[5] = hi.y; g.w[6] = hi.z; g.w[7] = hi.w;
        return;
    }
    g.E = blob[gi];
    if (f == 1) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blob + kExpBytes + gi * 16);
        g.w[0] = v.x; g.w[1] = v.y; g.w[2] = v.z; g.w[3] = v.w;
    } else if (f == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(blob + kExpBytes + gi * 8);
        g.w[0] = v.x; g.w[1] = v.y;
    } else {
        g.w[0] = *reinterpret_cast<const uint32_t *>(blob + kExpBytes + gi * 4);
    }
}

// ---- pack: lane = group (row lane >> 1, half lane & 1) of the wave's tile
// The group's 16 float32 words u → its bytes in the blob of format f (0..3): the same for whichever way the words were fetched.
__device__ __forceinline__ void pack_group(const uint32_t (&u)[kGroup], int f, int lane, uint8_t *__restrict__ blob)
{
    if (f == 0) {
        uint32_t y[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
        uint4 lo, hi;
        pack_halves(y, lo, hi);
        uint4 *d = reinterpret_cast<uint4 *>(blob + lane * 32);
        d[0] = lo;
        d[1] = hi;
        return;
    }
    const uint32_t E = group_shared_exp(u);
    const uint32_t M = f == 1 ? 7u : (f == 2 ? 3u : 1u), B = M + 1u;
    blob[lane] = (uint8_t)E;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const uint32_t code = bfp_code_rt(u[i], E, M);
        if (f == 1) w[i >> 2] |= code << (8 * (i & 3));
        else if (f == 2) w[i >> 3] |= code << (4 * (i & 7));
        else w[0] |= code << (2 * i);
    }
    uint8_t *dst = blob + kExpBytes + lane * (2 * (int)B);   // 16 codes of B bits
    if (f == 1) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else if (f == 2) *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
    else *reinterpret_cast<uint32_t *>(dst) = w[0];
}

// Tile t (format f, 0..3) of the rows × cols matrix x → the blob: what one wave does, for the single-tensor and the batched kernel alike.
template <typename T>
__device__ __forceinline__ void pack_tile(const T *__restrict__ x, int64_t rows, int64_t cols, int64_t ld, bool vec_ok, int64_t tiles_w, int64_t t,
                                          int f, int lane, uint8_t *__restrict__ blob)
{
    const int64_t row = (t / tiles_w) * kTile + (lane >> 1), col0 = (t % tiles_w) * kTile + kGroup * (lane & 1);
    uint32_t u[kGroup];
    Loader<T>::group(x, row, col0, rows, cols, ld, vec_ok, u);
    pack_group(u, f, lane, blob);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_tiles_kernel(const T *__restrict__ x, int64_t rows, int64_t cols, int64_t ld, int vec_ok,
                                                         const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets, int64_t tiles,
                                                         int64_t tiles_w, uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4) {
        const int f = map[t];
        const uint32_t size = packed_tile_bytes(f);
        const uint64_t off = (uint64_t)offsets[t] * kUnit;
        if (size == 0u || off + size > out_bytes) continue;   // wave-uniform
        pack_tile(x, rows, cols, ld, vec_ok != 0, tiles_w, t, f, lane, out + off);
    }
}

// The transposed entry: w is rows × cols as stored and the stream is that of wᵀ (cols × rows), whose grid the map, the offsets, `tiles` and
// `tiles_w` (= ceil(rows / 32)) describe.  The lane's group is row c = 32 tr + lane / 2 of wᵀ, columns r0 = 32 tc + 16 (lane & 1) ..: 16
// consecutive rows of column c of w.  For a fixed value index the wave reads two runs of 32 consecutive elements of a row of w.
__device__ __forceinline__ uint32_t word_of(const uint16_t *__restrict__ p, int64_t at) { return (uint32_t)p[at] << 16; }
__device__ __forceinline__ uint32_t word_of(const float *__restrict__ p, int64_t at) { return __float_as_uint(p[at]); }

template <typename T>
__global__ __launch_bounds__(256) void pack_tiles_transposed_kernel(const T *__restrict__ w, int64_t rows, int64_t cols, int64_t ld,
                                                                    const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets,
                                                                    int64_t tiles, int64_t tiles_w, uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4) {
        const int f = map[t];
        const uint32_t size = packed_tile_bytes(f);
        const uint64_t off = (uint64_t)offsets[t] * kUnit;
        if (size == 0u || off + size > out_bytes) continue;   // wave-uniform
        const int64_t c = (t / tiles_w) * kTile + (lane >> 1), r0 = (t % tiles_w) * kTile + kGroup * (lane & 1);
        uint32_t u[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) u[i] = (c < cols && r0 + i < rows) ? word_of(w, (r0 + i) * ld + c) : 0u;
        pack_group(u, f, lane, out + off);
    }
}

// The batch: wave g of count * tiles takes tile t = g % tiles of tensor i = g / tiles, whose matrix starts i * stride elements into x and
// whose stream starts at unit bases[i] of the arena `out`.  maps [count][tiles], offsets [count][tiles + 1].
template <typename T>
__global__ __launch_bounds__(256) void pack_tiles_batched_kernel(const T *__restrict__ x, int64_t count, int64_t rows, int64_t cols, int64_t ld,
                                                                 int64_t stride, int vec_ok, const int8_t *__restrict__ maps,
                                                                 const uint32_t *__restrict__ offsets, const uint64_t *__restrict__ bases,
                                                                 int64_t tiles, int64_t tiles_w, uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = count * tiles;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < total; g += (int64_t)gridDim.x * 4) {
        const int64_t i = g / tiles, t = g - i * tiles;
        const int f = maps[g];
        const uint32_t size = packed_tile_bytes(f);
        const uint64_t off = (bases[i] + offsets[i * (tiles + 1) + t]) * kUnit;
        if (size == 0u || off > out_bytes || size > out_bytes - off) continue;   // wave-uniform
        pack_tile(x + i * stride, rows, cols, ld, vec_ok != 0, tiles_w, t, f, lane, out + off);
    }
}

// ---- unpack: the same ownership; y float32 (the words) or bf16 (their upper halves)
// The blob at `a` → tile t of the rows × cols matrix y: a tile whose blob is not there stores nothing, nor does a lane past an edge.
template <bool BF16OUT>
__device__ __forceinline__ void unpack_tile(const uint8_t *__restrict__ packed, const TileAt &a, int64_t tiles_w, int64_t t, int lane, int64_t rows,
                                            int64_t cols, void *__restrict__ yv, int64_t ldy, bool vec_ok)
{
    const int64_t row = (t / tiles_w) * kTile + (lane >> 1), col0 = (t % tiles_w) * kTile + kGroup * (lane & 1);
    GroupRaw g;
    load_group(packed, a, lane, g);
    if (g.f < 0 || row >= rows || col0 >= cols) return;
    uint32_t y[kGroup];
    decode_group(g, y);
    const bool whole = col0 + kGroup <= cols && vec_ok;
    if constexpr (BF16OUT) {
        uint16_t *yr = static_cast<uint16_t *>(yv) + row * ldy + col0;
        if (whole) {
            uint4 lo, hi;
            pack_halves(y, lo, hi);
            reinterpret_cast<uint4 *>(yr)[0] = lo;
            reinterpret_cast<uint4 *>(yr)[1] = hi;
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (col0 + i < cols) yr[i] = (uint16_t)(y[i] >> 16);
        }
    } else {
        uint32_t *yr = static_cast<uint32_t *>(yv) + row * ldy + col0;
        if (whole) {
#pragma unroll
            for (int i = 0; i < 4; ++i) reinterpret_cast<uint4 *>(yr)[i] = make_uint4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (col0 + i < cols) yr[i] = y[i];
        }
    }
}

template <bool BF16OUT>
__global__ __launch_bounds__(256) void unpack_tiles_kernel(const uint8_t *__restrict__ packed, uint64_t packed_bytes, const int8_t *__restrict__ map,
                                                           const uint32_t *__restrict__ offsets, int64_t tiles, int64_t tiles_w, int64_t rows,
                                                           int64_t cols, void *__restrict__ yv, int64_t ldy, int vec_ok)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4)
        unpack_tile<BF16OUT>(packed, tile_at(packed_bytes, map, offsets, t), tiles_w, t, lane, rows, cols, yv, ldy, vec_ok != 0);
}

// The mirror image of pack_tiles_transposed_kernel: the stream of wᵀ → y in w's orientation (rows × cols, pitch ldy).  Nothing is stored
// outside rows × cols, nor for a tile whose blob is not there.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void unpack_tiles_transposed_kernel(const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                      const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets,
                                                                      int64_t tiles, int64_t tiles_w, int64_t rows, int64_t cols,
                                                                      void *__restrict__ yv, int64_t ldy)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4) {
        const int64_t c = (t / tiles_w) * kTile + (lane >> 1), r0 = (t % tiles_w) * kTile + kGroup * (lane & 1);
        GroupRaw g;
        load_group(packed, tile_at(packed_bytes, map, offsets, t), lane, g);
        if (g.f < 0 || c >= cols) continue;
        uint32_t y[kGroup];
        decode_group(g, y);
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            if (r0 + i >= rows) continue;
            if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[(r0 + i) * ldy + c] = (uint16_t)(y[i] >> 16);
            else static_cast<uint32_t *>(yv)[(r0 + i) * ldy + c] = y[i];
        }
    }
}

// The batch, as pack_tiles_batched_kernel numbers it: matrix i of y starts i * stride elements in.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void unpack_tiles_batched_kernel(const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                   const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets,
                                                                   const uint64_t *__restrict__ bases, int64_t count, int64_t tiles, int64_t tiles_w,
                                                                   int64_t rows, int64_t cols, void *__restrict__ yv, int64_t ldy, int64_t stride,
                                                                   int vec_ok)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = count * tiles;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < total; g += (int64_t)gridDim.x * 4) {
        const int64_t i = g / tiles, t = g - i * tiles;
        const TileAt a = tile_at(packed_bytes, maps + i * tiles, offsets + i * (tiles + 1), t, bases[i]);
        void *yi = BF16OUT ? static_cast<void *>(static_cast<uint16_t *>(yv) + i * stride) : static_cast<void *>(static_cast<uint32_t *>(yv) + i * stride);
        unpack_tile<BF16OUT>(packed, a, tiles_w, t, lane, rows, cols, yi, ldy, vec_ok != 0);
    }
}

// ---- the batched transposed pair: pack_tiles_transposed_kernel / unpack_tiles_transposed_kernel over a batch and its arena
//
// Pack's read path.  pack_tiles_transposed_kernel has every lane walk 16 rows of one column of w: 16 scalar loads per lane.  Here the wave
// first reads the tile's 32 × 32 region of w BY ROWS into an image of float32 words in LDS, 16 bytes per lane and load (a float32 row of
// the region is 8 lanes, a bf16 row 4: four / two loads per lane), and each lane then gathers its group down a column of the image.
// The 16-byte loads are taken when w, ld and stride keep every matrix 16-byte aligned (a region starts at a multiple of 32 columns) and
// the whole region lies inside rows × cols: a wave-uniform choice, so the loads of a tile are all in flight before the first store.
// Every other tile (a ragged edge, an unaligned view) is read element by element, +0 past an edge.
//
// Banks (stores and ds_read_b32: word address mod 32, by 32-lane halves).  The image's row pitch is 33 words, so word (r, c) is on
// bank (r + c) mod 32.  A store instruction writes word j of every lane's piece: a half holds 4 (float32) or 8 (bf16) consecutive rows and
// the pieces start 4 or 8 columns apart, r + c takes 32 distinct values.  A gather reads (16 (lane & 1) + i, lane >> 1): over a half
// 16 (lane & 1) + (lane >> 1) takes every value 0..31 once.  Neither side has a conflict.
//
// The image is one wave's (4224 bytes; 16.5 KB a workgroup): no __syncthreads.  Stores and reads are by different lanes, so the ordering
// is packed_matmul_skinny_kernel's: a workgroup-scope fence and a wave barrier between a tile's stores and its reads, a fence and a
// wave barrier after the reads before the next tile's stores.  Every branch around them is wave-uniform.
//
// MTQ_PACK_TRANSPOSED_BATCHED_DIRECT (a compile-time switch for A/B measurements) takes the per-tensor kernel's direct
// column reads instead; the group's words, and so the bytes, are the same.
constexpr int kImgPitch = kTile + 1;                 // words per image row
constexpr int kImgWords = kTile * kImgPitch;
#ifdef MTQ_PACK_TRANSPOSED_BATCHED_DIRECT
constexpr bool kPackTransposedStaged = false;
#else
constexpr bool kPackTransposedStaged = true;
#endif

// The region of w with its corner at (r0, c0) → img[32][kImgPitch] as float32 words, read by rows.  whole (wave-uniform): the region lies
// inside rows × cols and every row of it starts 16-byte aligned.
template <typename T>
__device__ __forceinline__ void stage_region(const T *__restrict__ w, int64_t rows, int64_t cols, int64_t ld, bool whole, int64_t r0, int64_t c0,
                                             int lane, uint32_t *__restrict__ img)
{
    constexpr int kPer = 16 / (int)sizeof(T);        // elements of a 16-byte piece: 4 float32, 8 bf16
    constexpr int kRowLanes = kTile / kPer;          // lanes to a row of the region: 8, 4
    constexpr int kPassRows = 64 / kRowLanes;        // rows to a load instruction: 8, 16
    constexpr int kPasses = kTile / kPassRows;       // 4, 2
    const int rl = lane / kRowLanes, cl = kPer * (lane % kRowLanes);
    const int64_t col = c0 + cl;
    uint32_t v[kPasses][kPer];
    if (whole) {
        uint4 q[kPasses];
#pragma unroll
        for (int p = 0; p < kPasses; ++p) q[p] = *reinterpret_cast<const uint4 *>(w + (r0 + p * kPassRows + rl) * ld + col);
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
            const uint32_t d[4] = {q[p].x, q[p].y, q[p].z, q[p].w};
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                if constexpr (sizeof(T) == 4) v[p][i] = d[i];
                else v[p][i] = (i & 1) ? (d[i >> 1] & 0xFFFF0000u) : (d[i >> 1] << 16);
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
            const int64_t row = r0 + p * kPassRows + rl;
#pragma unroll
            for (int i = 0; i < kPer; ++i) v[p][i] = (row < rows && col + i < cols) ? word_of(w, row * ld + col + i) : 0u;
        }
    }
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        uint32_t *dst = img + (p * kPassRows + rl) * kImgPitch + cl;
#pragma unroll
        for (int i = 0; i < kPer; ++i) dst[i] = v[p][i];
    }
}

// Wave g of count * tiles takes tile t = g % tiles of tensor i = g / tiles, as pack_tiles_batched_kernel; the grid (tiles, tiles_w) is the
// transpose's, as pack_tiles_transposed_kernel's.
template <typename T>
__global__ __launch_bounds__(256) void pack_tiles_transposed_batched_kernel(const T *__restrict__ w, int64_t count, int64_t rows, int64_t cols,
                                                                            int64_t ld, int64_t stride, int vec_ok, const int8_t *__restrict__ maps,
                                                                            const uint32_t *__restrict__ offsets, const uint64_t *__restrict__ bases,
                                                                            int64_t tiles, int64_t tiles_w, uint8_t *__restrict__ out, uint64_t out_bytes)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kPackTransposedStaged ? 4 * kImgWords : 4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *img = lds + (kPackTransposedStaged ? wave * kImgWords : 0);
    const int64_t total = count * tiles;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < total; g += (int64_t)gridDim.x * 4) {
        const int64_t i = g / tiles, t = g - i * tiles;
        const int f = maps[g];
        const uint32_t size = packed_tile_bytes(f);
        const uint64_t off = (bases[i] + offsets[i * (tiles + 1) + t]) * kUnit;
        if (size == 0u || off > out_bytes || size > out_bytes - off) continue;   // wave-uniform
        const T *wi = w + i * stride;
        const int64_t c0 = (t / tiles_w) * kTile, r0 = (t % tiles_w) * kTile;    // the region's corner in w
        const int cl = lane >> 1, rl = kGroup * (lane & 1);                      // the lane's group: column cl, rows rl .. rl + 15 of it
        uint32_t u[kGroup];
        if constexpr (kPackTransposedStaged) {
            stage_region(wi, rows, cols, ld, vec_ok != 0 && r0 + kTile <= rows && c0 + kTile <= cols, r0, c0, lane, img);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int j = 0; j < kGroup; ++j) u[j] = img[(rl + j) * kImgPitch + cl];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) u[j] = (c0 + cl < cols && r0 + rl + j < rows) ? word_of(wi, (r0 + rl + j) * ld + c0 + cl) : 0u;
        }
        pack_group(u, f, lane, out + off);
    }
}

// unpack_tiles_transposed_kernel's tile (its direct strided stores) for every (tensor, tile) of an arena: matrix i of y starts i * stride
// elements in.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void unpack_tiles_transposed_batched_kernel(const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                              const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets,
                                                                              const uint64_t *__restrict__ bases, int64_t count, int64_t tiles,
                                                                              int64_t tiles_w, int64_t rows, int64_t cols, void *__restrict__ yv,
                                                                              int64_t ldy, int64_t stride)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = count * tiles;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < total; g += (int64_t)gridDim.x * 4) {
        const int64_t i = g / tiles, t = g - i * tiles;
        const int64_t c = (t / tiles_w) * kTile + (lane >> 1), r0 = (t % tiles_w) * kTile + kGroup * (lane & 1);
        GroupRaw gr;
        load_group(packed, tile_at(packed_bytes, maps + i * tiles, offsets + i * (tiles + 1), t, bases[i]), lane, gr);
        if (gr.f < 0 || c >= cols) continue;
        uint32_t y[kGroup];
        decode_group(gr, y);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (r0 + j >= rows) continue;
            if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[i * stride + (r0 + j) * ldy + c] = (uint16_t)(y[j] >> 16);
            else static_cast<uint32_t *>(yv)[i * stride + (r0 + j) * ldy + c] = y[j];
        }
    }
}

// ---- batched offsets: the device counterpart of mtq_packed_offsets
// Exclusive prefix of v over the 256 threads of the workgroup (thread order) and the workgroup's total: a shuffle scan in each wave, the
// four wave totals through LDS.  lds: 4 words, free to reuse after the call.
template <typename U>
__device__ __forceinline__ U block_exclusive_scan(U v, U *lds, U &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    U incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const U up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();                                  // the previous use of lds is over
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    U before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const U s = lds[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + incl - v;
}

// One workgroup per tensor: thread k sums the units of tiles [k * per, (k + 1) * per), the workgroup scans the 256 sums, and a second
// pass over the same run writes the offsets.  A code outside 0..3 counts 0 units and 1 in bad[i].  tiles * 32 fits 32 bits (the entry
// checks it), so no sum wraps.
__global__ __launch_bounds__(256) void packed_offsets_batched_kernel(const int8_t *__restrict__ maps, int64_t count, int64_t tiles,
                                                                     uint32_t *__restrict__ offsets, int32_t *__restrict__ bad)
{
    __shared__ uint32_t lds[4];
    const int64_t per = (tiles + 255) / 256;
    const int64_t t0 = std::min<int64_t>((int64_t)threadIdx.x * per, tiles), t1 = std::min<int64_t>(t0 + per, tiles);
    for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int8_t *map = maps + i * tiles;
        uint32_t *off = offsets + i * (tiles + 1);
        uint32_t sum = 0u, nbad = 0u;
        for (int64_t t = t0; t < t1; ++t) {
            const uint32_t size = packed_tile_bytes(map[t]);
            sum += size / kUnit;
            nbad += size == 0u;
        }
        uint32_t total, total_bad;
        uint32_t run = block_exclusive_scan(sum, lds, total);
        block_exclusive_scan(nbad, lds, total_bad);
        for (int64_t t = t0; t < t1; ++t) {
            off[t] = run;
            run += packed_tile_bytes(map[t]) / kUnit;
        }
        if (threadIdx.x == 0) {
            off[tiles] = total;
            bad[i] = (int32_t)total_bad;
        }
    }
}

// bases[0 .. count]: the exclusive prefix sum of the tensors' totals offsets[i][tiles], by one workgroup (behind the kernel above on the
// same stream).
__global__ __launch_bounds__(256) void packed_bases_kernel(const uint32_t *__restrict__ offsets, int64_t count, int64_t tiles,
                                                           uint64_t *__restrict__ bases)
{
    __shared__ unsigned long long lds[4];
    const int64_t per = (count + 255) / 256;
    const int64_t i0 = std::min<int64_t>((int64_t)threadIdx.x * per, count), i1 = std::min<int64_t>(i0 + per, count);
    unsigned long long sum = 0ull;
    for (int64_t i = i0; i < i1; ++i) sum += offsets[i * (tiles + 1) + tiles];
    unsigned long long total;
    unsigned long long run = block_exclusive_scan(sum, lds, total);
    for (int64_t i = i0; i < i1; ++i) {
        bases[i] = run;
        run += offsets[i * (tiles + 1) + tiles];
    }
    if (threadIdx.x == 0) bases[count] = total;
}

// ---- linear
constexpr int kBM = 128, kBN = 64, kBK = 64, kThreads = 256;
constexpr int kLdk = kBK + 8;                      // LDS row pitch in bf16, as mtq_output_error.hip

// float32 → bf16, round to nearest even; NaN stays NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + (0x7FFFu + ((u >> 16) & 1u))) >> 16);
}

template <bool BF16OUT>
__global__ __launch_bounds__(kThreads) void packed_linear_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec,
                                                                 const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                 const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets, int64_t N,
                                                                 int64_t tiles_h, int64_t tiles_w, const float *__restrict__ bias,
                                                                 void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[(kBM + kBN) * kLdk];
    uint16_t *xs = lds;
    uint16_t *ws = lds + kBM * kLdk;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nblocks = (N + kBN - 1) / kBN;
    const int64_t bm = blockIdx.x / nblocks, bn = blockIdx.x % nblocks;
    const int64_t m0 = bm * kBM, n0 = bn * kBN;

    f32x16 acc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;

    // lane tid owns the group (row n0 + tid / 4, columns k0 + 16 (tid % 4) ..) of the W block: group 2 (n % 32) + half of tile (n / 32, k / 32)
    const int wrow = tid >> 2, wc16 = (tid & 3) * kGroup;
    const int64_t wtr = (n0 + wrow) >> 5;
    const int wgi = 2 * (int)((n0 + wrow) & 31) + ((tid & 3) & 1);
    uint4 xr[4];
    GroupRaw wr;
    TileAt at;                                       // of the step after the one in xr / wr: map and offsets run two steps ahead of the MFMAs
    auto locate = [&](int64_t k0) {
        const int64_t wtc = (k0 + wc16) >> 5;
        at.off = 0;
        at.f = -1;
        if (wtr < tiles_h && wtc < tiles_w) at = tile_at(packed_bytes, map, offsets, wtr * tiles_w + wtc);
    };
    auto load_step = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // X: 128 rows × 64 columns = 1024 pieces of 8 bf16, 4 per thread; columns past K are zeros, never read
            const int p = tid + kThreads * i, row = p >> 3, c8 = (p & 7) * 8;
            const int64_t gm = m0 + row, gk = k0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < M && gk < K) {
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
        load_group(packed, at, wgi, wr);             // the blob `at` names: located one step earlier
        locate(k0 + kBK);
    };
    locate(0);
    load_step(0);
    for (int64_t k0 = 0; k0 < K; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + kThreads * i;
            *reinterpret_cast<uint4 *>(xs + (p >> 3) * kLdk + (p & 7) * 8) = xr[i];
        }
        {
            uint32_t y[kGroup];
            decode_group(wr, y);
            uint4 lo, hi;
            pack_halves(y, lo, hi);
            uint4 *d = reinterpret_cast<uint4 *>(ws + wrow * kLdk + wc16);
            d[0] = lo;
            d[1] = hi;
        }
        __syncthreads();
        if (k0 + kBK < K) load_step(k0 + kBK);
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) {
            const int koff = kk * 16 + 8 * (lane >> 5);
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xs + (wave * 32 + (lane & 31)) * kLdk + koff);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 b = *reinterpret_cast<const bf16x8 *>(ws + (s * 32 + (lane & 31)) * kLdk + koff);
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: lane's outputs are (m0 + 32·wave + (r&3) + 8(r>>2) + 4(lane>>5), n0 + 32s + (lane&31))
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t n = n0 + 32 * s + (lane & 31);
        if (n >= N) continue;
        const float b = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= M) continue;
            const float v = acc[s][r] + b;
            if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[m * ldy + n] = f32_to_bf16(v);
            else static_cast<float *>(yv)[m * ldy + n] = v;
        }
    }
}

// ---- matmul: Y = X·P̂ + b for a packed k × n matrix P̂ (a group's 16 values run along n at one k)
//
// packed_linear_kernel's frame: the same block, K step, X staging, one-step-ahead fetch, MFMA sequence and epilogue.  The W side differs:
// lane tid owns the group at k-row k0 + tid / 4, columns n0 + 16 (tid % 4) .., and stores its 16 decoded bf16 as they lie (n-contiguous)
// into a [k][n] image; the B operand (8 consecutive k at one n per lane) comes out of that image through the transposed LDS read, two
// per operand (k +0..3, then +4..7).  Operand positions are the block kernel's - the same k at the same lane half and element, the same
// kk order - so the sums are the block kernel's on the transposed weight, bit for bit.
//
// The image: one sub-image per 32-column slot s, [64 k][32 n] bf16 with a 64-byte row pitch, sub-image 1 a further 16 bytes on.  A
// transposed read's 32-lane half takes 4 k-rows × 32 columns: byte q * 64 + 32 (g & 1) + 8 p for row q, group g, quarter p - 256
// consecutive bytes, every one of the 64 banks once: conflict-free by the bank rule ((a / 4) % 64).  A plain [64][64 (+ 8)] image would
// put rows q and q + 2 (128-byte pitch) or q + 2 less 8 banks (144-byte pitch) on the same banks: 2-way.  The 16 bytes between the
// sub-images keep the 16-byte stores of an 8-lane group (4 lanes to each sub-image, 128 consecutive bytes each) on disjoint banks
// ((a / 4) % 32): 0-3, 8-11, .. for s = 0 and 4-7, 12-15, .. for s = 1.
//
// The transposed read needs EXEC all ones: the kernel has no early return and the reads sit in no lane-dependent branch.  Tiles that are
// absent (past the grid, a bad code, a blob past packed_bytes) and k-rows at or past K are zeros in the image.
constexpr int kMmPitch = 32;                         // bf16 per image row: 64 bytes
constexpr int kMmSub = kBK * kMmPitch + 8;           // bf16 from sub-image 0 to sub-image 1: the rows and 16 bytes

typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ i16x4 lds_read_tr16(const uint16_t *p)
{
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4 *)(p));
}

template <bool BF16OUT>
__global__ __launch_bounds__(kThreads) void packed_matmul_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec,
                                                                 const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                 const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets, int64_t N,
                                                                 int64_t tiles_h, int64_t tiles_w, const float *__restrict__ bias,
                                                                 void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kBM * kLdk + 2 * kMmSub];
    uint16_t *xs = lds;
    uint16_t *ws = lds + kBM * kLdk;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nblocks = (N + kBN - 1) / kBN;
    const int64_t bm = blockIdx.x / nblocks, bn = blockIdx.x % nblocks;
    const int64_t m0 = bm * kBM, n0 = bn * kBN;

    f32x16 acc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;

    // lane tid owns the group (k-row k0 + tid / 4, columns n0 + 16 (tid % 4) ..): group 2 (k % 32) + half of tile (k / 32, n / 32)
    const int wrow = tid >> 2, wq = tid & 3;
    const int64_t wtc = (n0 + wq * kGroup) >> 5;
    const int wgi = 2 * (wrow & 31) + (wq & 1);      // k0 is a multiple of 64: (k0 + wrow) % 32 is wrow % 32
    uint16_t *wdst = ws + (wq >> 1) * kMmSub + wrow * kMmPitch + (wq & 1) * kGroup;
    // the transposed read of lane 16 g + 4 q + p: row 8 (lane >> 5) + q of the kk block, columns 16 (g & 1) + 4 p .. of the slot
    const uint16_t *wsrc = ws + (8 * (lane >> 5) + ((lane >> 2) & 3)) * kMmPitch + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    uint4 xr[4];
    GroupRaw wr;
    TileAt at;                                       // of the step after the one in xr / wr: map and offsets run two steps ahead of the MFMAs
    auto locate = [&](int64_t k0) {
        const int64_t wtr = (k0 + wrow) >> 5;
        at.off = 0;
        at.f = -1;
        if (k0 + wrow < K && wtc < tiles_w) at = tile_at(packed_bytes, map, offsets, wtr * tiles_w + wtc);
    };
    auto load_step = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // X: 128 rows × 64 columns = 1024 pieces of 8 bf16, 4 per thread; columns past K are zeros, never read
            const int p = tid + kThreads * i, row = p >> 3, c8 = (p & 7) * 8;
            const int64_t gm = m0 + row, gk = k0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < M && gk < K) {
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
        load_group(packed, at, wgi, wr);             // the blob `at` names: located one step earlier
        locate(k0 + kBK);
    };
    locate(0);
    load_step(0);
    for (int64_t k0 = 0; k0 < K; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + kThreads * i;
            *reinterpret_cast<uint4 *>(xs + (p >> 3) * kLdk + (p & 7) * 8) = xr[i];
        }
        {
            uint32_t y[kGroup];
            decode_group(wr, y);
            uint4 lo, hi;
            pack_halves(y, lo, hi);
            uint4 *d = reinterpret_cast<uint4 *>(wdst);
            d[0] = lo;
            d[1] = hi;
        }
        __syncthreads();
        if (k0 + kBK < K) load_step(k0 + kBK);
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) {
            const int koff = kk * 16 + 8 * (lane >> 5);
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xs + (wave * 32 + (lane & 31)) * kLdk + koff);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const uint16_t *src = wsrc + s * kMmSub + kk * 16 * kMmPitch;
                const i16x4 b0 = lds_read_tr16(src), b1 = lds_read_tr16(src + 4 * kMmPitch);   // k + 0..3, k + 4..7
                const i16x8 b = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, b), acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: lane's outputs are (m0 + 32·wave + (r&3) + 8(r>>2) + 4(lane>>5), n0 + 32s + (lane&31))
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t n = n0 + 32 * s + (lane & 31);
        if (n >= N) continue;
        const float b = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= M) continue;
            const float v = acc[s][r] + b;
            if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[m * ldy + n] = f32_to_bf16(v);
            else static_cast<float *>(yv)[m * ldy + n] = v;
        }
    }
}

// ---- skinny linear (m <= 32): one wave per (K slice, tile row) unit, W straight to registers, no LDS.
//
// A unit is the run of tiles [c0, c1) of tile row tr: one contiguous byte range of the stream.  Lane l owns group (row l & 31, half
// l >> 5) of every tile of the run, i.e. 16 consecutive K positions of one output feature.  mfma_f32_32x32x16_bf16 takes eight K values
// per lane and sums over whatever K positions the two operands agree on, so the lane's 16 decoded values feed two MFMAs (values 0..7,
// then 8..15) and the X operand of lane l is row l & 31 of X at the same sixteen positions 32 tc + 16 (l >> 5) + 0..15.  Rows of X at or
// past m and positions at or past k are zeros that are never read.  The map and offsets of up to 64 tiles of the run are fetched with one
// load (a lane each) and handed out with readlane; the loads of kSkinnyRing tiles (W and X) are issued before the first is decoded.
// split > 1: the unit's 32 × m partial goes to ws[slice][m][n] as f32 and skinny_reduce_kernel sums the slices in ascending order.
constexpr int kSkinnyRing = 8;                       // tiles in flight per wave: 9 VGPRs of W and 8 of X each
constexpr int kSkinnyWaves = 4;                      // units per workgroup; the waves share nothing

typedef float f32x2 __attribute__((ext_vector_type(2)));

// decode_as for a group whose exponent byte E is in [M, 254], in a third of the instructions.  bfp_code_bits_rt's word is the float
// ±man · 2^(E − 126 − M) (man = 2^msb · 1.frac, exponent field E − (M − 1 − msb) >= 1: normal), so it is the integer mantissa converted
// to float (exact) times the power of two with exponent field E − M + 1 >= 1 (exact: no rounding, no underflow, and the product's
// field is at most E <= 254), the code's sign bit moved into the factor.  man == 0 gives ±0, and fma(±0, s, +0) is +0 under round to
// nearest: the word 0 that bfp_code_bits_rt returns for man == 0 whatever the sign bit.  Below M the exponent wraps and at 255 the word
// is an Inf / NaN pattern that a product does not form: decode_skinny sends those groups to decode_as.
// tests/test_packed_skinny_gpu.py compares the two for every (exponent byte, code, position) on the device.
template <int F>
__device__ __forceinline__ void decode_scaled(const GroupRaw &g, uint32_t (&y)[kGroup])
{
    constexpr uint32_t M = F == 1 ? 7u : (F == 2 ? 3u : 1u);
    constexpr uint32_t B = M + 1u;
    const uint32_t scale = (g.E - (M - 1u)) << 23;
    float mf[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        if constexpr (F == 1) {                      // a byte of the word with the sign bits masked off: one cvt_f32_ubyte each
            mf[i] = (float)(((g.w[i >> 2] & 0x7F7F7F7Fu) >> (8 * (i & 3))) & 0xFFu);
        } else if constexpr (F == 2) {               // even nibbles and odd nibbles spread to bytes first
            const uint32_t word = g.w[i >> 3], src = (i & 1) ? ((word >> 4) & 0x07070707u) : (word & 0x07070707u);
            mf[i] = (float)((src >> (8 * ((i & 7) >> 1))) & 0xFFu);
        } else {
            mf[i] = (float)((g.w[0] >> (2 * i)) & 1u);
        }
    }
#pragma unroll
    for (int i = 0; i < kGroup; i += 2) {
        f32x2 a, s;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t pos = (((i + j) * B) & 31u) + M;              // the sign bit of code i + j in its word
            const uint32_t t = g.w[((i + j) * B) >> 5] << (31u - pos);
            a[j] = mf[i + j];
            s[j] = __uint_as_float((t & 0x80000000u) | scale);
        }
        const f32x2 zero = {0.0f, 0.0f};
        const f32x2 r = __builtin_elementwise_fma(a, s, zero);
        y[i] = __float_as_uint(r[0]);
        y[i + 1] = __float_as_uint(r[1]);
    }
}

template <int F>
__device__ __forceinline__ void decode_either(const GroupRaw &g, uint32_t (&y)[kGroup])
{
    constexpr uint32_t M = F == 1 ? 7u : (F == 2 ? 3u : 1u);
    if (g.E >= M && g.E <= 254u) decode_scaled<F>(g, y);
    else decode_as<F>(g, y);
}

// decode_group's words exactly
__device__ __forceinline__ void decode_skinny(const GroupRaw &g, uint32_t (&y)[kGroup])
{
    if (g.f == 1) decode_either<1>(g, y);
    else if (g.f == 2) decode_either<2>(g, y);
    else if (g.f == 3) decode_either<3>(g, y);
    else decode_group(g, y);
}

// The probe of decode_skinny: thread (rot, E, q) decodes the group with exponent byte E whose element i holds code
// (16 q + (i + rot) % 16) mod 2^B, and writes its words beside bfp_code_bits_rt's: 16 × 256 × 16 groups cover every (E, code) at every
// position of the group.  got, want: uint32 [16][256][16][16].
constexpr int kProbeGroups = 16 * 256 * 16;

__global__ __launch_bounds__(256) void packed_decode_probe_kernel(int f, uint32_t *__restrict__ got, uint32_t *__restrict__ want)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kProbeGroups) return;
    const uint32_t rot = idx >> 12, E = (idx >> 4) & 255u, q = idx & 15u;
    const uint32_t M = f == 1 ? 7u : (f == 2 ? 3u : 1u), B = M + 1u;
    GroupRaw g;
#pragma unroll
    for (int i = 0; i < 8; ++i) g.w[i] = 0u;
    g.E = E;
    g.f = f;
    uint32_t code[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        code[i] = (16u * q + ((i + rot) & 15u)) & ((1u << B) - 1u);
        if (f == 1) g.w[i >> 2] |= code[i] << (8 * (i & 3));
        else if (f == 2) g.w[i >> 3] |= code[i] << (4 * (i & 7));
        else g.w[0] |= code[i] << (2 * i);
    }
    uint32_t y[kGroup];
    decode_skinny(g, y);
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        got[(int64_t)idx * kGroup + i] = y[i];
        want[(int64_t)idx * kGroup + i] = bfp_code_bits_rt(code[i], E, M);
    }
}

__device__ __forceinline__ void load_x16(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec, int row, int64_t k0,
                                         uint4 &lo, uint4 &hi)
{
    lo = make_uint4(0u, 0u, 0u, 0u);
    hi = lo;
    if (row >= M || k0 >= K) return;
    const uint16_t *src = x + (int64_t)row * ldx + k0;
    if (x_vec && k0 + kGroup <= K) {
        lo = reinterpret_cast<const uint4 *>(src)[0];
        hi = reinterpret_cast<const uint4 *>(src)[1];
    } else {
        uint32_t h[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) h[j] = k0 + j < K ? (uint32_t)src[j] : 0u;
        lo = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        hi = make_uint4(h[8] | (h[9] << 16), h[10] | (h[11] << 16), h[12] | (h[13] << 16), h[14] | (h[15] << 16));
    }
}

__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 &v) { return __builtin_bit_cast(bf16x8, v); }

template <bool BF16OUT>
__device__ __forceinline__ void store_y(void *__restrict__ yv, int64_t at, float v)
{
    if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[at] = f32_to_bf16(v);
    else static_cast<float *>(yv)[at] = v;
}

// One tensor's stream as the wave that reads it holds it, for every kernel below: a single tensor, or one expert of an arena
// (pack_tiles_batched's tables).
struct PackedStream {
    const uint8_t *packed;                           // the tensor's stream, or the arena
    const int8_t *map;                               // the tensor's (the expert's) tables
    const uint32_t *off;
    uint64_t base, limit;                            // units: the blobs of this tensor lie in [base, limit)
};

__device__ __forceinline__ PackedStream tensor_stream(const uint8_t *packed, uint64_t packed_bytes, const int8_t *map, const uint32_t *offsets)
{
    return {packed, map, offsets, 0, packed_bytes / kUnit};
}

__device__ __forceinline__ PackedStream arena_stream(const uint8_t *packed, uint64_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                     const uint64_t *bases, int64_t e, int64_t tiles)
{
    return {packed, maps + e * tiles, offsets + e * (tiles + 1), bases[e], std::min<uint64_t>(bases[e + 1], packed_bytes / kUnit)};
}

// tile_at's answer for a tile of code f at unit o of the stream, the guard made in units against [base, limit).  For a single tensor
// (base = 0, limit = packed_bytes / 64) this is tile_at's byte guard: every offset and every blob size is a multiple of 64, so
// 64 o + size > packed_bytes exactly when o + size / 64 > packed_bytes / 64.
__device__ __forceinline__ TileAt stream_at(const PackedStream &st, int f, uint32_t o)
{
    TileAt a;
    const uint32_t size = packed_tile_bytes(f);
    const uint64_t pos = st.base + o;                // base <= limit < 2^58 where it counts
    a.off = pos * kUnit;
    a.f = (size == 0u || st.base > st.limit || pos + size / kUnit > st.limit) ? -1 : f;
    return a;
}

// What a skinny wave does with a decoded group: W (n, k) feeds it to the MFMAs as the B operand as it is.
struct FeedDirect {
    static constexpr bool kGroupIsKRow = false;
    __device__ __forceinline__ void operator()(int, const uint4 &xl, const uint4 &xh, const uint4 &lo, const uint4 &hi, f32x16 &acc) const
    {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(xl), as_bf16x8(lo), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(xh), as_bf16x8(hi), acc, 0, 0, 0);
    }
};

// A skinny wave's run: tiles t0 + c * tstep, c in [c0, c1), of one stream into one accumulator, X rows [0, M) at the K positions 32 c ...
// The map codes and offsets of up to 64 tiles of the run are fetched with one load (a lane each) and handed out with readlane; the loads
// of kSkinnyRing tiles (group gi of W, and X) are issued before the first is decoded; a blob is checked wave-uniformly (stream_at) before
// it is touched; decode_skinny, then `feed` (two MFMAs per tile, ascending K).  `lane` hands out, (row, half, gi) address: the grouped
// kernel forms the latter anew per chunk.  Feed::kGroupIsKRow: group gi is k-row gi / 2 of its tile, zeros at or past K.
template <typename Feed>
__device__ __forceinline__ void skinny_run(f32x16 &acc, const Feed &feed, const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx,
                                           int x_vec, const PackedStream &st, int64_t t0, int64_t tstep, int64_t c0, int64_t c1, int lane, int row,
                                           int half, int gi)
{
    const uint8_t *__restrict__ packed = st.packed;
    const int8_t *__restrict__ map = st.map;
    const uint32_t *__restrict__ off = st.off;
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int cnt = (int)std::min<int64_t>(64, c1 - cb);
        int mf = -1, mo = 0;                         // lane i: map code and offset of tile cb + i of the run
        if (lane < cnt) {
            const int64_t t = t0 + (cb + lane) * tstep;
            mf = map[t];
            mo = (int)off[t];
        }
        for (int b = 0; b < cnt; b += kSkinnyRing) {
            GroupRaw g[kSkinnyRing];
            uint4 xl[kSkinnyRing], xh[kSkinnyRing];
#pragma unroll
            for (int j = 0; j < kSkinnyRing; ++j) {
                const int i = b + j;                 // uniform
                TileAt a;
                a.off = 0;
                a.f = -1;
                xl[j] = make_uint4(0u, 0u, 0u, 0u);
                xh[j] = xl[j];
                if (i < cnt) {
                    a = stream_at(st, __builtin_amdgcn_readlane(mf, i), (uint32_t)__builtin_amdgcn_readlane(mo, i));
                    if constexpr (Feed::kGroupIsKRow) {
                        if ((cb + i) * kTile + (gi >> 1) >= K) a.f = -1;   // this lane's k-row
                    }
                    load_x16(x, M, K, ldx, x_vec, row, (cb + i) * kTile + kGroup * half, xl[j], xh[j]);
                }
                load_group(packed, a, gi, g[j]);
            }
#pragma unroll
            for (int j = 0; j < kSkinnyRing; ++j) {
                if (b + j < cnt) {
                    uint32_t y[kGroup];
                    decode_skinny(g[j], y);
                    uint4 lo, hi;
                    pack_halves(y, lo, hi);
                    feed(j, xl[j], xh[j], lo, hi, acc);
                }
            }
        }
    }
}

// A skinny lane's 16 accumulators are rows mu + 4 half, mu = (r&3) + 8(r>>2), of one column of a 32-row chunk: those below M go to
// dst[at + mu * ld], `at` the lane's own part of the address, so that what varies with r is uniform.  PARTIAL: dst is an f32 workspace
// slice and takes the sums as they are; otherwise dst is Y and takes them with the bias.
template <bool BF16OUT, bool PARTIAL>
__device__ __forceinline__ void store_lane_rows(const f32x16 &acc, int64_t M, int half, void *__restrict__ dst, int64_t at, int64_t ld, float bv)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mu = (r & 3) + 8 * (r >> 2);
        if (mu + 4 * half >= M) continue;
        if constexpr (PARTIAL) static_cast<float *>(dst)[at + mu * ld] = acc[r];
        else store_y<BF16OUT>(dst, at + mu * ld, acc[r] + bv);
    }
}

// split == 1: rows row0 .. of Y with the bias value bv; otherwise rows row0 .. of slice s of ws [split][T][N]
template <bool BF16OUT>
__device__ __forceinline__ void store_skinny(const f32x16 &acc, int64_t M, int half, int64_t row0, int64_t n, int split, float bv,
                                             void *__restrict__ yv, int64_t ldy, float *__restrict__ ws, int64_t s, int64_t T, int64_t N)
{
    const int64_t mh = row0 + 4 * half;
    if (split == 1) store_lane_rows<BF16OUT, false>(acc, M, half, yv, mh * ldy + n, ldy, bv);
    else store_lane_rows<false, true>(acc, M, half, ws, (s * T + mh) * N + n, N, 0.0f);
}

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    return acc;
}

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves) void packed_linear_skinny_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx,
                                                                                  int x_vec, const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                                  const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets,
                                                                                  int64_t N, int64_t tiles_h, int64_t tiles_w, int split,
                                                                                  const float *__restrict__ bias, void *__restrict__ yv, int64_t ldy,
                                                                                  float *__restrict__ ws)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= tiles_h * split) return;             // wave-uniform; the kernel has no barrier
    const int64_t s = unit / tiles_h, tr = unit % tiles_h;   // the waves of a workgroup share a slice of X
    const int row = lane & 31, half = lane >> 5;

    f32x16 acc = zero16();
    skinny_run(acc, FeedDirect(), x, M, K, ldx, x_vec, tensor_stream(packed, packed_bytes, map, offsets), tr * tiles_w, 1, s * tiles_w / split,
               (s + 1) * tiles_w / split, lane, row, half, 2 * row + half);

    // lane's outputs are (m = (r&3) + 8(r>>2) + 4·half, n = 32·tr + row)
    const int64_t n = tr * kTile + row;
    if (n >= N) return;
    store_skinny<BF16OUT>(acc, M, half, 0, n, split, split == 1 && bias ? bias[n] : 0.0f, yv, ldy, ws, s, M, N);
}

// Y[m][n] = ((p0 + p1) + ... + p_{split-1}) + b: ascending slices from slice 0, the bias last, one rounding for a bf16 Y.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float *__restrict__ ws, int64_t MN, int64_t N, int split,
                                                            const float *__restrict__ bias, void *__restrict__ yv, int64_t ldy)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= MN) return;
    const int64_t m = idx / N, n = idx % N;
    float v = ws[idx];
    for (int s = 1; s < split; ++s) v += ws[(int64_t)s * MN + idx];
    v += bias ? bias[n] : 0.0f;
    store_y<BF16OUT>(yv, m * ldy + n, v);
}

// The library's split for (m, n, k): a pure function of the shape.  Units (tile rows × slices) fill at most kSkinnyUnits waves, what the
// chip holds at once (256 CUs × 8: one unit over that and a second round of waves starts), and a slice keeps at least kSkinnyMinRun tiles
// (DESIGN.md §A.6h has the measurement behind both).
constexpr int64_t kSkinnyUnits = 2048, kSkinnyMinRun = 4;

int tile_grid(int64_t rows, int64_t cols, int64_t *tiles_h, int64_t *tiles_w);

int skinny_split(int64_t m, int64_t tiles_h, int64_t tiles_w)
{
    (void)m;
    const int64_t by_units = kSkinnyUnits / tiles_h, by_run = tiles_w / kSkinnyMinRun;
    return (int)std::max<int64_t>(1, std::min(by_units, by_run));
}

// MTQ_OK and the effective split, or the refusal every skinny entry shares
int skinny_shape(int64_t m, int64_t n, int64_t k, int split, int64_t *tiles_h, int64_t *tiles_w, int *split_eff)
{
    if (m <= 0) return fail(MTQ_ERR_INVALID, "m must be positive (empty operands are handled by the caller)");
    if (m > MTQ_PACKED_SKINNY_MAX_M) return fail(MTQ_ERR_INVALID, "m > 32: the skinny kernel takes at most MTQ_PACKED_SKINNY_MAX_M rows");
    if (split < 0) return fail(MTQ_ERR_INVALID, "split must not be negative (0: the library's choice)");
    if (int rc = tile_grid(n, k, tiles_h, tiles_w)) return rc;
    *split_eff = (int)std::min<int64_t>(split == 0 ? skinny_split(m, *tiles_h, *tiles_w) : split, *tiles_w);
    return MTQ_OK;
}

size_t skinny_workspace(int64_t m, int64_t n, int split_eff)
{
    return split_eff <= 1 ? 0 : (((size_t)split_eff * (size_t)m * (size_t)n * sizeof(float) + 15) & ~(size_t)15);
}

// ---- skinny matmul (m <= 32): Y = X·P̂ + b for a packed k × n P̂, one wave per (K slice s, tile column tc) unit.
//
// packed_linear_skinny_kernel with the weight the other way round: the wave covers 32 output columns over the tile rows
// [s tiles_kh / split, (s + 1) tiles_kh / split) of P̂'s grid tiles_kh × tiles_nw, unit = s tiles_nw + tc, so the four waves of a workgroup
// read four neighbouring blobs of each tile row and share a slice of X.  The hand-out, the ring, the blob check and the decode are the
// linear kernel's; the tiles of a run are tiles_nw apart, so the one load of up to 64 map codes and offsets is a strided gather.
//
// A group's 16 values run along n at one k-row, an MFMA operand wants 8 consecutive k at one n: lane l decodes group l of the tile
// (k-row l >> 1, columns 16 (l & 1) ..) and stores its 16 bf16 as they lie at bytes 32 l .. 32 l + 31 of a wave-private [32 k][32 n] image
// with 64-byte rows, in two 16-byte pieces; the two B operands of the tile come out of the image through the transposed LDS read, two
// reads per operand: lane 16 g + 4 q + p supplies row r0 + q, columns 16 (g & 1) + 4 p .., and gets column lane & 31, rows r0 .. r0 + 3.
// MFMA 1 takes k-rows 16 (lane >> 5) + 0..7 of the tile and MFMA 2 rows 16 (lane >> 5) + 8..15, element j at position j, X as in the
// linear kernel (row lane & 31, positions 32 tile_row + 16 (lane >> 5) + 0..15): the linear kernel's operands on the transposed weight,
// in its tile order, over its slices, so its bits at the same split.
//
// Banks: a 32-lane half of a transposed read takes 4 k-rows × 64 bytes, 256 consecutive bytes, every one of the 64 banks once.  The
// 16-byte stores go by 8-lane groups over 32 banks; bytes 32 l of eight lanes would put lanes i and i + 4 on the same banks, so lanes
// with (l >> 2) & 1 set store their upper piece first: an 8-lane group then covers 32 distinct banks with each of its two stores.
//
// The transposed read needs EXEC all ones: the only early exit is the wave-uniform return below (the wave index is made scalar, so every
// branch on the run's length is a scalar branch), and the reads sit in no lane-dependent branch.  Tiles with a bad code or a blob past
// packed_bytes and k-rows at or past K are zeros in the image (pad, don't mask); columns at or past N are never stored.
//
// The image is one wave's: no __syncthreads.  Stores and reads are by different lanes, so a workgroup-scope fence (an s_waitcnt on the
// LDS counter) and a wave barrier stand between a tile's stores and its reads, and a fence and a wave barrier after the reads keep the
// next stores into that image behind them.  Two images per wave (4 KB; 16 KB a workgroup) alternate by tile.
constexpr int kMmsImage = kTile * kMmPitch;          // bf16 per image: [32 k][32 n]

// W (k, n): the group goes through the wave's image `j & 1` and comes back as two B operands by the transposed read.
struct FeedTransposed {
    static constexpr bool kGroupIsKRow = true;
    uint16_t *st;                                    // where this lane stores its group, in image 0
    const uint16_t *rd;                              // where its transposed reads start, in image 0
    int up;                                          // this lane stores its upper 16 bytes first
    __device__ __forceinline__ void operator()(int j, const uint4 &xl, const uint4 &xh, const uint4 &lo, const uint4 &hi, f32x16 &acc) const
    {
        uint16_t *dst = st + (j & 1) * kMmsImage;
        *reinterpret_cast<uint4 *>(dst + 8 * up) = make_uint4(up ? hi.x : lo.x, up ? hi.y : lo.y, up ? hi.z : lo.z, up ? hi.w : lo.w);
        *reinterpret_cast<uint4 *>(dst + 8 * (up ^ 1)) = make_uint4(up ? lo.x : hi.x, up ? lo.y : hi.y, up ? lo.z : hi.z, up ? lo.w : hi.w);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint16_t *src = rd + (j & 1) * kMmsImage;
        const i16x4 b0 = lds_read_tr16(src), b1 = lds_read_tr16(src + 4 * kMmPitch);         // k + 0..3, k + 4..7
        const i16x4 b2 = lds_read_tr16(src + 8 * kMmPitch), b3 = lds_read_tr16(src + 12 * kMmPitch);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const i16x8 blo = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
        const i16x8 bhi = __builtin_shufflevector(b2, b3, 0, 1, 2, 3, 4, 5, 6, 7);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(xl), __builtin_bit_cast(bf16x8, blo), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(xh), __builtin_bit_cast(bf16x8, bhi), acc, 0, 0, 0);
    }
};

// the lane's part of a FeedTransposed in the wave's pair of images
__device__ __forceinline__ FeedTransposed feed_transposed(uint16_t *img, int lane)
{
    FeedTransposed feed;
    feed.st = img + lane * kGroup;
    feed.rd = img + (kGroup * (lane >> 5) + ((lane >> 2) & 3)) * kMmPitch + kGroup * ((lane >> 4) & 1) + 4 * (lane & 3);
    feed.up = (lane >> 2) & 1;
    return feed;
}

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves) void packed_matmul_skinny_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx,
                                                                                  int x_vec, const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                                                  const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets,
                                                                                  int64_t N, int64_t tiles_kh, int64_t tiles_nw, int split,
                                                                                  const float *__restrict__ bias, void *__restrict__ yv, int64_t ldy,
                                                                                  float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= tiles_nw * split) return;            // wave-uniform; the kernel has no workgroup barrier
    const int64_t s = unit / tiles_nw, tc = unit % tiles_nw;   // the waves of a workgroup share a slice of X
    const int row = lane & 31, half = lane >> 5;

    const FeedTransposed feed = feed_transposed(lds + wave * (2 * kMmsImage), lane);

    // the run is tile column tc over the slice's tile rows: tiles tiles_nw apart (a strided gather of the tables), group `lane`
    f32x16 acc = zero16();
    skinny_run(acc, feed, x, M, K, ldx, x_vec, tensor_stream(packed, packed_bytes, map, offsets), tc, tiles_nw, s * tiles_kh / split,
               (s + 1) * tiles_kh / split, lane, row, half, lane);

    // lane's outputs are (m = (r&3) + 8(r>>2) + 4·half, n = 32·tc + row)
    const int64_t n = tc * kTile + row;
    if (n >= N) return;
    store_skinny<BF16OUT>(acc, M, half, 0, n, split, split == 1 && bias ? bias[n] : 0.0f, yv, ldy, ws, s, M, N);
}

// ---- grouped skinny linear: the experts of one arena (pack_tiles_batched's tables), each over its own rows of X, in one launch.
//
// A unit is (slice s, group e, tile row tr), numbered ((s * count + e) * tiles_h + tr): the four waves of a workgroup share a slice of X
// and, but for a seam, an expert.  Group e owns rows [group_rows[e], group_rows[e + 1]) of X and Y, clamped into [0, T] before any use; a
// group without rows returns before its first load.  The wave walks its rows in chunks of 32 and does on each chunk exactly what
// packed_linear_skinny_kernel does for an m <= 32 call on that chunk and that expert at the same split: the same readlane hand-out, ring,
// decode and two MFMAs per tile in ascending K, so the bits are those of that call.  W is read again for every chunk: the entry is for
// decode-sized groups, and mtq_packed_linear per expert stays the route for a group of hundreds of rows.
// A blob is checked (wave-uniformly) against its group's own stream [64 bases[e], 64 bases[e + 1]) and against packed_bytes before it is
// touched; all sizes are multiples of 64, so the check is made in units.
struct GroupRows {
    int64_t r0, r1;
};

__device__ __forceinline__ GroupRows group_rows_of(const int32_t *__restrict__ group_rows, int64_t e, int64_t T)
{
    GroupRows g;
    g.r0 = std::min<int64_t>(std::max<int64_t>(group_rows[e], 0), T);
    g.r1 = std::min<int64_t>(std::max<int64_t>(group_rows[e + 1], g.r0), T);
    return g;
}

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_linear_skinny_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const uint8_t *__restrict__ packed, uint64_t packed_bytes, const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets,
    const uint64_t *__restrict__ bases, int count, int N, int tiles_h, int tiles_w, int split, const float *__restrict__ bias, int64_t ldb,
    void *__restrict__ yv, int64_t ldy, float *__restrict__ ws)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)tiles_h * count * split) return;   // wave-uniform; the kernel has no barrier
    const int64_t tr = unit % tiles_h, se = unit / tiles_h, e = se % count, s = se / count;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    if (gr.r1 == gr.r0) return;                      // nothing of this expert is read
    const PackedStream st = arena_stream(packed, packed_bytes, maps, offsets, bases, e, (int64_t)tiles_h * tiles_w);
    const int64_t c0 = s * tiles_w / split, c1 = (s + 1) * tiles_w / split;

    for (int64_t row0 = gr.r0; row0 < gr.r1; row0 += kTile) {
        int lv = lane;
        asm volatile("" : "+v"(lv));                 // the lane's addresses are formed per chunk, not kept in registers across chunks
        const int row = lv & 31, half = lv >> 5;
        const int64_t n = tr * kTile + row;
        const int64_t M = std::min<int64_t>(kTile, gr.r1 - row0);
        f32x16 acc = zero16();
        skinny_run(acc, FeedDirect(), x + row0 * ldx, M, K, ldx, x_vec, st, tr * tiles_w, 1, c0, c1, lane, row, half, 2 * row + half);

        // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tr + row)
        if (n < N) store_skinny<BF16OUT>(acc, M, half, row0, n, split, split == 1 && bias ? bias[e * ldb + n] : 0.0f, yv, ldy, ws, s, T, N);
    }
}

// One workgroup per (group e, 256 columns): thread n walks the group's clamped rows, so only rows inside a clamped group are written,
// whatever group_rows holds.  Per output: ((p0 + p1) + ... + p_{split-1}) + b[e], as skinny_reduce_kernel.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void skinny_grouped_reduce_kernel(const float *__restrict__ ws, int64_t T, int64_t N, int split,
                                                                    const int32_t *__restrict__ group_rows, int64_t nchunks,
                                                                    const float *__restrict__ bias, int64_t ldb, void *__restrict__ yv, int64_t ldy)
{
    const int64_t e = blockIdx.x / nchunks, n = (blockIdx.x % nchunks) * 256 + threadIdx.x;
    if (n >= N) return;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    if (gr.r1 == gr.r0) return;
    const float bv = bias ? bias[e * ldb + n] : 0.0f;
    for (int64_t m = gr.r0; m < gr.r1; ++m) {
        float v = ws[m * N + n];
        for (int s = 1; s < split; ++s) v += ws[((int64_t)s * T + m) * N + n];
        v += bv;
        store_y<BF16OUT>(yv, m * ldy + n, v);
    }
}

// ---- the combine of an MoE layer in the grouped skinny reduce: skinny_grouped_reduce_kernel and moe_combine_kernel (mtq_moe.hip) in one.
//
// One workgroup per (token t, 256 columns), thread n.  acc starts at (float) base[t][n] or +0; for j = 0 .. K - 1 in order, with
// r = row_of[t * K + j] inside [0, S): v = ((p0 + p1) + ... + p_{split-1}) + 0.0f over the slices of ws [split][S][N] ascending, the
// + 0.0f being the grouped entries' bias add without a bias (it turns a -0 sum into +0); EXPERT_BF16 rounds v to bf16 once and widens
// it, the rounding a bf16 ys would have had; acc = fl32(acc + fl32(w[t][j] * v)).  A slot with r outside [0, S) is skipped by a
// branch the whole workgroup takes (t is the workgroup's), never multiplied by zero, so rows of ws that no kept slot names are never
// read.  base_kind: 0 none, 1 bf16, 2 float32.  No atomics, nothing waits on another workgroup.
template <bool EXPERT_BF16, bool BF16OUT>
__global__ __launch_bounds__(256) void skinny_grouped_combine_kernel(const float *__restrict__ ws, int64_t S, int64_t N, int split,
                                                                     const int32_t *__restrict__ row_of, const float *__restrict__ weights,
                                                                     int64_t ldw, const void *__restrict__ base, int base_kind, int64_t ldbase,
                                                                     int K, int64_t nchunks, void *__restrict__ yv, int64_t ldy)
{
#pragma clang fp contract(off)
    const int64_t t = blockIdx.x / nchunks, n = (blockIdx.x % nchunks) * 256 + threadIdx.x;
    if (n >= N) return;
    float acc = 0.0f;
    if (base_kind == 1) acc = __uint_as_float((uint32_t) static_cast<const uint16_t *>(base)[t * ldbase + n] << 16);
    else if (base_kind == 2) acc = static_cast<const float *>(base)[t * ldbase + n];
    const int32_t *rows = row_of + t * K;
    const float *w = weights + t * ldw;
    for (int j = 0; j < K; ++j) {
        const int64_t r = rows[j];
        if (r < 0 || r >= S) continue;               // uniform over the workgroup
        float v = ws[r * N + n];
        for (int s = 1; s < split; ++s) v += ws[((int64_t)s * S + r) * N + n];
        v += 0.0f;
        if constexpr (EXPERT_BF16) v = __uint_as_float((uint32_t)f32_to_bf16(v) << 16);
        acc = __fadd_rn(acc, __fmul_rn(w[j], v));
    }
    store_y<BF16OUT>(yv, t * ldy + n, acc);
}

// ---- grouped skinny linear, a wave per 32-row chunk: the kernel above with its `for row0` loop handed out over waves.
//
// A unit is (slice s, chunk slot c, tile row tr), numbered ((s * slots + c) * tiles_h + tr): the four waves of a workgroup share a slice
// and, but for a seam, a chunk, i.e. the same rows of X, as in the kernel above.  (Chunks of one group next to each other in a workgroup
// would share a W run instead; a full chunk's X is 2 KiB a tile, no less than any packed tile, and X is what the waves of a workgroup
// share at every routing, a one-chunk group included.)  The chunks of all groups are numbered through: group e owns chunks
// [cstart[e], cstart[e + 1]), cstart the exclusive prefix sum of ceil(rows_e / 32) over the clamped groups, written by
// packed_grouped_plan_kernel on the same stream before this kernel.  slots is the host's bound on cstart[count], formed from
// (T, count) alone: floor((T + 31 min(count, T)) / 32).  A wave whose slot is at or past cstart[count] returns before any other load;
// chunks at or past `slots` (overlapping groups of a decreasing group_rows only) are not computed.
// The wave finds its group by search, not from a per-chunk table: cstart is count + 1 words whatever T is, a table would be `slots`
// words written by a plan kernel that walks them; the search is wave-uniform (scalar loads) down to a window of 64 entries, which one
// load, a lane each, and a ballot finish - for count <= 64 that one load is the whole search.
// On its chunk the wave calls skinny_run and store_skinny as the kernel above does for (expert, chunk, slice): the same bits.

// start[0 .. count], by one workgroup, for units of ROWS rows (32: the chunks of this kernel, cstart; 128: the blocks of the grouped wide
// kernels, bstart): thread k sums the unit counts of groups [k * per, (k + 1) * per), the workgroup scans the 256 sums, and a second
// pass over the same run writes the prefix (packed_bases_kernel's pattern).  Sums are 64-bit and stored saturated at INT32_MAX, above
// every slot number, so the prefix stays nondecreasing whatever group_rows holds.
template <int ROWS>
__global__ __launch_bounds__(256) void packed_grouped_plan_kernel(const int32_t *__restrict__ group_rows, int count, int T,
                                                                  int32_t *__restrict__ start)
{
    __shared__ unsigned long long lds[4];
    const int64_t per = ((int64_t)count + 255) / 256;
    const int64_t i0 = std::min<int64_t>((int64_t)threadIdx.x * per, count), i1 = std::min<int64_t>(i0 + per, count);
    unsigned long long sum = 0ull;
    for (int64_t e = i0; e < i1; ++e) {
        const GroupRows gr = group_rows_of(group_rows, e, T);
        sum += (unsigned long long)((gr.r1 - gr.r0 + ROWS - 1) / ROWS);
    }
    unsigned long long total;
    unsigned long long run = block_exclusive_scan(sum, lds, total);
    for (int64_t e = i0; e < i1; ++e) {
        start[e] = (int32_t)std::min<unsigned long long>(run, INT32_MAX);
        const GroupRows gr = group_rows_of(group_rows, e, T);
        run += (unsigned long long)((gr.r1 - gr.r0 + ROWS - 1) / ROWS);
    }
    if (threadIdx.x == 0) start[count] = (int32_t)std::min<unsigned long long>(total, INT32_MAX);
}

// The group of slot `slot` (below start[count]): the last e with start[e] <= slot.  Wave-uniform (scalar loads) down to a window of 64
// entries, which one load, a lane each, and a ballot finish.
__device__ __forceinline__ int group_of_slot(const int32_t *__restrict__ start, int count, int slot, int lane)
{
    int lo = 0, hi = count;                          // start[lo] <= slot < start[hi] throughout
    while (hi - lo > 64) {
        const int mid = lo + (hi - lo) / 2;
        if (start[mid] <= slot) lo = mid;
        else hi = mid;
    }
    const int at = lo + 1 + lane;
    return lo + (int)__popcll(__ballot(at < hi && start[at] <= slot));
}

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_linear_skinny_grouped_chunked_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const int32_t *__restrict__ cstart, int slots, const uint8_t *__restrict__ packed, uint64_t packed_bytes,
    const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets, const uint64_t *__restrict__ bases, int count, int N, int tiles_h,
    int tiles_w, int split, const float *__restrict__ bias, int64_t ldb, void *__restrict__ yv, int64_t ldy, float *__restrict__ ws)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)tiles_h * slots * split) return;   // wave-uniform; the kernel has no barrier
    const int64_t tr = unit % tiles_h, sc = unit / tiles_h, s = sc / slots;
    const int c = (int)(sc % slots);
    if (c >= cstart[count]) return;                  // a surplus slot: nothing else is read
    const int e = group_of_slot(cstart, count, c, lane);
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int64_t row0 = gr.r0 + (int64_t)(c - cstart[e]) * kTile;
    if (row0 >= gr.r1) return;                       // never for a prefix this launch's plan kernel wrote
    const PackedStream st = arena_stream(packed, packed_bytes, maps, offsets, bases, e, (int64_t)tiles_h * tiles_w);

    const int row = lane & 31, half = lane >> 5;
    const int64_t n = tr * kTile + row;
    const int64_t M = std::min<int64_t>(kTile, gr.r1 - row0);
    f32x16 acc = zero16();
    skinny_run(acc, FeedDirect(), x + row0 * ldx, M, K, ldx, x_vec, st, tr * tiles_w, 1, s * tiles_w / split, (s + 1) * tiles_w / split, lane, row,
               half, 2 * row + half);

    // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tr + row)
    if (n >= N) return;
    store_skinny<BF16OUT>(acc, M, half, row0, n, split, split == 1 && bias ? bias[e * ldb + n] : 0.0f, yv, ldy, ws, s, T, N);
}

// ---- grouped skinny matmul: the (k, n) experts of one arena, each over its own rows of X, in one launch.
//
// packed_matmul_skinny_kernel's wave in the two grouped frames above.  The walk kernel's unit is (slice s, group e, tile column tc),
// numbered (s * count + e) * tiles_nw + tc, the chunked kernel's (slice s, chunk slot c, tile column tc), numbered
// (s * slots + c) * tiles_nw + tc; the run is tiles tc + c * tiles_nw of expert e's tables over the slice's tile rows, through the wave's
// two [32 k][32 n] images.  On a 32-row chunk the wave does what packed_matmul_skinny_kernel does for an m <= 32 call on that chunk with
// expert e's stream and tables at the same split: that call's bits, hence the grouped linear kernels' on the transposed weight.
//
// EXEC at the transposed reads.  Everything a branch before or between runs depends on is wave-uniform and held in scalar registers: the
// wave index, the unit, the group's clamped rows and the chunk's first row go through readfirstlane, so "unit past the grid", "empty
// group", "surplus slot", "row0 >= r1" and the walk kernel's chunk loop (its trip count is the group's alone) are scalar branches taken
// by the whole wave or by none of it.  The one lane-dependent branch is the n < N guard around the stores, after a run; EXEC is whole
// again behind it, before the next chunk's run.  M = min(32, r1 - row0) is the row limit of every X load of a chunk; k-rows at or
// past K and tiles with a bad code or a blob outside [64 bases[e], 64 bases[e + 1]) or past packed_bytes are zeros in the image.

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_matmul_skinny_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const uint8_t *__restrict__ packed, uint64_t packed_bytes, const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets,
    const uint64_t *__restrict__ bases, int count, int N, int tiles_kh, int tiles_nw, int split, const float *__restrict__ bias, int64_t ldb,
    void *__restrict__ yv, int64_t ldy, float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)tiles_nw * count * split) return;  // wave-uniform; the kernel has no workgroup barrier
    const int64_t tc = unit % tiles_nw, se = unit / tiles_nw, e = se % count, s = se / count;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int r0 = __builtin_amdgcn_readfirstlane((int)gr.r0), r1 = __builtin_amdgcn_readfirstlane((int)gr.r1);   // 0 <= r0 <= r1 <= T
    if (r1 == r0) return;                            // nothing of this expert is read
    const PackedStream st = arena_stream(packed, packed_bytes, maps, offsets, bases, e, (int64_t)tiles_kh * tiles_nw);
    const int64_t c0 = s * tiles_kh / split, c1 = (s + 1) * tiles_kh / split;
    uint16_t *img = lds + wave * (2 * kMmsImage);

    for (int64_t row0 = r0; row0 < r1; row0 += kTile) {   // scalar: the trip count is the group's
        int lv = lane;
        asm volatile("" : "+v"(lv));                 // the lane's addresses are formed per chunk, not kept in registers across chunks
        const int row = lv & 31, half = lv >> 5;
        const int64_t n = tc * kTile + row;
        const int64_t M = std::min<int64_t>(kTile, r1 - row0);
        f32x16 acc = zero16();
        skinny_run(acc, feed_transposed(img, lv), x + row0 * ldx, M, K, ldx, x_vec, st, tc, tiles_nw, c0, c1, lane, row, half, lv);

        // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tc + row)
        if (n < N) store_skinny<BF16OUT>(acc, M, half, row0, n, split, split == 1 && bias ? bias[e * ldb + n] : 0.0f, yv, ldy, ws, s, T, N);
    }
}

template <bool BF16OUT>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_matmul_skinny_grouped_chunked_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const int32_t *__restrict__ cstart, int slots, const uint8_t *__restrict__ packed, uint64_t packed_bytes,
    const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets, const uint64_t *__restrict__ bases, int count, int N, int tiles_kh,
    int tiles_nw, int split, const float *__restrict__ bias, int64_t ldb, void *__restrict__ yv, int64_t ldy, float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)tiles_nw * slots * split) return;  // wave-uniform; the kernel has no workgroup barrier
    const int64_t tc = unit % tiles_nw, sc = unit / tiles_nw, s = sc / slots;
    const int c = (int)(sc % slots);
    if (c >= cstart[count]) return;                  // a surplus slot: nothing else is read
    const int e = __builtin_amdgcn_readfirstlane(group_of_slot(cstart, count, c, lane));
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int r1 = __builtin_amdgcn_readfirstlane((int)gr.r1);
    const int64_t row0 = __builtin_amdgcn_readfirstlane((int)gr.r0) + (int64_t)(c - __builtin_amdgcn_readfirstlane(cstart[e])) * kTile;
    if (row0 >= r1) return;                          // never for a prefix this launch's plan kernel wrote
    const PackedStream st = arena_stream(packed, packed_bytes, maps, offsets, bases, e, (int64_t)tiles_kh * tiles_nw);

    const int row = lane & 31, half = lane >> 5;
    const int64_t n = tc * kTile + row;
    const int64_t M = std::min<int64_t>(kTile, r1 - row0);
    f32x16 acc = zero16();
    skinny_run(acc, feed_transposed(lds + wave * (2 * kMmsImage), lane), x + row0 * ldx, M, K, ldx, x_vec, st, tc, tiles_nw, s * tiles_kh / split,
               (s + 1) * tiles_kh / split, lane, row, half, lane);

    // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tc + row)
    if (n >= N) return;
    store_skinny<BF16OUT>(acc, M, half, row0, n, split, split == 1 && bias ? bias[e * ldb + n] : 0.0f, yv, ldy, ws, s, T, N);
}

// ---- wide linear (m above the decode range): packed_linear_kernel's bits from a 128 × 128 block.
//
// A workgroup of 4 waves, 2 (M) × 2 (N), owns a 128 (M) × 128 (N) block and walks K in steps of 64; each wave owns 64 × 64 outputs,
// four accumulators; two workgroups fit a CU.  The W block of a step is 4 tile rows × 2 tile columns: wave w takes the two tiles of
// tile row n0 / 32 + w, a lane the group of its own number, so a tile's format is uniform over the wave and its 64 loads cover the
// blob's codes end to end.  decode_skinny gives decode_group's words at a third of the instructions.
// Two LDS images of 256 rows at pitch kLdk and two register sets: while step s multiplies from image s & 1, the registers that hold
// step s + 1 are decoded into the other image between the MFMA groups; the loads of step s + 2 are issued at the top of step s, two
// steps ahead in program order, the map codes and offsets of step s + 3 with them (looked at a step after they were fetched).  How
// much of that runs beside the MFMAs is the compiler's s_waitcnt placement: today its waits before a staged register is used are mostly
// vmcnt(0), so a step still waits for the loads it has just issued.  One barrier per step, no atomics, no workspace,
// nothing waits on another workgroup.
// Bits: an output has one accumulator that starts at +0 and takes mfma_f32_32x32x16_bf16 over ascending blocks of 16 K positions, X as
// the A operand and W as B, positions 8h .. 8h + 7 in lane half h, K zero-filled to the step of 64, the bias added once in f32 at the
// end: packed_linear_kernel's sequence for that output, operand for operand, so the result is that kernel's bit for bit.
constexpr int kWideBM = 128, kWideBN = 128;

constexpr int kWideImage = (kWideBM + kWideBN) * kLdk;   // one LDS image: the X block and four tile-row slots of W
constexpr int kMwSub = kBK * kMmPitch;               // a wave's [64 k][32 n] sub-image of the k × n wide block, in bf16: 4 KB, no stagger
static_assert(kWideBM * kLdk + 4 * kMwSub <= kWideImage, "the k x n W part fits the n x k one");

template <int V>
struct Tag {                                         // a compile-time integer as an argument: a register set's parity
    static constexpr int value = V;
};

// A 64-bit value every lane of the wave holds alike, into scalar registers.
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// The 128-row block of every wide kernel: rows [m0, min(m0 + 128, M)) of x / y, M the row limit of every access.  Wave `wave` stages
// slot `wave` of the W part of the image (rows 32 wave ..) from tile row wtr of the stream st, which with its tables and limits is
// uniform over the wave and lives in scalar registers; wave (wm, wn) multiplies slots 2 wn and 2 wn + 1 into acc[mt][0] and acc[mt][1].
// The frame chooses what the slots are, and GLU the epilogue that goes with the choice:
//   linear  slot w is tile row n0 / 32 + w of one stream: a lane's two accumulators are two column tiles, n0 + 64 wn + 32 nt + lane % 32,
//           one bias.
//   GLU     slot w is hidden tile row n0 / 32 + (w >> 1), from the gate stream when w is even and from the up stream when w is odd: the
//           two accumulators are the gate's and the up's output at the SAME column n0 + 32 wn + lane % 32, so glu_value is lane-local.
// Launched with bounds (kThreads, 2): the second is HIP's minimum of waves per SIMD, not workgroups per CU; a workgroup here is one wave
// per SIMD, so 2 is what lets two workgroups share a CU and caps the kernels at 256 VGPRs, which this function uses to the last:
// re-read `make report` on any edit.
template <bool GLU, bool XV, bool BF16OUT, bool WT = false>
__device__ __forceinline__ void wide_block(uint16_t *__restrict__ lds, const uint16_t *__restrict__ x, int64_t m0, int64_t M, int64_t K,
                                           int64_t ldx, const PackedStream &st, int64_t wtr, int64_t n0, int64_t N, int64_t tiles_h,
                                           int64_t tiles_w, const float *__restrict__ bias, const float *__restrict__ bias_up, int act,
                                           void *__restrict__ yv, int64_t ldy, int wave)
{
    constexpr int BM = kWideBM, MT = BM / 64, XP = BM * 8 / kThreads, kImage = kWideImage;   // a wave's 32-row MFMA blocks; pieces of 8 bf16 of the X block per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t steps = (K + kBK - 1) / kBK;
    const uint8_t *__restrict__ packed = st.packed;
    const int8_t *__restrict__ map = st.map;
    const uint32_t *__restrict__ off = st.off;

    f32x16 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = zero16();

    uint4 xr[2][XP];                                 // register set p holds the steps of parity p
    GroupRaw wr[2][2];
    int tf[2];                                       // map code and offset of the wave's two tiles of the step after the last one loaded,
    uint32_t to[2];                                  // fetched a step before they are looked at: no load waits for them
    // WT: wtr is the wave's tile COLUMN and the pair is tile rows 2 s and 2 s + 1 of it, tiles_w tiles apart, so every fetch leaves the
    // first-level caches.  A uniform byte load is read to a scalar register, and waited for, where it is issued - twice a step; so lane l
    // loads the code of tile row 2 s + (l & 1) itself, the value stays in a vector register and is handed out with readlane when
    // load_step looks at it a step later (tfv, tth), and an offset is not touched here either: nothing waits in this function.
    int tfv = 0;
    bool tth[2] = {false, false};
    auto fetch_tables = [&](int64_t s) __attribute__((always_inline)) {
        if constexpr (WT) {
            const int64_t tr = 2 * s + (lane & 1);
            tfv = map[tr < tiles_h && wtr < tiles_w ? tr * tiles_w + wtr : 0];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                tth[i] = 2 * s + i < tiles_h && wtr < tiles_w;
                to[i] = off[tth[i] ? (2 * s + i) * tiles_w + wtr : 0];       // of tile 0 when the tile is absent: never used (f < 0)
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t wtc = 2 * s + i;
                const bool there = wtr < tiles_h && wtc < tiles_w;
                const int64_t t = there ? wtr * tiles_w + wtc : 0;           // tile 0 is always there: the loads are unconditional
                const int f = map[t];
                const uint32_t o = off[t];
                tf[i] = there ? f : -1;
                to[i] = there ? o : 0u;
            }
        }
    };
    // load_group for a whole tile by one wave (lane = group), with two loads whatever the tile is: every step issues the same
    // number of loads on every path, which is what a counted wait for an earlier step's registers needs (the compiler does not
    // emit one yet: the wide section's head comment).
    // A tile that is not there reads bytes of the first 320 of `packed`, the stream's or the ARENA's head (they are there: the entry
    // checks packed_bytes against 320 bytes per tile), not of a group's own stream, which a cut-short `bases` may not own, and keeps
    // f < 0, which decodes as zeros.
    auto load_tile = [&](const TileAt &a, GroupRaw &g) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) g.w[i] = 0u;
        g.E = 0u;
        g.f = a.f;
        const int f = __builtin_amdgcn_readfirstlane(a.f);                   // uniform over the wave
        const uint8_t *blob = packed + (f < 0 ? 0 : uniform64(a.off));
        if (f == 0) {
            const uint4 *q = reinterpret_cast<const uint4 *>(blob + lane * 32);
            const uint4 lo = q[0], hi = q[1];
            g.w[0] = lo.x; g.w[1] = lo.y; g.w[2] = lo.z; g.w[3] = lo.w;
            g.w[4] = hi.x; g.w[5] = hi.y; g.w[6] = hi.z; g.w[7] = hi.w;
        } else if (f == 1) {
            g.E = blob[lane];
            const uint4 v = *reinterpret_cast<const uint4 *>(blob + kExpBytes + lane * 16);
            g.w[0] = v.x; g.w[1] = v.y; g.w[2] = v.z; g.w[3] = v.w;
        } else if (f == 2) {
            g.E = blob[lane];
            const uint2 v = *reinterpret_cast<const uint2 *>(blob + kExpBytes + lane * 8);
            g.w[0] = v.x; g.w[1] = v.y;
        } else {
            g.E = blob[lane];
            g.w[0] = *reinterpret_cast<const uint32_t *>(blob + kExpBytes + lane * 4);
        }
    };
    auto load_step = [&](auto par, int64_t s) __attribute__((always_inline)) {
        constexpr int p = decltype(par)::value;
        const int64_t k0 = s * kBK;
        if constexpr (WT) {
#pragma unroll
            for (int i = 0; i < 2; ++i) tf[i] = tth[i] ? __builtin_amdgcn_readlane(tfv, i) : -1;
        }
        const TileAt ta[2] = {stream_at(st, tf[0], to[0]), stream_at(st, tf[1], to[1])};   // the fetched pair, guarded
        if constexpr (!WT) fetch_tables(s + 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) load_tile(ta[i], wr[p][i]);
#pragma unroll
        for (int j = 0; j < XP; ++j) {               // columns past K and rows past M are zeros, never read
            const int q = tid + kThreads * j, row = q >> 3, c8 = (q & 7) * 8;
            const int64_t gm = m0 + row, gk = k0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (XV) {                      // K % 8 == 0: a piece is inside or outside; the load is of a piece inside (m0 <= M - 1)
                const bool inside = gm < M && gk < K;
                const uint4 got = *reinterpret_cast<const uint4 *>(x + (gm < M ? gm : M - 1) * ldx + (gk < K ? gk : K - 8));
                if (inside) v = got;
            } else if (gm < M && gk < K) {
                const uint16_t *src = x + gm * ldx + gk;
                uint32_t h[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) h[c] = gk + c < K ? (uint32_t)src[c] : 0u;
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
            xr[p][j] = v;
        }
        // WT: the step's newest load.  The waits the compiler places before a register of an earlier step is written again count back
        // from the newest load; behind the tile and X loads the fetch stays in flight through them, in front it would be waited for.
        if constexpr (WT) fetch_tables(s + 1);
    };
    // register set p → image `img`: tile i of the wave's slot (rows 32 wave .. of the W part), and X pieces [j0, j1)
    // WT: the lane's group is k-row 32 i + lane / 2 of step s, 16 values along n, and goes as it lies to bytes 2048 i + 32 lane of the
    // wave's [64 k][32 n] sub-image; a k-row at or past K is zeros in the image whatever the stream holds.  Lanes with (lane >> 2) & 1
    // set store their upper piece first (FeedTransposed's order): each 16-byte store of an 8-lane group covers 32 distinct banks.
    auto stage_w = [&](auto par, int i, uint16_t *img, int64_t s) __attribute__((always_inline)) {
        constexpr int p = decltype(par)::value;
        uint32_t y[kGroup];
        decode_skinny(wr[p][i], y);
        uint4 lo, hi;
        pack_halves(y, lo, hi);
        if constexpr (WT) {
            const bool pad = s * kBK + kTile * i + (lane >> 1) >= K, up = (lane >> 2) & 1;
            if (pad) lo = hi = make_uint4(0u, 0u, 0u, 0u);
            uint16_t *d = img + BM * kLdk + wave * kMwSub + (kTile * i) * kMmPitch + lane * kGroup;
            *reinterpret_cast<uint4 *>(d + 8 * up) = make_uint4(up ? hi.x : lo.x, up ? hi.y : lo.y, up ? hi.z : lo.z, up ? hi.w : lo.w);
            *reinterpret_cast<uint4 *>(d + 8 * (up ^ 1)) = make_uint4(up ? lo.x : hi.x, up ? lo.y : hi.y, up ? lo.z : hi.z, up ? lo.w : hi.w);
        } else {
            uint4 *d = reinterpret_cast<uint4 *>(img + (BM + kTile * wave + (lane >> 1)) * kLdk + kTile * i + kGroup * (lane & 1));
            d[0] = lo;
            d[1] = hi;
        }
    };
    auto stage_x = [&](auto par, int j0, int j1, uint16_t *img) __attribute__((always_inline)) {
        constexpr int p = decltype(par)::value;
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            const int q = tid + kThreads * j;
            *reinterpret_cast<uint4 *>(img + (q >> 3) * kLdk + (q & 7) * 8) = xr[p][j];
        }
    };
    // MFMA group kk of a step: the 16 K positions 16 kk .. of the images xs / ws, 2 MT MFMAs; nt = 0 is slot 2 wn, nt = 1 slot 2 wn + 1
    auto mfma_group = [&](const uint16_t *xs, const uint16_t *ws, int kk) __attribute__((always_inline)) {
        const int koff = kk * 16 + 8 * (lane >> 5);
        bf16x8 b[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            if constexpr (WT) {                      // packed_matmul_kernel's lane addressing in sub-image 2 wn + nt: k + 0..3, then k + 4..7
                const uint16_t *src = ws + (2 * wn + nt) * kMwSub + (kk * 16 + 8 * (lane >> 5) + ((lane >> 2) & 3)) * kMmPitch +
                                      16 * ((lane >> 4) & 1) + 4 * (lane & 3);
                const i16x4 b0 = lds_read_tr16(src), b1 = lds_read_tr16(src + 4 * kMmPitch);
                b[nt] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
            } else {
                b[nt] = *reinterpret_cast<const bf16x8 *>(ws + (64 * wn + 32 * nt + (lane & 31)) * kLdk + koff);
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xs + (32 * MT * wm + 32 * mt + (lane & 31)) * kLdk + koff);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[nt], acc[mt][nt], 0, 0, 0);
        }
    };
    // step s from image s & 1; the registers of step s + 1 go to the other image between the MFMA groups (two waves to a SIMD: the
    // other workgroup's MFMAs run beside this wave's decode)
    auto step = [&](auto par, int64_t s) __attribute__((always_inline)) {
        constexpr int cur = decltype(par)::value;
        const Tag<cur ^ 1> other;
        const uint16_t *xs = lds + cur * kImage, *ws = xs + BM * kLdk;
        uint16_t *next = lds + (cur ^ 1) * kImage;
        const bool more = s + 1 < steps;
        load_step(par, s + 2 < steps ? s + 2 : steps - 1);   // into this parity's registers, staged a step ago; past the end the
                                                     // last step is loaded again and not used: the same loads on every path
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) {
            if (!more) {
                mfma_group(xs, ws, kk);
            } else if (kk < 2) {
                mfma_group(xs, ws, kk);
                stage_w(other, kk, next, s + 1);
            } else {
                mfma_group(xs, ws, kk);
                stage_x(other, (kk - 2) * (XP / 2), (kk - 1) * (XP / 2), next);
            }
        }
        __syncthreads();
    };

    fetch_tables(0);
    load_step(Tag<0>(), 0);
    load_step(Tag<1>(), steps > 1 ? 1 : 0);
    stage_w(Tag<0>(), 0, lds, 0);
    stage_w(Tag<0>(), 1, lds, 0);
    stage_x(Tag<0>(), 0, XP, lds);
    __syncthreads();
    int64_t s = 0;
    for (; s + 1 < steps; s += 2) {
        step(Tag<0>(), s);
        step(Tag<1>(), s + 1);
    }
    if (s < steps) {                                 // an odd count's last step: nothing left to load or stage
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) mfma_group(lds, lds + BM * kLdk, kk);
    }

    // epilogue: lane's rows are m0 + 32 MT·wm + 32 mt + (r&3) + 8(r>>2) + 4(lane>>5); the bias is added as the block kernel adds it (+0
    // without one), glu_value is the one place the activation is computed
    if constexpr (GLU) {
        const int64_t n = n0 + 32 * wn + (lane & 31);
        if (n >= N) return;
        const float bg = bias ? bias[n] : 0.0f, bu = bias_up ? bias_up[n] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + 32 * MT * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < M) store_y<BF16OUT>(yv, m * ldy + n, glu_value(acc[mt][0][r] + bg, acc[mt][1][r] + bu, act));
            }
    } else {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t n = n0 + 64 * wn + 32 * nt + (lane & 31);
            if (n >= N) continue;
            const float b = bias ? bias[n] : 0.0f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = m0 + 32 * MT * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < M) store_y<BF16OUT>(yv, m * ldy + n, acc[mt][nt][r] + b);
                }
        }
    }
}

// The frames below take the orientation as WT and hand it to wide_block; tiles_h × tiles_w is the tile grid of the stream as it was
// packed: of the n × k weight, or with WT of the k × n matrix.
//
// ---- wide matmul (WT): Y = X·P̂ + b for a packed k × n matrix from the wide block, for m >= 64.
//
// wide_block<.., WT = true>: everything of the block but its W side.  The stream is of a k × n matrix, so a step's W block is 2 tile rows
// × 4 tile columns: wave w takes tile column n0 / 32 + w and, at step s, its tiles of the tile rows 2 s and 2 s + 1, a lane the group of its
// own number (k-row 64 s + 32 i + lane / 2, columns n0 + 32 w + 16 (lane & 1) ..).  The W part of an image is four [64 k][32 n] sub-images
// at packed_matmul_kernel's 64-byte pitch, 4 KB each and back to back (16 KB of the 18 KB the n × k block takes): a wave writes its own
// sub-image end to end, 32 bytes a lane, and wave (wm, wn) reads sub-images 2 wn and 2 wn + 1 through the transposed LDS read, two reads
// per operand with packed_matmul_kernel's lane addressing.  The same k at the same lane half and element, ascending kk, the same K step,
// zeros at and past K: packed_matmul_kernel's bits.
// Banks: a 32-lane half of a transposed read takes 4 k-rows × 64 bytes of ONE sub-image, 256 consecutive bytes, every bank once.  A
// 16-byte store goes by 8-lane groups over 32 banks; bytes 32 lane would put lanes i and i + 4 on the same banks, so those lanes store
// their upper piece first.  No instruction touches two sub-images, and each starts on a multiple of 256 bytes: §A.6p's 16-byte shift
// between sub-images has nothing left to separate.
// EXEC is all ones at every transposed read: they sit in wave-uniform control flow only, and nothing returns before the epilogue.
template <bool XV, bool BF16OUT, bool WT>
__global__ __launch_bounds__(kThreads, 2) void packed_wide_kernel(
    const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, const uint8_t *__restrict__ packed, uint64_t packed_bytes,
    const int8_t *__restrict__ map, const uint32_t *__restrict__ offsets, int64_t N, int64_t tiles_h, int64_t tiles_w,
    const float *__restrict__ bias, void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kWideImage];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nblocks = (N + kWideBN - 1) / kWideBN;
    const int64_t bm = blockIdx.x / nblocks, n0 = (blockIdx.x % nblocks) * kWideBN;
    wide_block<false, XV, BF16OUT, WT>(lds, x, bm * kWideBM, M, K, ldx, tensor_stream(packed, packed_bytes, map, offsets), (n0 >> 5) + wave, n0,
                                       N, tiles_h, tiles_w, bias, nullptr, 0, yv, ldy, wave);
}

// ---- grouped wide linear: packed_wide_kernel's block for every expert of an arena over the expert's own rows, one launch.
//
// The 128-row blocks of all groups are numbered through, as the chunked kernel numbers 32-row chunks: group e owns blocks
// [bstart[e], bstart[e + 1]), bstart the exclusive prefix sum of ceil(rows_e / 128) over the clamped groups, written by
// packed_grouped_plan_kernel<128> on the same stream before this kernel.  The grid is slots × ceil(N / 128) workgroups, the column block
// fastest; slots is the host's bound on bstart[count], formed from (T, count) alone: floor((T + 127 min(count, T)) / 128).  A workgroup
// whose slot is at or past bstart[count] returns before any other load and before any barrier; blocks at or past `slots` (overlapping
// groups of a decreasing group_rows only) are not computed.  The group of a slot is found by the chunked kernel's search
// (group_of_slot), by every wave alike: the group, its rows, its tables and its stream are uniform over the workgroup and live in
// scalar registers.
// On its block the workgroup calls wide_block as packed_wide_kernel does, for x[r0:r1] and expert e's stream and tables at row
// block (slot - bstart[e]): M is the group's end r1 (every row limit, the clamped 16-byte X loads included), a blob is checked against
// the group's own stream and against packed_bytes, an absent tile's unconditional loads read the arena's first 320 bytes.  The same
// function, so that kernel's bits, which are the block kernel's.
//
// ---- grouped wide matmul (WT): packed_wide_kernel<.., WT = true>'s block for every (k, n) expert of an arena over the expert's own rows.
//
// The same frame with wide_block<.., WT = true>: the plan (packed_grouped_plan_kernel<128>), the slot bound, the grid of slots ×
// ceil(N / 128) with the column block fastest, the search and the stream in scalar registers are unchanged; wave w stages tile COLUMN
// n0 / 32 + w of expert e's k × n tables, and M is the group's clamped end.  The same function as packed_wide_kernel<.., true> on
// x[r0:r1] with expert e's stream, so that kernel's bits, which are packed_matmul_kernel's.
// EXEC is all ones at every transposed read: the surplus-slot return is taken by the whole workgroup before any barrier, and everything
// behind it is wide_block's wave-uniform control flow.

// What the grouped wide frames share: block `slot` is rows [m0, min(m0 + 128, M)) of group e, all uniform over the workgroup and in
// scalar registers.  False for a surplus slot, after the load of bstart[count] alone: the frame returns, before any barrier.
struct GroupBlock {
    int e;
    int64_t m0, M;
};

__device__ __forceinline__ bool group_block(const int32_t *__restrict__ bstart, int count, int slot, const int32_t *__restrict__ group_rows, int T,
                                            int lane, GroupBlock &b)
{
    if (slot >= bstart[count]) return false;
    b.e = __builtin_amdgcn_readfirstlane(group_of_slot(bstart, count, slot, lane));
    const GroupRows gr = group_rows_of(group_rows, b.e, T);
    const int64_t r0 = __builtin_amdgcn_readfirstlane((int)gr.r0);           // 0 <= r0 <= M <= T
    b.M = __builtin_amdgcn_readfirstlane((int)gr.r1);
    b.m0 = r0 + (int64_t)kWideBM * (slot - __builtin_amdgcn_readfirstlane(bstart[b.e]));
    return b.m0 < b.M;                               // never false for a prefix this launch's plan kernel wrote
}

// arena_stream with its limits in scalar registers
__device__ __forceinline__ PackedStream arena_stream_uniform(const uint8_t *packed, uint64_t packed_bytes, const int8_t *maps,
                                                             const uint32_t *offsets, const uint64_t *bases, int64_t e, int64_t tiles)
{
    PackedStream st = arena_stream(packed, packed_bytes, maps, offsets, bases, e, tiles);
    st.base = uniform64(st.base);
    st.limit = uniform64(st.limit);
    return st;
}

template <bool XV, bool BF16OUT, bool WT>
__global__ __launch_bounds__(kThreads, 2) void packed_wide_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int64_t K, int64_t ldx, const int32_t *__restrict__ group_rows, const int32_t *__restrict__ bstart,
    const uint8_t *__restrict__ packed, uint64_t packed_bytes, const int8_t *__restrict__ maps, const uint32_t *__restrict__ offsets,
    const uint64_t *__restrict__ bases, int count, int64_t N, int64_t tiles_h, int64_t tiles_w, const float *__restrict__ bias, int64_t ldb,
    void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kWideImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nblocks = (N + kWideBN - 1) / kWideBN;
    const int64_t n0 = (blockIdx.x % nblocks) * kWideBN;
    GroupBlock b;
    if (!group_block(bstart, count, (int)(blockIdx.x / nblocks), group_rows, T, lane, b)) return;   // the whole workgroup, before any barrier
    const PackedStream st = arena_stream_uniform(packed, packed_bytes, maps, offsets, bases, b.e, tiles_h * tiles_w);
    wide_block<false, XV, BF16OUT, WT>(lds, x, b.m0, b.M, K, ldx, st, (n0 >> 5) + wave, n0, N, tiles_h, tiles_w,
                                       bias ? bias + b.e * ldb : nullptr, nullptr, 0, yv, ldy, wave);
}

// ---- gated wide linear (SwiGLU): glu_value(X·Ŵgᵀ + bg, X·Ŵuᵀ + bu) from packed_wide_kernel's step, one launch, one store.
//
// A workgroup of 4 waves owns 128 rows × 64 HIDDEN columns.  The W part of its LDS image keeps the wide kernel's four tile-row slots:
// slot sl holds hidden tile row n0 / 32 + (sl >> 1), from the gate stream when sl is even and from the up stream when sl is odd.  Wave w
// stages slot w, as there: its stream, its tables and its limits are uniform over the wave and chosen once, in scalar registers.  Wave
// (wm, wn) multiplies slots 2 wn and 2 wn + 1 with the wide kernel's mfma_group unchanged, so acc[mt][0] is the gate's and acc[mt][1]
// the up's output at the SAME (row, hidden column n0 + 32 wn + lane % 32): the epilogue is lane-local.  The loads (unconditional, an
// absent tile clamped to its stream's tile 0 and read from the stream's head), the blob check against the tile's own stream, a map code
// outside 0..3 as zeros, both X paths, two images, two register sets, one barrier per step: packed_wide_grouped_kernel's, with
// the stream limits in units ([base, limit) of 64 bytes; for a single tensor base = 0, limit = packed_bytes / 64, the byte check's
// equal since every blob size is a multiple of 64).
// Bits: each accumulator takes the block kernel's sequence for its projection, the bias is added once in f32 as there, and glu_value
// (mtq_glu.hpp) is what mtq_glu_combine applies to the two stored f32 results: the unfused route's bits.
//
// ---- gated wide matmul (WT): glu_value(X·P̂g + bg, X·P̂u + bu) for packed k × n gate and up matrices.
//
// The same frame around wide_block<true, .., WT = true>: a workgroup owns 128 rows × 64 hidden columns, wave w stages sub-image w of the
// [64 k][32 n] W part, which is hidden tile COLUMN n0 / 32 + (w >> 1) of the k × n grid tiles_h × tiles_w, from the gate stream when w is
// even and from the up stream when w is odd; wave (wm, wn) reads sub-images 2 wn and 2 wn + 1 through the transposed LDS read, so
// acc[mt][0] is the gate's and acc[mt][1] the up's output at the same (row, hidden column n0 + 32 wn + lane % 32) and the epilogue is
// lane-local glu_value.  Each accumulator takes packed_wide_kernel<.., WT = true>'s sequence for its projection (that kernel's bits are
// packed_matmul_kernel's), the bias is added once in f32 and glu_value is what mtq_glu_combine applies: the bits of two
// mtq_packed_matmul calls into f32 and the combine.
// Pad, don't mask: a bad map code, a blob past its own stream's range and k-rows at or past K are zeros in the image; columns at or past
// N are never stored.  No atomics, no workspace but the grouped plan, nothing waits on another workgroup.
// EXEC is all ones at every transposed read: the single-tensor frame returns nowhere before the epilogue; the grouped frame's
// surplus-slot return is taken by the whole workgroup before any barrier; behind either is wide_block's wave-uniform control flow,
// where no read sits in a lane-dependent branch.
constexpr int kGluBN = 64;                           // hidden columns of a workgroup

template <bool XV, bool BF16OUT, bool WT>
__global__ __launch_bounds__(kThreads, 2) void packed_glu_wide_kernel(
    const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, const uint8_t *__restrict__ gate, uint64_t gate_bytes,
    const int8_t *__restrict__ gate_map, const uint32_t *__restrict__ gate_offsets, const uint8_t *__restrict__ up, uint64_t up_bytes,
    const int8_t *__restrict__ up_map, const uint32_t *__restrict__ up_offsets, int64_t N, int64_t tiles_h, int64_t tiles_w,
    const float *__restrict__ bias_gate, const float *__restrict__ bias_up, int act, void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kWideImage];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nblocks = (N + kGluBN - 1) / kGluBN;
    const int64_t bm = blockIdx.x / nblocks, n0 = (blockIdx.x % nblocks) * kGluBN;
    const bool is_up = wave & 1;                     // the wave's slot or sub-image: even from the gate stream, odd from the up stream
    const PackedStream st = tensor_stream(is_up ? up : gate, is_up ? up_bytes : gate_bytes, is_up ? up_map : gate_map,
                                          is_up ? up_offsets : gate_offsets);
    wide_block<true, XV, BF16OUT, WT>(lds, x, bm * kWideBM, M, K, ldx, st, (n0 >> 5) + (wave >> 1), n0, N, tiles_h, tiles_w, bias_gate, bias_up,
                                      act, yv, ldy, wave);
}

// packed_wide_grouped_kernel's frame with column blocks of 64 hidden columns: the plan, the slot bound, the search and the stream in
// scalar registers are that kernel's; a blob is checked against its own group's range [64 bases[e], 64 bases[e + 1]) of its OWN arena.
template <bool XV, bool BF16OUT, bool WT>
__global__ __launch_bounds__(kThreads, 2) void packed_glu_wide_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int64_t K, int64_t ldx, const int32_t *__restrict__ group_rows, const int32_t *__restrict__ bstart,
    const uint8_t *__restrict__ gate, uint64_t gate_bytes, const int8_t *__restrict__ gate_maps, const uint32_t *__restrict__ gate_offsets,
    const uint64_t *__restrict__ gate_bases, const uint8_t *__restrict__ up, uint64_t up_bytes, const int8_t *__restrict__ up_maps,
    const uint32_t *__restrict__ up_offsets, const uint64_t *__restrict__ up_bases, int count, int64_t N, int64_t tiles_h, int64_t tiles_w,
    const float *__restrict__ bias_gate, const float *__restrict__ bias_up, int64_t ldb, int act, void *__restrict__ yv, int64_t ldy)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kWideImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nblocks = (N + kGluBN - 1) / kGluBN;
    const int64_t n0 = (blockIdx.x % nblocks) * kGluBN;
    GroupBlock b;
    if (!group_block(bstart, count, (int)(blockIdx.x / nblocks), group_rows, T, lane, b)) return;   // the whole workgroup, before any barrier
    const bool is_up = wave & 1;
    const PackedStream st = arena_stream_uniform(is_up ? up : gate, is_up ? up_bytes : gate_bytes, is_up ? up_maps : gate_maps,
                                                 is_up ? up_offsets : gate_offsets, is_up ? up_bases : gate_bases, b.e, tiles_h * tiles_w);
    wide_block<true, XV, BF16OUT, WT>(lds, x, b.m0, b.M, K, ldx, st, (n0 >> 5) + (wave >> 1), n0, N, tiles_h, tiles_w,
                                      bias_gate ? bias_gate + b.e * ldb : nullptr, bias_up ? bias_up + b.e * ldb : nullptr, act, yv, ldy, wave);
}

// y[r][c] = glu_value(g[r][c], u[r][c], act): the second half of the unfused route, one thread per element in a grid-stride walk.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void glu_combine_kernel(const float *__restrict__ g, int64_t ldg, const float *__restrict__ u, int64_t ldu,
                                                          int64_t rows, int64_t cols, int act, void *__restrict__ yv, int64_t ldy)
{
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols, c = i - r * cols;
        store_y<BF16OUT>(yv, r * ldy + c, glu_value(g[r * ldg + c], u[r * ldu + c], act));
    }
}

// ---- skinny GLU (m <= 32): packed_linear_skinny_kernel's wave on one more unit axis, the projection p (0 the gate, 1 the up).
//
// A unit is (slice s, projection p, tile row tr), numbered ((2 s + p) * tiles_h + tr): the tile row is fastest, so the four waves of a
// workgroup share a slice of X as in the linear kernel.  The wave takes its projection's stream, map, offsets and bytes and does on them
// what that kernel's wave does: the readlane hand-out of up to 64 tiles per load, the ring of kSkinnyRing tiles with every load issued
// before the first decode, the blob check against its own stream's bytes, decode_skinny and two MFMAs per tile in ascending K.  Its f32
// partial always goes to ws[p][s][m][n] with plain stores, at split 1 too: no wave holds both projections, and glu_skinny_reduce_kernel
// is where they meet.  No LDS, no barrier, no atomics; the only early exit before the loads is the wave-uniform unit bound.
__global__ __launch_bounds__(64 * kSkinnyWaves) void packed_glu_skinny_kernel(
    const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec, const uint8_t *__restrict__ gate, uint64_t gate_bytes,
    const int8_t *__restrict__ gate_map, const uint32_t *__restrict__ gate_offsets, const uint8_t *__restrict__ up, uint64_t up_bytes,
    const int8_t *__restrict__ up_map, const uint32_t *__restrict__ up_offsets, int64_t N, int64_t tiles_h, int64_t tiles_w, int split,
    float *__restrict__ ws)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= 2 * tiles_h * split) return;         // wave-uniform; the kernel has no barrier
    const int64_t tr = unit % tiles_h, sp = unit / tiles_h, p = sp & 1, s = sp >> 1;
    const PackedStream st = tensor_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_map : gate_map, p ? up_offsets : gate_offsets);
    const int row = lane & 31, half = lane >> 5;

    f32x16 acc = zero16();
    skinny_run(acc, FeedDirect(), x, M, K, ldx, x_vec, st, tr * tiles_w, 1, s * tiles_w / split, (s + 1) * tiles_w / split, lane, row, half,
               2 * row + half);

    // lane's outputs are (m = (r&3) + 8(r>>2) + 4·half, n = 32·tr + row) of slice s of projection p
    const int64_t n = tr * kTile + row;
    if (n >= N) return;
    store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * M + 4 * half) * N + n, N, 0.0f);
}

// One thread per output: g = ((p0 + p1) + ... + p_{split-1}) + bias_gate over the gate's slices in ascending order from slice 0, the
// bias last, as skinny_reduce_kernel forms it; u the same from the up's slices, which lie `split` slices behind the gate's; then
// glu_value and one rounding for a bf16 Y.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void glu_skinny_reduce_kernel(const float *__restrict__ ws, int64_t MN, int64_t N, int split,
                                                                const float *__restrict__ bias_gate, const float *__restrict__ bias_up, int act,
                                                                void *__restrict__ yv, int64_t ldy)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= MN) return;
    const int64_t m = idx / N, n = idx % N;
    const float *wu = ws + (int64_t)split * MN;
    float g = ws[idx], u = wu[idx];
    for (int s = 1; s < split; ++s) g += ws[(int64_t)s * MN + idx];
    for (int s = 1; s < split; ++s) u += wu[(int64_t)s * MN + idx];
    g += bias_gate ? bias_gate[n] : 0.0f;
    u += bias_up ? bias_up[n] : 0.0f;
    store_y<BF16OUT>(yv, m * ldy + n, glu_value(g, u, act));
}

// ---- the gather of an MoE layer in a grouped skinny wave's X address (GATHER of the two grouped skinny GLU kernels below).
//
// x is the TOKEN matrix and row r of the matrix the wave multiplies is x[src[r] / topk] when 0 <= src[r] < T (T = S = tokens * topk,
// so the token is below `tokens` whatever src holds), else a row of +0: moe_dispatch_kernel's rule, and the words load_x16 hands the
// MFMAs are those it would read from the dispatched copy.  A lane looks its row's src up once per 32-row chunk and hands skinny_run
// its own row base with row 0 of M = 1 rows, or M = 0 ("no row": load_x16 returns zeros before it forms an address).  Lanes at or past
// the chunk's rows read no src.  x_vec keeps its meaning: every row starts at x + t * ldx.
struct GatherRow {
    const uint16_t *x;
    int64_t m;
};

__device__ __forceinline__ GatherRow gather_row(const uint16_t *__restrict__ x, int64_t ldx, const int32_t *__restrict__ src, int topk, int T,
                                                int64_t row0, int row, int64_t M)
{
    const int v = row < M ? src[row0 + row] : -1;    // row0 + row < r1 <= T
    const bool from = v >= 0 && v < T;
    return {x + (int64_t)(from ? v / topk : 0) * ldx, from ? 1 : 0};
}

// ---- grouped skinny GLU: packed_linear_skinny_grouped_kernel's wave on the projection axis, over two arenas.
//
// A unit is (slice s, projection p, group e, tile row tr), numbered (((2 s + p) * count + e) * tiles_h + tr).  The group's clamped rows,
// the walk in 32-row chunks by the same wave, the hand-out, ring, decode and MFMAs are that kernel's; the maps, offsets, bases and bytes
// are the wave's own arena's, and a blob is checked against its own group's range of that arena.  The partial of every chunk goes to
// ws[p][s][row][n] with plain stores at every split.
template <bool GATHER>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_glu_skinny_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const uint8_t *__restrict__ gate, uint64_t gate_bytes, const int8_t *__restrict__ gate_maps, const uint32_t *__restrict__ gate_offsets,
    const uint64_t *__restrict__ gate_bases, const uint8_t *__restrict__ up, uint64_t up_bytes, const int8_t *__restrict__ up_maps,
    const uint32_t *__restrict__ up_offsets, const uint64_t *__restrict__ up_bases, int count, int N, int tiles_h, int tiles_w, int split,
    float *__restrict__ ws, const int32_t *__restrict__ src, int topk)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)2 * tiles_h * count * split) return;   // wave-uniform; the kernel has no barrier
    const int64_t tr = unit % tiles_h, spe = unit / tiles_h, e = spe % count, sp = spe / count, p = sp & 1, s = sp >> 1;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    if (gr.r1 == gr.r0) return;                      // nothing of this expert is read
    const PackedStream st = arena_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_maps : gate_maps, p ? up_offsets : gate_offsets,
                                         p ? up_bases : gate_bases, e, (int64_t)tiles_h * tiles_w);
    const int64_t c0 = s * tiles_w / split, c1 = (s + 1) * tiles_w / split;

    for (int64_t row0 = gr.r0; row0 < gr.r1; row0 += kTile) {
        int lv = lane;
        asm volatile("" : "+v"(lv));                 // the lane's addresses are formed per chunk, not kept in registers across chunks
        const int row = lv & 31, half = lv >> 5;
        const int64_t n = tr * kTile + row;
        const int64_t M = std::min<int64_t>(kTile, gr.r1 - row0);
        f32x16 acc = zero16();
        if constexpr (GATHER) {
            const GatherRow xr = gather_row(x, ldx, src, topk, T, row0, row, M);
            skinny_run(acc, FeedDirect(), xr.x, xr.m, K, ldx, x_vec, st, tr * tiles_w, 1, c0, c1, lane, 0, half, 2 * row + half);
        } else {
            skinny_run(acc, FeedDirect(), x + row0 * ldx, M, K, ldx, x_vec, st, tr * tiles_w, 1, c0, c1, lane, row, half, 2 * row + half);
        }

        // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tr + row) of slice s of projection p
        if (n < N) store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * T + row0 + 4 * half) * N + n, N, 0.0f);
    }
}

// skinny_grouped_reduce_kernel's frame: one workgroup per (group e, 256 columns), thread n walks the group's clamped rows, so only rows
// inside a clamped group are written.  Per output glu_value(g, u) with g and u formed as glu_skinny_reduce_kernel forms them, the
// biases rows e of both bias matrices.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void glu_skinny_grouped_reduce_kernel(const float *__restrict__ ws, int64_t T, int64_t N, int split,
                                                                        const int32_t *__restrict__ group_rows, int64_t nchunks,
                                                                        const float *__restrict__ bias_gate, const float *__restrict__ bias_up,
                                                                        int64_t ldb, int act, void *__restrict__ yv, int64_t ldy)
{
    const int64_t e = blockIdx.x / nchunks, n = (blockIdx.x % nchunks) * 256 + threadIdx.x;
    if (n >= N) return;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    if (gr.r1 == gr.r0) return;
    const float bg = bias_gate ? bias_gate[e * ldb + n] : 0.0f, bu = bias_up ? bias_up[e * ldb + n] : 0.0f;
    const float *wu = ws + (int64_t)split * T * N;
    for (int64_t m = gr.r0; m < gr.r1; ++m) {
        float g = ws[m * N + n], u = wu[m * N + n];
        for (int s = 1; s < split; ++s) g += ws[((int64_t)s * T + m) * N + n];
        for (int s = 1; s < split; ++s) u += wu[((int64_t)s * T + m) * N + n];
        g += bg;
        u += bu;
        store_y<BF16OUT>(yv, m * ldy + n, glu_value(g, u, act));
    }
}

// The skinny GLU entries' workspace: both projections' partials at every split, the gate's first; never empty.
size_t glu_skinny_workspace(int64_t m, int64_t n, int split_eff)
{
    return (2 * (size_t)std::max(split_eff, 1) * (size_t)m * (size_t)n * sizeof(float) + 15) & ~(size_t)15;
}

// ---- gated skinny matmul (m <= 32): glu_value(X·P̂g + bg, X·P̂u + bu) for packed k × n gate and up matrices; the wide frames of this
// product are packed_glu_wide_kernel and packed_glu_wide_grouped_kernel with WT = true.  packed_matmul_skinny_kernel's wave on one more unit axis, the projection p (0 the gate, 1 the up): a unit is (slice s,
// projection p, tile column tc), numbered (2 s + p) * tiles_nw + tc, the tile column fastest, so the four waves of a workgroup share a
// slice of X.  The wave takes its projection's stream and tables and does what that kernel's wave does: the strided hand-out, the ring,
// the blob check against its own stream, decode_skinny, the group through one of its two wave-private [32 k][32 n] images and back as two
// B operands by the transposed read.  Its f32 partial goes to ws[p][s][m][n] with plain stores at every split; glu_skinny_reduce_kernel,
// unchanged, is where the projections meet.  Per projection the sums are packed_matmul_skinny_kernel's at the same split.
// EXEC is all ones at every transposed read: the only exit before a read is the unit bound, wave-uniform (the wave index is scalar);
// the reads sit in no lane-dependent branch; the n < N guard comes after the run.  A bad map code, a blob past its stream and k-rows at
// or past K are zeros in the image; columns at or past N are never stored.  No barrier across waves, no atomics.
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_glu_matmul_skinny_kernel(
    const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec, const uint8_t *__restrict__ gate, uint64_t gate_bytes,
    const int8_t *__restrict__ gate_map, const uint32_t *__restrict__ gate_offsets, const uint8_t *__restrict__ up, uint64_t up_bytes,
    const int8_t *__restrict__ up_map, const uint32_t *__restrict__ up_offsets, int64_t N, int64_t tiles_kh, int64_t tiles_nw, int split,
    float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= 2 * tiles_nw * split) return;        // wave-uniform; the kernel has no workgroup barrier
    const int64_t tc = unit % tiles_nw, sp = unit / tiles_nw, p = sp & 1, s = sp >> 1;
    const PackedStream st = tensor_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_map : gate_map, p ? up_offsets : gate_offsets);
    const int row = lane & 31, half = lane >> 5;

    f32x16 acc = zero16();
    skinny_run(acc, feed_transposed(lds + wave * (2 * kMmsImage), lane), x, M, K, ldx, x_vec, st, tc, tiles_nw, s * tiles_kh / split,
               (s + 1) * tiles_kh / split, lane, row, half, lane);

    // lane's outputs are (m = (r&3) + 8(r>>2) + 4·half, n = 32·tc + row) of slice s of projection p
    const int64_t n = tc * kTile + row;
    if (n >= N) return;
    store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * M + 4 * half) * N + n, N, 0.0f);
}

// Grouped skinny.  packed_matmul_skinny_grouped_kernel's wave on the projection axis, over two arenas: a unit is (slice s, projection p,
// group e, tile column tc), numbered ((2 s + p) * count + e) * tiles_nw + tc.  The group's clamped rows, the walk in 32-row chunks by the
// same wave, the run and the images are that kernel's; the tables, bases and bytes are the wave's own arena's, and a blob is checked
// against its own group's range of that arena.  The partial of every chunk goes to ws[p][s][row][n] with plain stores at every split;
// glu_skinny_grouped_reduce_kernel finishes.
// EXEC: as in packed_matmul_skinny_grouped_kernel, everything a branch before or between runs depends on (the unit bound, the group
// without rows, the chunk loop's trip count) is wave-uniform and in scalar registers; the one lane-dependent branch is the n < N guard
// around the stores, after a run, and EXEC is whole again behind it.
template <bool GATHER>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_glu_matmul_skinny_grouped_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const uint8_t *__restrict__ gate, uint64_t gate_bytes, const int8_t *__restrict__ gate_maps, const uint32_t *__restrict__ gate_offsets,
    const uint64_t *__restrict__ gate_bases, const uint8_t *__restrict__ up, uint64_t up_bytes, const int8_t *__restrict__ up_maps,
    const uint32_t *__restrict__ up_offsets, const uint64_t *__restrict__ up_bases, int count, int N, int tiles_kh, int tiles_nw, int split,
    float *__restrict__ ws, const int32_t *__restrict__ src, int topk)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)2 * tiles_nw * count * split) return;   // wave-uniform; the kernel has no workgroup barrier
    const int64_t tc = unit % tiles_nw, spe = unit / tiles_nw, e = spe % count, sp = spe / count, p = sp & 1, s = sp >> 1;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int r0 = __builtin_amdgcn_readfirstlane((int)gr.r0), r1 = __builtin_amdgcn_readfirstlane((int)gr.r1);   // 0 <= r0 <= r1 <= T
    if (r1 == r0) return;                            // nothing of this expert is read
    const PackedStream st = arena_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_maps : gate_maps, p ? up_offsets : gate_offsets,
                                         p ? up_bases : gate_bases, e, (int64_t)tiles_kh * tiles_nw);
    const int64_t c0 = s * tiles_kh / split, c1 = (s + 1) * tiles_kh / split;
    uint16_t *img = lds + wave * (2 * kMmsImage);

    for (int64_t row0 = r0; row0 < r1; row0 += kTile) {   // scalar: the trip count is the group's
        int lv = lane;
        asm volatile("" : "+v"(lv));                 // the lane's addresses are formed per chunk, not kept in registers across chunks
        const int row = lv & 31, half = lv >> 5;
        const int64_t n = tc * kTile + row;
        const int64_t M = std::min<int64_t>(kTile, r1 - row0);
        f32x16 acc = zero16();
        if constexpr (GATHER) {
            const GatherRow xr = gather_row(x, ldx, src, topk, T, row0, row, M);
            skinny_run(acc, feed_transposed(img, lv), xr.x, xr.m, K, ldx, x_vec, st, tc, tiles_nw, c0, c1, lane, 0, half, lv);
        } else {
            skinny_run(acc, feed_transposed(img, lv), x + row0 * ldx, M, K, ldx, x_vec, st, tc, tiles_nw, c0, c1, lane, row, half, lv);
        }

        // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tc + row) of slice s of projection p
        if (n < N) store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * T + row0 + 4 * half) * N + n, N, 0.0f);
    }
}

// ---- grouped skinny GLU, a wave per 32-row chunk: packed_glu_skinny_grouped_kernel's wave on packed_linear_skinny_grouped_chunked_kernel's
// frame.
//
// A unit is (slice s, projection p, chunk slot c, tile row tr), numbered (((2 s + p) * slots + c) * tiles_h + tr): the four waves of a
// workgroup share a slice, a projection and, but for a seam, a chunk's rows of X.  cstart is packed_grouped_plan_kernel<32>'s prefix on
// the same stream, slots the host's bound on cstart[count]; a wave whose slot is at or past cstart[count] returns before any other load,
// the group comes from group_of_slot and row0 = r0 + 32 (c - cstart[e]).  On its chunk the wave does the body of the walking kernel's
// `for row0` loop: the same arena_stream of its projection's arena, the same skinny_run arguments (gather_row as it stands with GATHER),
// the same store_lane_rows into ws[p][s][row][n] at every split - that kernel's partials, bit for bit, for nondecreasing group_rows.
template <bool GATHER>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_glu_skinny_grouped_chunked_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const int32_t *__restrict__ cstart, int slots, const uint8_t *__restrict__ gate, uint64_t gate_bytes, const int8_t *__restrict__ gate_maps,
    const uint32_t *__restrict__ gate_offsets, const uint64_t *__restrict__ gate_bases, const uint8_t *__restrict__ up, uint64_t up_bytes,
    const int8_t *__restrict__ up_maps, const uint32_t *__restrict__ up_offsets, const uint64_t *__restrict__ up_bases, int count, int N,
    int tiles_h, int tiles_w, int split, float *__restrict__ ws, const int32_t *__restrict__ src, int topk)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)2 * tiles_h * slots * split) return;   // wave-uniform; the kernel has no barrier
    const int64_t tr = unit % tiles_h, spc = unit / tiles_h, sp = spc / slots, p = sp & 1, s = sp >> 1;
    const int c = (int)(spc % slots);
    if (c >= cstart[count]) return;                  // a surplus slot: nothing else is read
    const int e = group_of_slot(cstart, count, c, lane);
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int64_t row0 = gr.r0 + (int64_t)(c - cstart[e]) * kTile;
    if (row0 >= gr.r1) return;                       // never for a prefix this launch's plan kernel wrote
    const PackedStream st = arena_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_maps : gate_maps, p ? up_offsets : gate_offsets,
                                         p ? up_bases : gate_bases, e, (int64_t)tiles_h * tiles_w);
    const int64_t c0 = s * tiles_w / split, c1 = (s + 1) * tiles_w / split;

    const int row = lane & 31, half = lane >> 5;
    const int64_t n = tr * kTile + row;
    const int64_t M = std::min<int64_t>(kTile, gr.r1 - row0);
    f32x16 acc = zero16();
    if constexpr (GATHER) {
        const GatherRow xr = gather_row(x, ldx, src, topk, T, row0, row, M);
        skinny_run(acc, FeedDirect(), xr.x, xr.m, K, ldx, x_vec, st, tr * tiles_w, 1, c0, c1, lane, 0, half, 2 * row + half);
    } else {
        skinny_run(acc, FeedDirect(), x + row0 * ldx, M, K, ldx, x_vec, st, tr * tiles_w, 1, c0, c1, lane, row, half, 2 * row + half);
    }

    // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tr + row) of slice s of projection p
    if (n >= N) return;
    store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * T + row0 + 4 * half) * N + n, N, 0.0f);
}

// The (k, n) twin on packed_matmul_skinny_grouped_chunked_kernel's frame: a unit is (slice s, projection p, chunk slot c, tile column tc),
// numbered (((2 s + p) * slots + c) * tiles_nw + tc), the run goes through the wave's two [32 k][32 n] images (feed_transposed).
// EXEC: packed_matmul_skinny_grouped_chunked_kernel's rule.  Every branch before the run - the unit bound, the surplus slot,
// row0 >= r1 - is wave-uniform: the wave index, the group, its clamped rows and row0 go through readfirstlane.  gather_row's src load is
// a select on the lane's row, not a branch around the run; the one lane-dependent branch is the n < N guard after the run.
template <bool GATHER>
__global__ __launch_bounds__(64 * kSkinnyWaves, 2) void packed_glu_matmul_skinny_grouped_chunked_kernel(
    const uint16_t *__restrict__ x, int T, int K, int64_t ldx, int x_vec, const int32_t *__restrict__ group_rows,
    const int32_t *__restrict__ cstart, int slots, const uint8_t *__restrict__ gate, uint64_t gate_bytes, const int8_t *__restrict__ gate_maps,
    const uint32_t *__restrict__ gate_offsets, const uint64_t *__restrict__ gate_bases, const uint8_t *__restrict__ up, uint64_t up_bytes,
    const int8_t *__restrict__ up_maps, const uint32_t *__restrict__ up_offsets, const uint64_t *__restrict__ up_bases, int count, int N,
    int tiles_kh, int tiles_nw, int split, float *__restrict__ ws, const int32_t *__restrict__ src, int topk)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[kSkinnyWaves * 2 * kMmsImage];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit = (int64_t)blockIdx.x * kSkinnyWaves + wave;
    if (unit >= (int64_t)2 * tiles_nw * slots * split) return;   // wave-uniform; the kernel has no workgroup barrier
    const int64_t tc = unit % tiles_nw, spc = unit / tiles_nw, sp = spc / slots, p = sp & 1, s = sp >> 1;
    const int c = (int)(spc % slots);
    if (c >= cstart[count]) return;                  // a surplus slot: nothing else is read
    const int e = __builtin_amdgcn_readfirstlane(group_of_slot(cstart, count, c, lane));
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int r1 = __builtin_amdgcn_readfirstlane((int)gr.r1);
    const int64_t row0 = __builtin_amdgcn_readfirstlane((int)gr.r0) + (int64_t)(c - __builtin_amdgcn_readfirstlane(cstart[e])) * kTile;
    if (row0 >= r1) return;                          // never for a prefix this launch's plan kernel wrote
    const PackedStream st = arena_stream(p ? up : gate, p ? up_bytes : gate_bytes, p ? up_maps : gate_maps, p ? up_offsets : gate_offsets,
                                         p ? up_bases : gate_bases, e, (int64_t)tiles_kh * tiles_nw);
    const int64_t c0 = s * tiles_kh / split, c1 = (s + 1) * tiles_kh / split;

    const int row = lane & 31, half = lane >> 5;
    const int64_t n = tc * kTile + row;
    const int64_t M = std::min<int64_t>(kTile, r1 - row0);
    f32x16 acc = zero16();
    const FeedTransposed feed = feed_transposed(lds + wave * (2 * kMmsImage), lane);
    if constexpr (GATHER) {
        const GatherRow xr = gather_row(x, ldx, src, topk, T, row0, row, M);
        skinny_run(acc, feed, xr.x, xr.m, K, ldx, x_vec, st, tc, tiles_nw, c0, c1, lane, 0, half, lane);
    } else {
        skinny_run(acc, feed, x + row0 * ldx, M, K, ldx, x_vec, st, tc, tiles_nw, c0, c1, lane, row, half, lane);
    }

    // lane's outputs are (row0 + (r&3) + 8(r>>2) + 4·half, n = 32·tc + row) of slice s of projection p
    if (n >= N) return;
    store_lane_rows<false, true>(acc, M, half, ws, (((int64_t)p * split + s) * T + row0 + 4 * half) * N + n, N, 0.0f);
}

// The reduce over chunk slots: one workgroup per (chunk slot c, 256 columns), thread n walks the chunk's at most 32 rows, so a hot
// group's rows are spread over its chunks' workgroups where glu_skinny_grouped_reduce_kernel gives them all to one thread per column.
// The slot's group is the main kernel's (group_of_slot on the same cstart, by every wave of the workgroup alike, before the column
// guard: the search's ballot wants the whole wave).  g, u and glu_value are formed as that kernel forms them - slices ascending, bias
// last - and an output depends on its own row and column alone: that kernel's bits.  Only rows inside a clamped group are written.
template <bool BF16OUT>
__global__ __launch_bounds__(256) void glu_skinny_grouped_chunked_reduce_kernel(const float *__restrict__ ws, int64_t T, int64_t N, int split,
                                                                                const int32_t *__restrict__ group_rows,
                                                                                const int32_t *__restrict__ cstart, int count, int64_t nchunks,
                                                                                const float *__restrict__ bias_gate,
                                                                                const float *__restrict__ bias_up, int64_t ldb, int act,
                                                                                void *__restrict__ yv, int64_t ldy)
{
    const int c = (int)(blockIdx.x / nchunks);
    const int64_t n = (blockIdx.x % nchunks) * 256 + threadIdx.x;
    if (c >= cstart[count]) return;                  // a surplus slot, the whole workgroup
    const int e = group_of_slot(cstart, count, c, threadIdx.x & 63);
    if (n >= N) return;
    const GroupRows gr = group_rows_of(group_rows, e, T);
    const int64_t row0 = gr.r0 + (int64_t)(c - cstart[e]) * kTile, row1 = std::min<int64_t>(row0 + kTile, gr.r1);
    const float bg = bias_gate ? bias_gate[e * ldb + n] : 0.0f, bu = bias_up ? bias_up[e * ldb + n] : 0.0f;
    const float *wu = ws + (int64_t)split * T * N;
    for (int64_t m = row0; m < row1; ++m) {
        float g = ws[m * N + n], u = wu[m * N + n];
        for (int s = 1; s < split; ++s) g += ws[((int64_t)s * T + m) * N + n];
        for (int s = 1; s < split; ++s) u += wu[((int64_t)s * T + m) * N + n];
        g += bg;
        u += bu;
        store_y<BF16OUT>(yv, m * ldy + n, glu_value(g, u, act));
    }
}

// skinny_shape for the grouped entry: skinny_split's rule with count * tiles_h tile rows, which for count == 1 is that rule.
int grouped_shape(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split, int64_t *tiles_h, int64_t *tiles_w, int *split_eff)
{
    if (total_rows <= 0) return fail(MTQ_ERR_INVALID, "total_rows must be positive (empty operands are handled by the caller)");
    if (total_rows > INT32_MAX) return fail(MTQ_ERR_INVALID, "total_rows does not fit the 32-bit group_rows");
    if (count <= 0) return fail(MTQ_ERR_INVALID, "count must be positive");
    if (count > INT32_MAX) return fail(MTQ_ERR_INVALID, "count does not fit 32 bits");
    if (split < 0) return fail(MTQ_ERR_INVALID, "split must not be negative (0: the library's choice)");
    if (int rc = tile_grid(n, k, tiles_h, tiles_w)) return rc;
    if (*tiles_h * *tiles_w > MTQ_PACKED_BATCH_MAX_TILES) return fail(MTQ_ERR_INVALID, "too many tiles: a tensor's stream must fit 32-bit units");
    if (count > ((int64_t)1 << 40) / (*tiles_h * *tiles_w)) return fail(MTQ_ERR_INVALID, "too many tiles in the batch");
    const int64_t own = std::max<int64_t>(1, std::min(kSkinnyUnits / (count * *tiles_h), *tiles_w / kSkinnyMinRun));
    *split_eff = (int)std::min<int64_t>(split == 0 ? own : split, *tiles_w);
    if (*split_eff > 1 && total_rows > ((int64_t)1 << 56) / n / *split_eff) return fail(MTQ_ERR_INVALID, "the workspace of this split is too large");
    return MTQ_OK;
}

int tile_grid(int64_t rows, int64_t cols, int64_t *tiles_h, int64_t *tiles_w)
{
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty tensors are handled by the caller)");
    if (rows > (int64_t)1 << 30 || cols > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    *tiles_h = (rows + kTile - 1) / kTile;
    *tiles_w = (cols + kTile - 1) / kTile;
    if (*tiles_h * *tiles_w > (int64_t)1 << 31) return fail(MTQ_ERR_INVALID, "too many tiles for 32-bit offsets");
    return MTQ_OK;
}

unsigned tile_blocks(int64_t tiles) { return (unsigned)std::min<int64_t>((tiles + 3) / 4, (int64_t)1 << 20); }

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_packed_tile_bytes(int fmt) { return packed_tile_bytes(fmt); }

extern "C" int mtq_packed_offsets(const int8_t *map, int64_t tiles, uint32_t *offsets)
{
    if (!map || !offsets) return fail(MTQ_ERR_INVALID, "null argument");
    if (tiles <= 0) return fail(MTQ_ERR_INVALID, "tiles must be positive");
    uint64_t units = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        const uint32_t size = packed_tile_bytes(map[t]);
        if (size == 0u) return failf(MTQ_ERR_INVALID, "map[%lld] = %d is no packed format (codes 0..3: bf16, bfp8, bfp4, bfp2)", (long long)t, (int)map[t]);
        offsets[t] = (uint32_t)units;
        units += size / kUnit;
        if (units > UINT32_MAX) return fail(MTQ_ERR_INVALID, "the stream is too long for 32-bit offsets in units of 64 bytes");
    }
    offsets[tiles] = (uint32_t)units;
    return MTQ_OK;
}

// ---- the checks that several entries word alike, each text in one place

static const char *const kNullArg = "null argument";

static int dtype_arg(int dtype, const char *name)
{
    if (dtype != MTQ_DTYPE_BF16 && dtype != MTQ_DTYPE_F32) return failf(MTQ_ERR_INVALID, "%s must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32", name);
    return MTQ_OK;
}

static int aligned_arg(const void *p, const char *name)
{
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return failf(MTQ_ERR_INVALID, "%s must be 16-byte aligned", name);
    return MTQ_OK;
}

// A buffer of `tiles` tiles is at least as long as their bfp2 blobs; `plural`: the streams of a batch or an arena
static int stream_bytes_arg(size_t bytes, int64_t tiles, const char *name, bool plural)
{
    if (bytes < (uint64_t)tiles * packed_tile_bytes(MTQ_FMT_BFP2))
        return failf(MTQ_ERR_INVALID, "%s_bytes is smaller than the stream%s", name, plural ? "s" : "");
    return MTQ_OK;
}

// What the batched entries share: the tile grid of one matrix and the batch's tile total
static int batch_grid(int64_t count, int64_t rows, int64_t cols, int64_t *tiles_h, int64_t *tiles_w)
{
    if (count <= 0) return fail(MTQ_ERR_INVALID, "count must be positive");
    if (int rc = tile_grid(rows, cols, tiles_h, tiles_w)) return rc;
    if (*tiles_h * *tiles_w > MTQ_PACKED_BATCH_MAX_TILES) return fail(MTQ_ERR_INVALID, "too many tiles: a tensor's stream must fit 32-bit units");
    if (count > ((int64_t)1 << 40) / (*tiles_h * *tiles_w)) return fail(MTQ_ERR_INVALID, "too many tiles in the batch");
    return MTQ_OK;
}

// A matrix of the batch must not reach into the next: stride 0 is allowed for a batch of one only
static int batch_pitch(int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride, const char *ld_msg)
{
    if (ld < cols) return fail(MTQ_ERR_INVALID, ld_msg);
    if (count > 1 && stride < (rows - 1) * ld + cols) return fail(MTQ_ERR_INVALID, "the matrix stride is smaller than a matrix");
    return MTQ_OK;
}

// ---- pack / unpack.  The argument block of the eight entries, checked in the one order they all report in, down to the device: the
// pointers, the matrix's type, the grid, the pitches, then the stream.  A pack entry names its matrix side in_dtype / ld and its stream
// out, an unpack entry out_dtype / ldy and packed.  kTransposed: the matrix (rows × cols, pitch ld) is in the stored orientation, the
// stream, its maps, offsets and the grid *th × *tw are those of the cols × rows transpose.  kBatched: count matrices `stride` elements
// apart and an arena of their streams; without it the entry passes count 1 and stride 0.
enum : unsigned { kUnpack = 0, kPack = 1, kTransposed = 2, kBatched = 4 };

static int tiles_args(unsigned entry, bool any_null, int dtype, int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
                      const void *stream_buf, size_t stream_bytes, int64_t *th, int64_t *tw)
{
    const bool pack = entry & kPack, batched = entry & kBatched;
    if (any_null) return fail(MTQ_ERR_INVALID, kNullArg);
    if (int rc = dtype_arg(dtype, pack ? "in_dtype" : "out_dtype")) return rc;
    const int64_t grid_rows = entry & kTransposed ? cols : rows, grid_cols = entry & kTransposed ? rows : cols;
    if (int rc = batched ? batch_grid(count, grid_rows, grid_cols, th, tw) : tile_grid(grid_rows, grid_cols, th, tw)) return rc;
    if (int rc = batch_pitch(count, rows, cols, ld, stride, pack ? "ld < cols" : "ldy < cols")) return rc;
    if (int rc = aligned_arg(stream_buf, pack ? "out" : "packed")) return rc;
    if (int rc = stream_bytes_arg(stream_bytes, count * *th * *tw, pack ? "out" : "packed", batched)) return rc;
    return require_device();
}

// whole 16-byte pieces of a matrix's rows: the base, the row pitch and, between the matrices of a batch, the stride
static int tiles_vec_ok(const void *p, int dtype, int64_t ld, int64_t count, int64_t stride)
{
    const int64_t esz = dtype == MTQ_DTYPE_F32 ? 4 : 2;
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * esz) % 16 == 0 && (count == 1 || (stride * esz) % 16 == 0);
}

extern "C" int mtq_pack_tiles(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld, const int8_t *map, const uint32_t *offsets,
                              void *out, size_t out_bytes, void *stream)
{
    int64_t th, tw;
    if (int rc = tiles_args(kPack, !x || !map || !offsets || !out, in_dtype, 1, rows, cols, ld, 0, out, out_bytes, &th, &tw)) return rc;
    const int vec_ok = tiles_vec_ok(x, in_dtype, ld, 1, 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(th * tw));
    if (in_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(pack_tiles_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(x), rows, cols, ld, vec_ok, map, offsets,
                           th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    else
        hipLaunchKernelGGL(pack_tiles_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), rows, cols, ld, vec_ok, map, offsets,
                           th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    return check_launch("mtq_pack_tiles");
}

extern "C" int mtq_unpack_tiles(const void *packed, size_t packed_bytes, const int8_t *map, const uint32_t *offsets, int64_t rows, int64_t cols,
                                void *y, int out_dtype, int64_t ldy, void *stream)
{
    int64_t th, tw;
    if (int rc = tiles_args(kUnpack, !packed || !map || !offsets || !y, out_dtype, 1, rows, cols, ldy, 0, packed, packed_bytes, &th, &tw)) return rc;
    const int vec_ok = tiles_vec_ok(y, out_dtype, ldy, 1, 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(th * tw));
    const uint8_t *pp = static_cast<const uint8_t *>(packed);
    if (out_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(unpack_tiles_kernel<true>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, map, offsets, th * tw, tw, rows, cols, y, ldy, vec_ok);
    else
        hipLaunchKernelGGL(unpack_tiles_kernel<false>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, map, offsets, th * tw, tw, rows, cols, y, ldy, vec_ok);
    return check_launch("mtq_unpack_tiles");
}

// The transposed pair: w / y in the stored orientation (rows × cols), the stream that of the cols × rows transpose.
extern "C" int mtq_pack_tiles_transposed(const void *w, int in_dtype, int64_t rows, int64_t cols, int64_t ld, const int8_t *map,
                                         const uint32_t *offsets, void *out, size_t out_bytes, void *stream)
{
    int64_t th, tw;                                   // of the transpose
    if (int rc = tiles_args(kPack | kTransposed, !w || !map || !offsets || !out, in_dtype, 1, rows, cols, ld, 0, out, out_bytes, &th, &tw)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(th * tw));
    if (in_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(pack_tiles_transposed_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(w), rows, cols, ld, map, offsets,
                           th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    else
        hipLaunchKernelGGL(pack_tiles_transposed_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(w), rows, cols, ld, map,
                           offsets, th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    return check_launch("mtq_pack_tiles_transposed");
}

extern "C" int mtq_unpack_tiles_transposed(const void *packed, size_t packed_bytes, const int8_t *map, const uint32_t *offsets, int64_t rows,
                                           int64_t cols, void *y, int out_dtype, int64_t ldy, void *stream)
{
    int64_t th, tw;                                   // of the transpose
    if (int rc = tiles_args(kUnpack | kTransposed, !packed || !map || !offsets || !y, out_dtype, 1, rows, cols, ldy, 0, packed, packed_bytes, &th, &tw))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(th * tw));
    const uint8_t *pp = static_cast<const uint8_t *>(packed);
    if (out_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(unpack_tiles_transposed_kernel<true>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, map, offsets, th * tw, tw, rows, cols, y, ldy);
    else
        hipLaunchKernelGGL(unpack_tiles_transposed_kernel<false>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, map, offsets, th * tw, tw, rows, cols, y, ldy);
    return check_launch("mtq_unpack_tiles_transposed");
}

extern "C" int mtq_packed_offsets_batched(const int8_t *maps, int64_t count, int64_t tiles, uint32_t *offsets, uint64_t *bases, int32_t *bad,
                                          void *stream)
{
    if (!maps || !offsets || !bases || !bad) return fail(MTQ_ERR_INVALID, kNullArg);
    if (count <= 0) return fail(MTQ_ERR_INVALID, "count must be positive");
    if (tiles <= 0) return fail(MTQ_ERR_INVALID, "tiles must be positive");
    if (tiles > MTQ_PACKED_BATCH_MAX_TILES) return fail(MTQ_ERR_INVALID, "too many tiles: a tensor's stream must fit 32-bit units");
    if (count > ((int64_t)1 << 40) / tiles) return fail(MTQ_ERR_INVALID, "too many tiles in the batch");
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)std::min<int64_t>(count, (int64_t)1 << 20));
    hipLaunchKernelGGL(packed_offsets_batched_kernel, grid, dim3(256), 0, st, maps, count, tiles, offsets, bad);
    if (int rc = check_launch("mtq_packed_offsets_batched")) return rc;
    hipLaunchKernelGGL(packed_bases_kernel, dim3(1), dim3(256), 0, st, offsets, count, tiles, bases);
    return check_launch("mtq_packed_offsets_batched");
}

extern "C" int mtq_pack_tiles_batched(const void *x, int in_dtype, int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
                                      const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, void *out, size_t out_bytes, void *stream)
{
    int64_t th, tw;
    if (int rc = tiles_args(kPack | kBatched, !x || !maps || !offsets || !bases || !out, in_dtype, count, rows, cols, ld, stride, out, out_bytes, &th,
                            &tw))
        return rc;
    const int vec_ok = tiles_vec_ok(x, in_dtype, ld, count, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(count * th * tw));
    if (in_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(pack_tiles_batched_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(x), count, rows, cols, ld, stride, vec_ok,
                           maps, offsets, bases, th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    else
        hipLaunchKernelGGL(pack_tiles_batched_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(x), count, rows, cols, ld, stride,
                           vec_ok, maps, offsets, bases, th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    return check_launch("mtq_pack_tiles_batched");
}

extern "C" int mtq_unpack_tiles_batched(const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                        int64_t count, int64_t rows, int64_t cols, void *y, int out_dtype, int64_t ldy, int64_t stride, void *stream)
{
    int64_t th, tw;
    if (int rc = tiles_args(kUnpack | kBatched, !packed || !maps || !offsets || !bases || !y, out_dtype, count, rows, cols, ldy, stride, packed,
                            packed_bytes, &th, &tw))
        return rc;
    const int vec_ok = tiles_vec_ok(y, out_dtype, ldy, count, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(count * th * tw));
    const uint8_t *pp = static_cast<const uint8_t *>(packed);
    if (out_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(unpack_tiles_batched_kernel<true>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, maps, offsets, bases, count, th * tw, tw,
                           rows, cols, y, ldy, stride, vec_ok);
    else
        hipLaunchKernelGGL(unpack_tiles_batched_kernel<false>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, maps, offsets, bases, count, th * tw, tw,
                           rows, cols, y, ldy, stride, vec_ok);
    return check_launch("mtq_unpack_tiles_batched");
}

// The batched transposed pair: w / y hold `count` matrices in the stored orientation (rows × cols), the arena the streams of their
// cols × rows transposes; maps, offsets and the grid are the transposes'.
extern "C" int mtq_pack_tiles_transposed_batched(const void *w, int in_dtype, int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
                                                 const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, void *out, size_t out_bytes,
                                                 void *stream)
{
    int64_t th, tw;                                   // of the transpose
    if (int rc = tiles_args(kPack | kTransposed | kBatched, !w || !maps || !offsets || !bases || !out, in_dtype, count, rows, cols, ld, stride, out,
                            out_bytes, &th, &tw))
        return rc;
    const int vec_ok = tiles_vec_ok(w, in_dtype, ld, count, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(count * th * tw));
    if (in_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(pack_tiles_transposed_batched_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(w), count, rows, cols, ld,
                           stride, vec_ok, maps, offsets, bases, th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    else
        hipLaunchKernelGGL(pack_tiles_transposed_batched_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(w), count, rows, cols,
                           ld, stride, vec_ok, maps, offsets, bases, th * tw, tw, static_cast<uint8_t *>(out), (uint64_t)out_bytes);
    return check_launch("mtq_pack_tiles_transposed_batched");
}

extern "C" int mtq_unpack_tiles_transposed_batched(const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                   const uint64_t *bases, int64_t count, int64_t rows, int64_t cols, void *y, int out_dtype,
                                                   int64_t ldy, int64_t stride, void *stream)
{
    int64_t th, tw;                                   // of the transpose
    if (int rc = tiles_args(kUnpack | kTransposed | kBatched, !packed || !maps || !offsets || !bases || !y, out_dtype, count, rows, cols, ldy, stride,
                            packed, packed_bytes, &th, &tw))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tile_blocks(count * th * tw));
    const uint8_t *pp = static_cast<const uint8_t *>(packed);
    if (out_dtype == MTQ_DTYPE_BF16)
        hipLaunchKernelGGL(unpack_tiles_transposed_batched_kernel<true>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, maps, offsets, bases, count,
                           th * tw, tw, rows, cols, y, ldy, stride);
    else
        hipLaunchKernelGGL(unpack_tiles_transposed_batched_kernel<false>, grid, dim3(256), 0, st, pp, (uint64_t)packed_bytes, maps, offsets, bases, count,
                           th * tw, tw, rows, cols, y, ldy, stride);
    return check_launch("mtq_unpack_tiles_transposed_batched");
}

// ---- products.  Every entry for an (n, k) weight has a twin for a (k, n) matrix with the same arguments, checks, workspaces and texts:
// a pair is ONE body below, which takes the orientation `kn` and the entry's name for check_launch, and the extern "C" entries forward
// to it.  What kn changes is the kernel and which way round the kernel takes the tile grid: the checks form the grid of n × k (tile_grid
// of n × k is the grid check of k × n), a kernel wants the grid of the stream as it was packed (TileGrid::sh / sw).
struct TileGrid {
    int64_t th, tw;                                  // the tile grid of one weight: th tiles along n, tw tiles along k
    int eff;                                         // the effective split (the split entries)
    int64_t sh(bool kn) const { return kn ? tw : th; }   // the stream's own grid, sh × sw
    int64_t sw(bool kn) const { return kn ? th : tw; }
};

// One launch of the instantiation that stores a bf16 Y (kt) or an f32 Y (kf)
template <typename... P, typename... A>
static void launch_out(int out_dtype, void (*kt)(P...), void (*kf)(P...), dim3 grid, dim3 block, hipStream_t st, A... args)
{
    hipLaunchKernelGGL(out_dtype == MTQ_DTYPE_BF16 ? kt : kf, grid, block, 0, st, args...);
}

// launch_out's two kernels: <BF16OUT> of a twin pair's kernel templates for the orientation ...
#define MTQ_TWIN_PAIR(kn, linear, matmul) (kn) ? matmul<true> : linear<true>, (kn) ? matmul<false> : linear<false>

// ... and kernel<XV, BF16OUT, WT> of a wide kernel template for (x_vec, out_dtype, kn)
#define MTQ_WIDE_OF(kernel, x_vec, out, kn)                                                                                                          \
    ((kn) ? ((x_vec) ? kernel<true, out, true> : kernel<false, out, true>) : ((x_vec) ? kernel<true, out, false> : kernel<false, out, false>))
#define MTQ_WIDE_PAIR(kernel, x_vec, kn) MTQ_WIDE_OF(kernel, x_vec, true, kn), MTQ_WIDE_OF(kernel, x_vec, false, kn)

// whole pieces of 8 bf16 of x by 16-byte loads: every row aligned (a group may start at any row).  The wide kernels also want k % 8 == 0
// and take any other x (a ragged k included) element by element.
static bool x_vec_of(const void *x, int64_t ldx) { return reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0; }
static bool x_vec_wide(const void *x, int64_t ldx, int64_t k) { return x_vec_of(x, ldx) && k % 8 == 0; }

// No dimension of a grid may pass INT32_MAX.  The entries without a workspace say what the caller can do about it.
static int grid_args(std::initializer_list<int64_t> dims, bool m_in_chunks = false)
{
    for (const int64_t d : dims)
        if (d > INT32_MAX)
            return fail(MTQ_ERR_INVALID, m_in_chunks ? "too many workgroups for one launch: pass M in chunks" : "too many workgroups for one launch");
    return MTQ_OK;
}

// What the block and the wide entries check before a device is looked for, and the tile grid
static int linear_args(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                       const uint32_t *offsets, int64_t n, const void *y, int out_dtype, int64_t ldy, TileGrid &g)
{
    if (!x || !packed || !map || !offsets || !y) return fail(MTQ_ERR_INVALID, kNullArg);
    if (int rc = dtype_arg(out_dtype, "out_dtype")) return rc;
    if (m <= 0) return fail(MTQ_ERR_INVALID, "m must be positive (empty operands are handled by the caller)");
    if (int rc = tile_grid(n, k, &g.th, &g.tw)) return rc;
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldy < n) return fail(MTQ_ERR_INVALID, "ldy < n");
    if (m > (int64_t)1 << 40) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (int rc = aligned_arg(packed, "packed")) return rc;
    return stream_bytes_arg(packed_bytes, g.th * g.tw, "packed", false);
}

// The argument block of the skinny, grouped and wide-grouped entries, checked in the one order they all report in: the pointers, the
// output type, the entry's shape rule (skinny_shape, grouped_shape, glu_grouped_shape: it fills g), the pitches, then the streams.
// count == 0: a single tensor, else an arena of count; a gated entry passes both streams, any other its one stream twice.
struct StreamArg {
    const void *packed;
    size_t bytes;
};

template <typename Shape>
static int gemm_args(bool any_null, int out_dtype, Shape shape, TileGrid &g, int64_t k, int64_t ldx, int64_t n, int64_t ldy, bool bias_rows,
                     int64_t ldb, int64_t count, StreamArg a, StreamArg b)
{
    if (any_null) return fail(MTQ_ERR_INVALID, kNullArg);
    if (int rc = dtype_arg(out_dtype, "out_dtype")) return rc;
    if (int rc = shape(g)) return rc;
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldy < n) return fail(MTQ_ERR_INVALID, "ldy < n");
    if (bias_rows && count > 1 && ldb < n) return fail(MTQ_ERR_INVALID, "ldb < n");
    if (int rc = aligned_arg(a.packed, "packed")) return rc;
    if (int rc = aligned_arg(b.packed, "packed")) return rc;
    return stream_bytes_arg(std::min(a.bytes, b.bytes), std::max<int64_t>(count, 1) * g.th * g.tw, "packed", count != 0);
}

// The workspace block: need == 0 asks for none; null_msg says why this entry needs one, `whose` is "split" or "call"
static int workspace_args(const void *workspace, size_t workspace_bytes, size_t need, const char *null_msg, const char *whose)
{
    if (need == 0) return MTQ_OK;
    if (!workspace) return fail(MTQ_ERR_INVALID, null_msg);
    if (int rc = aligned_arg(workspace, "workspace")) return rc;
    if (workspace_bytes < need)
        return failf(MTQ_ERR_INVALID, "workspace_bytes %zu is smaller than the %zu bytes this %s needs", workspace_bytes, need, whose);
    return MTQ_OK;
}

static const char *const kWsSplit = "workspace is null and this split needs one";
static const char *const kWsPlan = "workspace is null and the block plan needs one";
static const char *const kWsChunks = "workspace is null and the chunk plan needs one at every split";
static const char *const kWsGlu = "workspace is null: the partial sums of both projections need one at every split";

// The grouped entries' plan region: start[0 .. count] as int32 at the head of the workspace, rounded to 16 so that the f32 partials
// behind it keep the workspace's alignment.  A function of count alone.
static size_t grouped_plan_bytes(int64_t count)
{
    return (((size_t)count + 1) * sizeof(int32_t) + 15) & ~(size_t)15;
}

// The plan's slot bound for pieces of `rows` rows (32-row chunks, 128-row blocks), formed from (total_rows, count) alone: every piece
// of disjoint groups has a slot, since a group with rows adds at most (rows - 1) / rows of a piece over its own rows / rows.
static int64_t grouped_slots(int64_t total_rows, int64_t count, int64_t rows)
{
    return (total_rows + (rows - 1) * std::min(count, total_rows)) / rows;
}

// The plan on the stream, before the kernel that searches it
template <int ROWS>
static int launch_plan(const char *name, hipStream_t st, const int32_t *group_rows, int64_t count, int64_t total_rows, int32_t *start)
{
    hipLaunchKernelGGL(packed_grouped_plan_kernel<ROWS>, dim3(1), dim3(256), 0, st, group_rows, (int)count, (int)total_rows, start);
    return check_launch(name);
}

// The grouped reduces walk a group's columns in chunks of 256: count × grouped_nchunks(n) workgroups
static int64_t grouped_nchunks(int64_t n) { return (n + 255) / 256; }

// mtq_moe_plan's limits on (tokens, topk), for the entries that take a plan's src or row_of; *slots = S = tokens * topk
static int moe_slots_arg(int64_t tokens, int64_t topk, int64_t *slots)
{
    if (tokens <= 0) return fail(MTQ_ERR_INVALID, "tokens must be positive");
    if (topk <= 0 || topk > MTQ_MOE_MAX_TOPK) return fail(MTQ_ERR_INVALID, "topk must be 1 .. MTQ_MOE_MAX_TOPK (64)");
    if (tokens > (((int64_t)1 << 31) - 1) / topk) return fail(MTQ_ERR_INVALID, "tokens * topk must be below 2^31");
    *slots = tokens * topk;
    return MTQ_OK;
}

// 1. block
static int packed_block(bool kn, const char *name, const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes,
                        const int8_t *map, const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    TileGrid g;
    if (int rc = linear_args(x, m, k, ldx, packed, packed_bytes, map, offsets, n, y, out_dtype, ldy, g)) return rc;
    const int64_t blocks = ((m + kBM - 1) / kBM) * ((n + kBN - 1) / kBN);
    if (int rc = grid_args({blocks}, true)) return rc;
    if (int rc = require_device()) return rc;
    launch_out(out_dtype, MTQ_TWIN_PAIR(kn, packed_linear_kernel, packed_matmul_kernel), dim3((unsigned)blocks), dim3(kThreads),
               static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(x), m, k, ldx, (int)x_vec_of(x, ldx),
               static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, map, offsets, n, g.sh(kn), g.sw(kn), bias, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_linear(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                 const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_block(false, "mtq_packed_linear", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream);
}

extern "C" int mtq_packed_matmul(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                 const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_block(true, "mtq_packed_matmul", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream);
}

// 2. wide
static int packed_wide(bool kn, const char *name, const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes,
                       const int8_t *map, const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    TileGrid g;
    if (int rc = linear_args(x, m, k, ldx, packed, packed_bytes, map, offsets, n, y, out_dtype, ldy, g)) return rc;
    const int64_t blocks = ((m + kWideBM - 1) / kWideBM) * ((n + kWideBN - 1) / kWideBN);
    if (int rc = grid_args({blocks}, true)) return rc;
    if (int rc = require_device()) return rc;
    const bool x_vec = x_vec_wide(x, ldx, k);
    launch_out(out_dtype, MTQ_WIDE_PAIR(packed_wide_kernel, x_vec, kn), dim3((unsigned)blocks), dim3(kThreads), static_cast<hipStream_t>(stream),
               static_cast<const uint16_t *>(x), m, k, ldx, static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, map, offsets, n, g.sh(kn),
               g.sw(kn), bias, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_linear_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                      const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_wide(false, "mtq_packed_linear_wide", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream);
}

extern "C" int mtq_packed_matmul_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                      const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_wide(true, "mtq_packed_matmul_wide", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, stream);
}

// 3. skinny
extern "C" size_t mtq_packed_linear_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (skinny_shape(m, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    return skinny_workspace(m, n, g.eff);
}

extern "C" size_t mtq_packed_matmul_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split)
{
    return mtq_packed_linear_skinny_workspace_bytes(m, n, k, split);
}

static int packed_skinny(bool kn, const char *name, const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes,
                         const int8_t *map, const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, int split,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    TileGrid g;
    const StreamArg w = {packed, packed_bytes};
    if (int rc = gemm_args(!x || !packed || !map || !offsets || !y, out_dtype,
                           [&](TileGrid &s) { return skinny_shape(m, n, k, split, &s.th, &s.tw, &s.eff); }, g, k, ldx, n, ldy, false, 0, 0, w, w))
        return rc;
    if (int rc = workspace_args(workspace, workspace_bytes, skinny_workspace(m, n, g.eff), kWsSplit, "split")) return rc;
    const int64_t blocks = (g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves;
    if (int rc = grid_args({blocks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = static_cast<float *>(workspace);
    launch_out(out_dtype, MTQ_TWIN_PAIR(kn, packed_linear_skinny_kernel, packed_matmul_skinny_kernel), dim3((unsigned)blocks),
               dim3(64 * kSkinnyWaves), st, static_cast<const uint16_t *>(x), m, k, ldx, (int)x_vec_of(x, ldx), static_cast<const uint8_t *>(packed),
               (uint64_t)packed_bytes, map, offsets, n, g.sh(kn), g.sw(kn), g.eff, bias, y, ldy, ws);
    if (g.eff > 1) {
        if (int rc = check_launch(name)) return rc;
        launch_out(out_dtype, skinny_reduce_kernel<true>, skinny_reduce_kernel<false>, dim3((unsigned)((m * n + 255) / 256)), dim3(256), st, ws,
                   m * n, n, g.eff, bias, y, ldy);
    }
    return check_launch(name);
}

extern "C" int mtq_packed_linear_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                        const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, int split,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_skinny(false, "mtq_packed_linear_skinny", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, split,
                         workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_matmul_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                                        const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, int split,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_skinny(true, "mtq_packed_matmul_skinny", x, m, k, ldx, packed, packed_bytes, map, offsets, n, bias, y, out_dtype, ldy, split,
                         workspace, workspace_bytes, stream);
}

// 4. skinny grouped, and 5. its chunked form.  Both end in the same reduce when the split is above 1.
extern "C" size_t mtq_packed_linear_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (grouped_shape(total_rows, count, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    return skinny_workspace(total_rows, n, g.eff);
}

extern "C" size_t mtq_packed_matmul_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_linear_skinny_grouped_workspace_bytes(total_rows, count, n, k, split);
}

static int grouped_reduce(const char *name, int out_dtype, hipStream_t st, const float *ws, int64_t total_rows, int64_t n, int split,
                          const int32_t *group_rows, int64_t count, const float *bias, int64_t ldb, void *y, int64_t ldy)
{
    if (split > 1) {
        if (int rc = check_launch(name)) return rc;
        const int64_t nchunks = grouped_nchunks(n);
        launch_out(out_dtype, skinny_grouped_reduce_kernel<true>, skinny_grouped_reduce_kernel<false>, dim3((unsigned)(count * nchunks)), dim3(256),
                   st, ws, total_rows, n, split, group_rows, nchunks, bias, ldb, y, ldy);
    }
    return check_launch(name);
}

static int packed_skinny_grouped(bool kn, const char *name, const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                 const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                 int64_t count, int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, int split,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    TileGrid g;
    const StreamArg w = {packed, packed_bytes};
    if (int rc = gemm_args(!x || !group_rows || !packed || !maps || !offsets || !bases || !y, out_dtype,
                           [&](TileGrid &s) { return grouped_shape(total_rows, count, n, k, split, &s.th, &s.tw, &s.eff); }, g, k, ldx, n, ldy,
                           bias != nullptr, ldb, count, w, w))
        return rc;
    if (int rc = workspace_args(workspace, workspace_bytes, skinny_workspace(total_rows, n, g.eff), kWsSplit, "split")) return rc;
    const int64_t blocks = (count * g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves;
    if (int rc = grid_args({blocks, count * grouped_nchunks(n)})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = static_cast<float *>(workspace);
    launch_out(out_dtype, MTQ_TWIN_PAIR(kn, packed_linear_skinny_grouped_kernel, packed_matmul_skinny_grouped_kernel), dim3((unsigned)blocks),
               dim3(64 * kSkinnyWaves), st, static_cast<const uint16_t *>(x), total_rows, k, ldx, (int)x_vec_of(x, ldx), group_rows,
               static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, maps, offsets, bases, count, n, g.sh(kn), g.sw(kn), g.eff, bias, ldb, y,
               ldy, ws);
    return grouped_reduce(name, out_dtype, st, ws, total_rows, n, g.eff, group_rows, count, bias, ldb, y, ldy);
}

extern "C" int mtq_packed_linear_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                                int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_skinny_grouped(false, "mtq_packed_linear_skinny_grouped", x, total_rows, k, ldx, group_rows, packed, packed_bytes, maps, offsets,
                                 bases, count, n, bias, ldb, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_matmul_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                                int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_skinny_grouped(true, "mtq_packed_matmul_skinny_grouped", x, total_rows, k, ldx, group_rows, packed, packed_bytes, maps, offsets,
                                 bases, count, n, bias, ldb, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

// 4c. skinny grouped with an MoE layer's combine in its reduce.  The wave is 4.'s, storing float32 to the workspace at every split: at an
// effective split of 1 it is launched with the workspace as its float32 Y at pitch n and no bias, slice 0 of [1][S][n], and stores
// acc + 0.0f there; the combine kernel's own + 0.0f leaves that value as it is.
static size_t skinny_combine_workspace(int64_t total_rows, int64_t n, int split_eff)
{
    return ((size_t)std::max(split_eff, 1) * (size_t)total_rows * (size_t)n * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" size_t mtq_packed_linear_skinny_grouped_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (grouped_shape(total_rows, count, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    if (total_rows > ((int64_t)1 << 56) / n) return (size_t)-1;
    return skinny_combine_workspace(total_rows, n, g.eff);
}

extern "C" size_t mtq_packed_matmul_skinny_grouped_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_linear_skinny_grouped_combine_workspace_bytes(total_rows, count, n, k, split);
}

static int packed_skinny_grouped_combine(bool kn, const char *name, const void *x, int64_t k, int64_t ldx, const int32_t *group_rows,
                                         const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                         const uint64_t *bases, int64_t count, int64_t n, int expert_dtype, const int32_t *row_of,
                                         const float *weights, int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens,
                                         int64_t topk, void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                         void *stream, bool chunks = false)
{
    TileGrid g;
    int64_t S = 0;
    const StreamArg w = {packed, packed_bytes};
    if (!row_of || !weights) return fail(MTQ_ERR_INVALID, kNullArg);
    if (int rc = gemm_args(!x || !group_rows || !packed || !maps || !offsets || !bases || !y, out_dtype,
                           [&](TileGrid &s) {
                               if (int rc = dtype_arg(expert_dtype, "expert_dtype")) return rc;
                               if (base)
                                   if (int rc = dtype_arg(base_dtype, "base_dtype")) return rc;
                               if (int rc = moe_slots_arg(tokens, topk, &S)) return rc;
                               if (int rc = grouped_shape(S, count, n, k, split, &s.th, &s.tw, &s.eff)) return rc;
                               if (S > ((int64_t)1 << 56) / n) return fail(MTQ_ERR_INVALID, "the workspace of this split is too large");
                               return (int)MTQ_OK;
                           },
                           g, k, ldx, n, ldy, false, 0, count, w, w))
        return rc;
    if (ldw < topk) return fail(MTQ_ERR_INVALID, "ldw < topk");
    if (base && ldbase < n) return fail(MTQ_ERR_INVALID, "ldbase < n");
    if (ldw > (int64_t)1 << 31 || ldy > (int64_t)1 << 31 || (base && ldbase > (int64_t)1 << 31)) return fail(MTQ_ERR_INVALID, "matrix too large");
    const size_t y_el = out_dtype == MTQ_DTYPE_BF16 ? 2 : 4, base_el = base_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(y) % y_el != 0 || reinterpret_cast<uintptr_t>(row_of) % 4 != 0 || reinterpret_cast<uintptr_t>(weights) % 4 != 0 ||
        (base && reinterpret_cast<uintptr_t>(base) % base_el != 0))
        return fail(MTQ_ERR_INVALID, "an operand is not aligned to its type");
    // chunks: the plan region at the workspace's head and 5.'s wave, a unit axis of `slots` chunk slots where the walk has `count` groups
    const size_t plan = chunks ? grouped_plan_bytes(count) : 0;
    if (int rc = workspace_args(workspace, workspace_bytes, plan + skinny_combine_workspace(S, n, g.eff),
                                "workspace is null: the experts' partial sums need one at every split", "split"))
        return rc;
    const int64_t slots = chunks ? grouped_slots(S, count, kTile) : count;
    const int64_t blocks = (slots * g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves, nchunks = grouped_nchunks(n);
    if (int rc = grid_args({slots, blocks, tokens * nchunks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + plan);
    if (chunks) {
        int32_t *cstart = static_cast<int32_t *>(workspace);
        if (int rc = launch_plan<kTile>(name, st, group_rows, count, S, cstart)) return rc;
        hipLaunchKernelGGL(kn ? packed_matmul_skinny_grouped_chunked_kernel<false> : packed_linear_skinny_grouped_chunked_kernel<false>,
                           dim3((unsigned)blocks), dim3(64 * kSkinnyWaves), 0, st, static_cast<const uint16_t *>(x), (int)S, (int)k, ldx,
                           (int)x_vec_of(x, ldx), group_rows, static_cast<const int32_t *>(cstart), (int)slots,
                           static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, maps, offsets, bases, (int)count, (int)n, (int)g.sh(kn),
                           (int)g.sw(kn), g.eff, static_cast<const float *>(nullptr), (int64_t)0, static_cast<void *>(ws), n, ws);
    } else {
        hipLaunchKernelGGL(kn ? packed_matmul_skinny_grouped_kernel<false> : packed_linear_skinny_grouped_kernel<false>, dim3((unsigned)blocks),
                           dim3(64 * kSkinnyWaves), 0, st, static_cast<const uint16_t *>(x), S, k, ldx, (int)x_vec_of(x, ldx), group_rows,
                           static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, maps, offsets, bases, count, n, g.sh(kn), g.sw(kn), g.eff,
                           static_cast<const float *>(nullptr), (int64_t)0, static_cast<void *>(ws), n, ws);
    }
    if (int rc = check_launch(name)) return rc;
    const int base_kind = !base ? 0 : (base_dtype == MTQ_DTYPE_BF16 ? 1 : 2);
    const dim3 grid((unsigned)(tokens * nchunks));
    if (expert_dtype == MTQ_DTYPE_BF16)
        launch_out(out_dtype, skinny_grouped_combine_kernel<true, true>, skinny_grouped_combine_kernel<true, false>, grid, dim3(256), st, ws, S, n,
                   g.eff, row_of, weights, ldw, base, base_kind, ldbase, (int)topk, nchunks, y, ldy);
    else
        launch_out(out_dtype, skinny_grouped_combine_kernel<false, true>, skinny_grouped_combine_kernel<false, false>, grid, dim3(256), st, ws, S, n,
                   g.eff, row_of, weights, ldw, base, base_kind, ldbase, (int)topk, nchunks, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_linear_skinny_grouped_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                                        size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                                        int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                                        int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                                        void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                        void *stream)
{
    return packed_skinny_grouped_combine(false, "mtq_packed_linear_skinny_grouped_combine", x, k, ldx, group_rows, packed, packed_bytes, maps,
                                         offsets, bases, count, n, expert_dtype, row_of, weights, ldw, base, base_dtype, ldbase, tokens, topk, y,
                                         out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_matmul_skinny_grouped_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                                        size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                                        int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                                        int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                                        void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                        void *stream)
{
    return packed_skinny_grouped_combine(true, "mtq_packed_matmul_skinny_grouped_combine", x, k, ldx, group_rows, packed, packed_bytes, maps,
                                         offsets, bases, count, n, expert_dtype, row_of, weights, ldw, base, base_dtype, ldbase, tokens, topk, y,
                                         out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" size_t mtq_packed_linear_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (grouped_shape(total_rows, count, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    return grouped_plan_bytes(count) + skinny_workspace(total_rows, n, g.eff);
}

extern "C" size_t mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_linear_skinny_grouped_chunked_workspace_bytes(total_rows, count, n, k, split);
}

static int packed_skinny_grouped_chunked(bool kn, const char *name, const void *x, int64_t total_rows, int64_t k, int64_t ldx,
                                         const int32_t *group_rows, const void *packed, size_t packed_bytes, const int8_t *maps,
                                         const uint32_t *offsets, const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb,
                                         void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    TileGrid g;
    const StreamArg w = {packed, packed_bytes};
    if (int rc = gemm_args(!x || !group_rows || !packed || !maps || !offsets || !bases || !y, out_dtype,
                           [&](TileGrid &s) { return grouped_shape(total_rows, count, n, k, split, &s.th, &s.tw, &s.eff); }, g, k, ldx, n, ldy,
                           bias != nullptr, ldb, count, w, w))
        return rc;
    const size_t plan = grouped_plan_bytes(count);
    if (int rc = workspace_args(workspace, workspace_bytes, plan + skinny_workspace(total_rows, n, g.eff), kWsChunks, "call")) return rc;
    const int64_t slots = grouped_slots(total_rows, count, kTile);
    const int64_t blocks = (slots * g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves;
    if (int rc = grid_args({slots, blocks, count * grouped_nchunks(n)})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *cstart = static_cast<int32_t *>(workspace);
    float *ws = reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + plan);
    if (int rc = launch_plan<kTile>(name, st, group_rows, count, total_rows, cstart)) return rc;
    launch_out(out_dtype, MTQ_TWIN_PAIR(kn, packed_linear_skinny_grouped_chunked_kernel, packed_matmul_skinny_grouped_chunked_kernel),
               dim3((unsigned)blocks), dim3(64 * kSkinnyWaves), st, static_cast<const uint16_t *>(x), total_rows, k, ldx, (int)x_vec_of(x, ldx),
               group_rows, cstart, (int)slots, static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, maps, offsets, bases, count, n,
               g.sh(kn), g.sw(kn), g.eff, bias, ldb, y, ldy, ws);
    return grouped_reduce(name, out_dtype, st, ws, total_rows, n, g.eff, group_rows, count, bias, ldb, y, ldy);
}

extern "C" int mtq_packed_linear_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                        const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                        const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                                        int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                        void *stream)
{
    return packed_skinny_grouped_chunked(false, "mtq_packed_linear_skinny_grouped_chunked", x, total_rows, k, ldx, group_rows, packed, packed_bytes,
                                         maps, offsets, bases, count, n, bias, ldb, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_matmul_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                        const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                                        const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                                        int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                        void *stream)
{
    return packed_skinny_grouped_chunked(true, "mtq_packed_matmul_skinny_grouped_chunked", x, total_rows, k, ldx, group_rows, packed, packed_bytes,
                                         maps, offsets, bases, count, n, bias, ldb, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

// 6. wide grouped
extern "C" size_t mtq_packed_linear_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k)
{
    TileGrid g;
    if (grouped_shape(total_rows, count, n, k, 1, &g.th, &g.tw, &g.eff)) return (size_t)-1;   // split 1: no split over K, no partials
    return grouped_plan_bytes(count);
}

extern "C" size_t mtq_packed_matmul_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k)
{
    return mtq_packed_linear_wide_grouped_workspace_bytes(total_rows, count, n, k);
}

static int packed_wide_grouped(bool kn, const char *name, const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                               const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                               int64_t count, int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    TileGrid g;
    const StreamArg w = {packed, packed_bytes};
    if (int rc = gemm_args(!x || !group_rows || !packed || !maps || !offsets || !bases || !y, out_dtype,
                           [&](TileGrid &s) { return grouped_shape(total_rows, count, n, k, 1, &s.th, &s.tw, &s.eff); }, g, k, ldx, n, ldy,
                           bias != nullptr, ldb, count, w, w))
        return rc;
    if (int rc = workspace_args(workspace, workspace_bytes, grouped_plan_bytes(count), kWsPlan, "call")) return rc;
    const int64_t slots = grouped_slots(total_rows, count, kWideBM);
    const int64_t blocks = slots * ((n + kWideBN - 1) / kWideBN);
    if (int rc = grid_args({slots, blocks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *bstart = static_cast<int32_t *>(workspace);
    if (int rc = launch_plan<kWideBM>(name, st, group_rows, count, total_rows, bstart)) return rc;
    const bool x_vec = x_vec_wide(x, ldx, k);
    launch_out(out_dtype, MTQ_WIDE_PAIR(packed_wide_grouped_kernel, x_vec, kn), dim3((unsigned)blocks), dim3(kThreads), st,
               static_cast<const uint16_t *>(x), (int)total_rows, k, ldx, group_rows, bstart, static_cast<const uint8_t *>(packed),
               (uint64_t)packed_bytes, maps, offsets, bases, (int)count, n, g.sh(kn), g.sw(kn), bias, ldb, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_linear_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                              const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                              const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                              int out_dtype, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_wide_grouped(false, "mtq_packed_linear_wide_grouped", x, total_rows, k, ldx, group_rows, packed, packed_bytes, maps, offsets, bases,
                               count, n, bias, ldb, y, out_dtype, ldy, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_matmul_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                              const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                              const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                              int out_dtype, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_wide_grouped(true, "mtq_packed_matmul_wide_grouped", x, total_rows, k, ldx, group_rows, packed, packed_bytes, maps, offsets, bases,
                               count, n, bias, ldb, y, out_dtype, ldy, workspace, workspace_bytes, stream);
}

// ---- gated entries
static int glu_act(int act)
{
    if (act != MTQ_ACT_SILU && act != MTQ_ACT_NONE) return fail(MTQ_ERR_UNSUPPORTED, "act must be MTQ_ACT_SILU or MTQ_ACT_NONE");
    return MTQ_OK;
}

extern "C" int mtq_glu_combine(const float *g, int64_t ldg, const float *u, int64_t ldu, int64_t rows, int64_t cols, int act, void *y,
                               int out_dtype, int64_t ldy, void *stream)
{
    if (!g || !u || !y) return fail(MTQ_ERR_INVALID, kNullArg);
    if (int rc = dtype_arg(out_dtype, "out_dtype")) return rc;
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive (empty operands are handled by the caller)");
    if (rows > (int64_t)1 << 40 || cols > (int64_t)1 << 30 || rows > ((int64_t)1 << 56) / cols) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (ldg < cols) return fail(MTQ_ERR_INVALID, "ldg < cols");
    if (ldu < cols) return fail(MTQ_ERR_INVALID, "ldu < cols");
    if (ldy < cols) return fail(MTQ_ERR_INVALID, "ldy < cols");
    if (int rc = glu_act(act)) return rc;
    if (int rc = require_device()) return rc;
    const dim3 grid((unsigned)std::min<int64_t>((rows * cols + 255) / 256, (int64_t)1 << 20));
    launch_out(out_dtype, glu_combine_kernel<true>, glu_combine_kernel<false>, grid, dim3(256), static_cast<hipStream_t>(stream), g, ldg, u, ldu, rows,
               cols, act, y, ldy);
    return check_launch("mtq_glu_combine");
}

// 7. glu wide
static int packed_glu_wide(bool kn, const char *name, const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                           const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes, const int8_t *up_map,
                           const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up, int act, void *y, int out_dtype,
                           int64_t ldy, void *stream)
{
    TileGrid g;
    if (int rc = linear_args(x, m, k, ldx, gate_packed, gate_bytes, gate_map, gate_offsets, n, y, out_dtype, ldy, g)) return rc;
    if (int rc = linear_args(x, m, k, ldx, up_packed, up_bytes, up_map, up_offsets, n, y, out_dtype, ldy, g)) return rc;
    if (int rc = glu_act(act)) return rc;
    const int64_t blocks = ((m + kWideBM - 1) / kWideBM) * ((n + kGluBN - 1) / kGluBN);
    if (int rc = grid_args({blocks}, true)) return rc;
    if (int rc = require_device()) return rc;
    const bool x_vec = x_vec_wide(x, ldx, k);
    launch_out(out_dtype, MTQ_WIDE_PAIR(packed_glu_wide_kernel, x_vec, kn), dim3((unsigned)blocks), dim3(kThreads), static_cast<hipStream_t>(stream),
               static_cast<const uint16_t *>(x), m, k, ldx, static_cast<const uint8_t *>(gate_packed), (uint64_t)gate_bytes, gate_map, gate_offsets,
               static_cast<const uint8_t *>(up_packed), (uint64_t)up_bytes, up_map, up_offsets, n, g.sh(kn), g.sw(kn), bias_gate, bias_up, act, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_glu_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                                   const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                                   const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up,
                                   int act, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_glu_wide(false, "mtq_packed_glu_wide", x, m, k, ldx, gate_packed, gate_bytes, gate_map, gate_offsets, up_packed, up_bytes, up_map,
                           up_offsets, n, bias_gate, bias_up, act, y, out_dtype, ldy, stream);
}

extern "C" int mtq_packed_glu_matmul_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                                          const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                                          const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate,
                                          const float *bias_up, int act, void *y, int out_dtype, int64_t ldy, void *stream)
{
    return packed_glu_wide(true, "mtq_packed_glu_matmul_wide", x, m, k, ldx, gate_packed, gate_bytes, gate_map, gate_offsets, up_packed, up_bytes,
                           up_map, up_offsets, n, bias_gate, bias_up, act, y, out_dtype, ldy, stream);
}

// 8. glu wide grouped: the wide grouped entry's plan and slot bound, column blocks of kGluBN
extern "C" size_t mtq_packed_glu_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k)
{
    return mtq_packed_linear_wide_grouped_workspace_bytes(total_rows, count, n, k);   // the same plan
}

extern "C" size_t mtq_packed_glu_matmul_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k)
{
    return mtq_packed_glu_wide_grouped_workspace_bytes(total_rows, count, n, k);
}

static int packed_glu_wide_grouped(bool kn, const char *name, const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                   const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                   const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                   const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                   const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    TileGrid g;
    if (int rc = gemm_args(!x || !group_rows || !gate_packed || !gate_maps || !gate_offsets || !gate_bases || !up_packed || !up_maps || !up_offsets ||
                               !up_bases || !y,
                           out_dtype, [&](TileGrid &s) { return grouped_shape(total_rows, count, n, k, 1, &s.th, &s.tw, &s.eff); }, g, k, ldx, n,
                           ldy, bias_gate || bias_up, ldb, count, {gate_packed, gate_bytes}, {up_packed, up_bytes}))
        return rc;
    if (int rc = glu_act(act)) return rc;
    if (int rc = workspace_args(workspace, workspace_bytes, grouped_plan_bytes(count), kWsPlan, "call")) return rc;
    const int64_t slots = grouped_slots(total_rows, count, kWideBM);
    const int64_t blocks = slots * ((n + kGluBN - 1) / kGluBN);
    if (int rc = grid_args({slots, blocks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *bstart = static_cast<int32_t *>(workspace);
    if (int rc = launch_plan<kWideBM>(name, st, group_rows, count, total_rows, bstart)) return rc;
    const bool x_vec = x_vec_wide(x, ldx, k);
    launch_out(out_dtype, MTQ_WIDE_PAIR(packed_glu_wide_grouped_kernel, x_vec, kn), dim3((unsigned)blocks), dim3(kThreads), st,
               static_cast<const uint16_t *>(x), (int)total_rows, k, ldx, group_rows, bstart, static_cast<const uint8_t *>(gate_packed),
               (uint64_t)gate_bytes, gate_maps, gate_offsets, gate_bases, static_cast<const uint8_t *>(up_packed), (uint64_t)up_bytes, up_maps,
               up_offsets, up_bases, (int)count, n, g.sh(kn), g.sw(kn), bias_gate, bias_up, ldb, act, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_glu_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                           const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                           const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                           const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                           const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return packed_glu_wide_grouped(false, "mtq_packed_glu_wide_grouped", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes, gate_maps,
                                   gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate, bias_up, ldb, act,
                                   y, out_dtype, ldy, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_glu_matmul_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                  const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                  const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed, size_t up_bytes,
                                                  const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count,
                                                  int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y,
                                                  int out_dtype, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_glu_wide_grouped(true, "mtq_packed_glu_matmul_wide_grouped", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes, gate_maps,
                                   gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate, bias_up, ldb, act,
                                   y, out_dtype, ldy, workspace, workspace_bytes, stream);
}

// 9. glu skinny: the gated entries for decode, both projections in one split-K launch, the activation in the reduce
extern "C" size_t mtq_packed_glu_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (skinny_shape(m, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    return glu_skinny_workspace(m, n, g.eff);
}

extern "C" size_t mtq_packed_glu_matmul_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_workspace_bytes(m, n, k, split);
}

static int packed_glu_skinny(bool kn, const char *name, const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                             const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes, const int8_t *up_map,
                             const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up, int act, void *y, int out_dtype,
                             int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    TileGrid g;
    if (int rc = gemm_args(!x || !gate_packed || !gate_map || !gate_offsets || !up_packed || !up_map || !up_offsets || !y, out_dtype,
                           [&](TileGrid &s) { return skinny_shape(m, n, k, split, &s.th, &s.tw, &s.eff); }, g, k, ldx, n, ldy, false, 0, 0,
                           {gate_packed, gate_bytes}, {up_packed, up_bytes}))
        return rc;
    if (int rc = glu_act(act)) return rc;
    if (int rc = workspace_args(workspace, workspace_bytes, glu_skinny_workspace(m, n, g.eff), kWsGlu, "split")) return rc;
    const int64_t blocks = (2 * g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves;
    if (int rc = grid_args({blocks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = static_cast<float *>(workspace);
    hipLaunchKernelGGL(kn ? packed_glu_matmul_skinny_kernel : packed_glu_skinny_kernel, dim3((unsigned)blocks), dim3(64 * kSkinnyWaves), 0, st,
                       static_cast<const uint16_t *>(x), m, k, ldx, (int)x_vec_of(x, ldx), static_cast<const uint8_t *>(gate_packed),
                       (uint64_t)gate_bytes, gate_map, gate_offsets, static_cast<const uint8_t *>(up_packed), (uint64_t)up_bytes, up_map, up_offsets, n,
                       g.sh(kn), g.sw(kn), g.eff, ws);
    if (int rc = check_launch(name)) return rc;
    launch_out(out_dtype, glu_skinny_reduce_kernel<true>, glu_skinny_reduce_kernel<false>, dim3((unsigned)((m * n + 255) / 256)), dim3(256), st, ws,
               m * n, n, g.eff, bias_gate, bias_up, act, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_glu_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                                     const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                                     const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up,
                                     int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    return packed_glu_skinny(false, "mtq_packed_glu_skinny", x, m, k, ldx, gate_packed, gate_bytes, gate_map, gate_offsets, up_packed, up_bytes, up_map,
                             up_offsets, n, bias_gate, bias_up, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_glu_matmul_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                                            const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                                            const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate,
                                            const float *bias_up, int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    return packed_glu_skinny(true, "mtq_packed_glu_matmul_skinny", x, m, k, ldx, gate_packed, gate_bytes, gate_map, gate_offsets, up_packed, up_bytes,
                             up_map, up_offsets, n, bias_gate, bias_up, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

// 10. glu skinny grouped.  grouped_shape and the bound that keeps the two projections' partials inside size_t at every split
static int glu_grouped_shape(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split, int64_t *th, int64_t *tw, int *eff)
{
    if (int rc = grouped_shape(total_rows, count, n, k, split, th, tw, eff)) return rc;
    if (total_rows > ((int64_t)1 << 55) / n / *eff) return fail(MTQ_ERR_INVALID, "the workspace of this split is too large");
    return MTQ_OK;
}

extern "C" size_t mtq_packed_glu_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    TileGrid g;
    if (glu_grouped_shape(total_rows, count, n, k, split, &g.th, &g.tw, &g.eff)) return (size_t)-1;
    return glu_skinny_workspace(total_rows, n, g.eff);
}

extern "C" size_t mtq_packed_glu_matmul_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_grouped_workspace_bytes(total_rows, count, n, k, split);
}

// gather: the *_gather entries - x is the (tokens, k) token matrix, src the plan's int32 [S], and total_rows is formed here as
// S = tokens * topk once mtq_moe_plan's limits hold; what mtq_moe_dispatch refuses is refused here too.
static int packed_glu_skinny_grouped(bool kn, const char *name, const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                     const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                     const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                     const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                     const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                     size_t workspace_bytes, void *stream, bool gather = false, const int32_t *src = nullptr, int64_t tokens = 0,
                                     int64_t topk = 0, bool chunks = false)
{
    TileGrid g;
    if (int rc = gemm_args(!x || !group_rows || !gate_packed || !gate_maps || !gate_offsets || !gate_bases || !up_packed || !up_maps || !up_offsets ||
                               !up_bases || !y || (gather && !src),
                           out_dtype,
                           [&](TileGrid &s) {
                               if (gather) {
                                   if (int rc = moe_slots_arg(tokens, topk, &total_rows)) return rc;
                               }
                               return glu_grouped_shape(total_rows, count, n, k, split, &s.th, &s.tw, &s.eff);
                           },
                           g, k, ldx, n, ldy, bias_gate || bias_up, ldb, count, {gate_packed, gate_bytes}, {up_packed, up_bytes}))
        return rc;
    if (gather) {
        if (ldx > (int64_t)1 << 40) return fail(MTQ_ERR_INVALID, "matrix too large");
        if (reinterpret_cast<uintptr_t>(x) % 2 != 0 || reinterpret_cast<uintptr_t>(src) % 4 != 0)
            return fail(MTQ_ERR_INVALID, "x or src is not aligned to its type");
    }
    if (int rc = glu_act(act)) return rc;
    // chunks: the plan region at the workspace's head, a unit axis of `slots` chunk slots where the walk has `count` groups
    const size_t plan = chunks ? grouped_plan_bytes(count) : 0;
    if (int rc = workspace_args(workspace, workspace_bytes, plan + glu_skinny_workspace(total_rows, n, g.eff), kWsGlu, "split")) return rc;
    const int64_t slots = chunks ? grouped_slots(total_rows, count, kTile) : count;
    const int64_t blocks = (2 * slots * g.th * g.eff + kSkinnyWaves - 1) / kSkinnyWaves;
    const int64_t nchunks = grouped_nchunks(n);
    if (int rc = grid_args({slots, blocks, slots * nchunks})) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + plan);
    if (chunks) {
        int32_t *cstart = static_cast<int32_t *>(workspace);
        if (int rc = launch_plan<kTile>(name, st, group_rows, count, total_rows, cstart)) return rc;
        hipLaunchKernelGGL(gather ? (kn ? packed_glu_matmul_skinny_grouped_chunked_kernel<true> : packed_glu_skinny_grouped_chunked_kernel<true>)
                                  : (kn ? packed_glu_matmul_skinny_grouped_chunked_kernel<false> : packed_glu_skinny_grouped_chunked_kernel<false>),
                           dim3((unsigned)blocks), dim3(64 * kSkinnyWaves), 0, st, static_cast<const uint16_t *>(x), (int)total_rows, (int)k, ldx,
                           (int)x_vec_of(x, ldx), group_rows, static_cast<const int32_t *>(cstart), (int)slots,
                           static_cast<const uint8_t *>(gate_packed), (uint64_t)gate_bytes, gate_maps, gate_offsets, gate_bases,
                           static_cast<const uint8_t *>(up_packed), (uint64_t)up_bytes, up_maps, up_offsets, up_bases, (int)count, (int)n,
                           (int)g.sh(kn), (int)g.sw(kn), g.eff, ws, src, (int)topk);
        if (int rc = check_launch(name)) return rc;
        launch_out(out_dtype, glu_skinny_grouped_chunked_reduce_kernel<true>, glu_skinny_grouped_chunked_reduce_kernel<false>,
                   dim3((unsigned)(slots * nchunks)), dim3(256), st, ws, total_rows, n, g.eff, group_rows, static_cast<const int32_t *>(cstart),
                   (int)count, nchunks, bias_gate, bias_up, ldb, act, y, ldy);
        return check_launch(name);
    }
    hipLaunchKernelGGL(gather ? (kn ? packed_glu_matmul_skinny_grouped_kernel<true> : packed_glu_skinny_grouped_kernel<true>)
                              : (kn ? packed_glu_matmul_skinny_grouped_kernel<false> : packed_glu_skinny_grouped_kernel<false>),
                       dim3((unsigned)blocks), dim3(64 * kSkinnyWaves), 0, st, static_cast<const uint16_t *>(x), (int)total_rows, (int)k, ldx,
                       (int)x_vec_of(x, ldx), group_rows, static_cast<const uint8_t *>(gate_packed), (uint64_t)gate_bytes, gate_maps, gate_offsets,
                       gate_bases, static_cast<const uint8_t *>(up_packed), (uint64_t)up_bytes, up_maps, up_offsets, up_bases, (int)count, (int)n,
                       (int)g.sh(kn), (int)g.sw(kn), g.eff, ws, src, (int)topk);
    if (int rc = check_launch(name)) return rc;
    launch_out(out_dtype, glu_skinny_grouped_reduce_kernel<true>, glu_skinny_grouped_reduce_kernel<false>, dim3((unsigned)(count * nchunks)), dim3(256),
               st, ws, total_rows, n, g.eff, group_rows, nchunks, bias_gate, bias_up, ldb, act, y, ldy);
    return check_launch(name);
}

extern "C" int mtq_packed_glu_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                             const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                             const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                             const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                             const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y, int out_dtype,
                                             int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_glu_skinny_grouped(false, "mtq_packed_glu_skinny_grouped", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes, gate_maps,
                                     gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate, bias_up, ldb,
                                     act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

extern "C" int mtq_packed_glu_matmul_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                    const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                    const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed,
                                                    size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                    int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb, int act,
                                                    void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                    void *stream)
{
    return packed_glu_skinny_grouped(true, "mtq_packed_glu_matmul_skinny_grouped", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream);
}

// 10g. glu skinny grouped with an MoE layer's gather in the wave's X loads: 10.'s body, workspace and reduce
extern "C" size_t mtq_packed_glu_skinny_grouped_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_grouped_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" size_t mtq_packed_glu_matmul_skinny_grouped_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_grouped_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" int mtq_packed_glu_skinny_grouped_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                                    const int32_t *group_rows, const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                    const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed,
                                                    size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                    int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb, int act,
                                                    void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                    void *stream)
{
    return packed_glu_skinny_grouped(false, "mtq_packed_glu_skinny_grouped_gather", x, 0, k, ldx, group_rows, gate_packed, gate_bytes, gate_maps,
                                     gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate, bias_up, ldb,
                                     act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, true, src, tokens, topk);
}

extern "C" int mtq_packed_glu_matmul_skinny_grouped_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                                           const int32_t *group_rows, const void *gate_packed, size_t gate_bytes,
                                                           const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                                           const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                                           const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                                           const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y,
                                                           int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                           void *stream)
{
    return packed_glu_skinny_grouped(true, "mtq_packed_glu_matmul_skinny_grouped_gather", x, 0, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, true, src, tokens, topk);
}

// 10c. The decode route's entries with a wave per 32-row chunk (include/mtq_glu_chunked.h): the bodies of 10., 10g. and 4c. with
// `chunks` set - the parent's checks in the parent's order, the plan region of 5. at the head of the parent's workspace.
static size_t chunked_size(size_t parent, int64_t count) { return parent == (size_t)-1 ? parent : grouped_plan_bytes(count) + parent; }

extern "C" size_t mtq_packed_glu_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return chunked_size(mtq_packed_glu_skinny_grouped_workspace_bytes(total_rows, count, n, k, split), count);
}

extern "C" size_t mtq_packed_glu_matmul_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_grouped_chunked_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" size_t mtq_packed_glu_skinny_grouped_chunked_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_glu_skinny_grouped_chunked_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" size_t mtq_packed_glu_matmul_skinny_grouped_chunked_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k,
                                                                                      int split)
{
    return mtq_packed_glu_skinny_grouped_chunked_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" size_t mtq_packed_linear_skinny_grouped_chunked_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return chunked_size(mtq_packed_linear_skinny_grouped_combine_workspace_bytes(total_rows, count, n, k, split), count);
}

extern "C" size_t mtq_packed_matmul_skinny_grouped_chunked_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split)
{
    return mtq_packed_linear_skinny_grouped_chunked_combine_workspace_bytes(total_rows, count, n, k, split);
}

extern "C" int mtq_packed_glu_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                     const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                     const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed,
                                                     size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                     int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb, int act,
                                                     void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                     void *stream)
{
    return packed_glu_skinny_grouped(false, "mtq_packed_glu_skinny_grouped_chunked", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, false, nullptr, 0, 0, true);
}

extern "C" int mtq_packed_glu_matmul_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                            const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                            const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed,
                                                            size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets,
                                                            const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                                            const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy,
                                                            int split, void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_glu_skinny_grouped(true, "mtq_packed_glu_matmul_skinny_grouped_chunked", x, total_rows, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, false, nullptr, 0, 0, true);
}

extern "C" int mtq_packed_glu_skinny_grouped_chunked_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                                            const int32_t *group_rows, const void *gate_packed, size_t gate_bytes,
                                                            const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                                            const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                                            const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                                            const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y,
                                                            int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                            void *stream)
{
    return packed_glu_skinny_grouped(false, "mtq_packed_glu_skinny_grouped_chunked_gather", x, 0, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, true, src, tokens, topk, true);
}

extern "C" int mtq_packed_glu_matmul_skinny_grouped_chunked_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx,
                                                                   const int32_t *src, const int32_t *group_rows, const void *gate_packed,
                                                                   size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                                                   const uint64_t *gate_bases, const void *up_packed, size_t up_bytes,
                                                                   const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                                   int64_t count, int64_t n, const float *bias_gate, const float *bias_up,
                                                                   int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split,
                                                                   void *workspace, size_t workspace_bytes, void *stream)
{
    return packed_glu_skinny_grouped(true, "mtq_packed_glu_matmul_skinny_grouped_chunked_gather", x, 0, k, ldx, group_rows, gate_packed, gate_bytes,
                                     gate_maps, gate_offsets, gate_bases, up_packed, up_bytes, up_maps, up_offsets, up_bases, count, n, bias_gate,
                                     bias_up, ldb, act, y, out_dtype, ldy, split, workspace, workspace_bytes, stream, true, src, tokens, topk, true);
}

extern "C" int mtq_packed_linear_skinny_grouped_chunked_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                                const void *packed, size_t packed_bytes, const int8_t *maps,
                                                                const uint32_t *offsets, const uint64_t *bases, int64_t count, int64_t n,
                                                                int expert_dtype, const int32_t *row_of, const float *weights, int64_t ldw,
                                                                const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                                                void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                                                size_t workspace_bytes, void *stream)
{
    return packed_skinny_grouped_combine(false, "mtq_packed_linear_skinny_grouped_chunked_combine", x, k, ldx, group_rows, packed, packed_bytes, maps,
                                         offsets, bases, count, n, expert_dtype, row_of, weights, ldw, base, base_dtype, ldbase, tokens, topk, y,
                                         out_dtype, ldy, split, workspace, workspace_bytes, stream, true);
}

extern "C" int mtq_packed_matmul_skinny_grouped_chunked_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                                const void *packed, size_t packed_bytes, const int8_t *maps,
                                                                const uint32_t *offsets, const uint64_t *bases, int64_t count, int64_t n,
                                                                int expert_dtype, const int32_t *row_of, const float *weights, int64_t ldw,
                                                                const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                                                void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                                                size_t workspace_bytes, void *stream)
{
    return packed_skinny_grouped_combine(true, "mtq_packed_matmul_skinny_grouped_chunked_combine", x, k, ldx, group_rows, packed, packed_bytes, maps,
                                         offsets, bases, count, n, expert_dtype, row_of, weights, ldw, base, base_dtype, ldbase, tokens, topk, y,
                                         out_dtype, ldy, split, workspace, workspace_bytes, stream, true);
}

extern "C" int mtq_debug_packed_decode(int fmt, uint32_t *got, uint32_t *want, void *stream)
{
    if (!got || !want) return fail(MTQ_ERR_INVALID, "null argument");
    if (fmt < MTQ_FMT_BFP8 || fmt > MTQ_FMT_BFP2) return fail(MTQ_ERR_INVALID, "fmt must be MTQ_FMT_BFP8, MTQ_FMT_BFP4 or MTQ_FMT_BFP2");
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(packed_decode_probe_kernel, dim3(kProbeGroups / 256), dim3(256), 0, static_cast<hipStream_t>(stream), fmt, got, want);
    return check_launch("mtq_debug_packed_decode");
}
