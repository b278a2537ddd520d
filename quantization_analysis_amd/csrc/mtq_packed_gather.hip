// mtq_packed_gather.hip — the input embedding over a packed table (include/mtq_packed_gather.h): token rows gathered straight from the
// packed stream of include/mtq.h ("PACKED mixed-tile weights"), no unpacked table anywhere.  No arithmetic but the decode (and one f32
// multiply when a scale is given): a scattered, latency-bound walk id → map code and offset → blob.
//
//   packed_gather_rows_kernel      the stream of a (vocab, hidden) table; token i is row i.  A lane is one 16-value group of one token's
//       row, a wave 64 consecutive groups (1024 columns, 32 tiles of one tile row): a unit.  A wave takes kUnits consecutive units at a
//       time (a row's next 1024 columns, then the next token) and issues the id, map and offset loads of all of them, then all their
//       code loads, then decodes and stores: the three dependent loads of kUnits units overlap.  The two lanes of a tile share one
//       lookup (the even lane's, passed across).  Every lane stores 32 contiguous bytes of bf16 (64 of f32): a wave's store is one run.
//   packed_gather_columns_kernel   the stream of the (hidden, vocab) transpose; token i is column i.  A lane is one element, hidden
//       index h: row h & 31 of tile (h >> 5, id >> 5); a wave is 64 consecutive h (two tiles, lanes 0 and 32 look them up), kUnits units
//       at a time in the same three phases.  Each element costs a 32-byte sector of the stream: inherent to a column of a row-major
//       blob.  Consecutive lanes store consecutive outputs.
//
// Both: ids int32 or int64, id_first subtracted in 64 bits, an id outside the table → a row of +0; a tile whose code is outside 0..3 or
// whose blob passes packed_bytes reads as zeros (unpack's guard, before the blob is touched); nothing is stored outside
// tokens × hidden.  No atomics, no workspace, no LDS.  Without a scale the words are mtq_unpack_tiles's, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kUnit = 64;                           // offsets count units of 64 bytes
constexpr int kExpBytes = 64;                       // shared exponents at the head of a BFP blob
constexpr int kUnits = 4;                           // units a wave has in flight
constexpr int kWaves = 4;                           // waves of a workgroup
constexpr int64_t kMaxBlocks = 2048;                // the grid's cap: 256 CUs x 8 workgroups of 4 waves; more work loops

__host__ __device__ constexpr uint32_t blob_bytes(int f)
{
    return f == 0 ? 2048u : (f == 1 ? 1088u : (f == 2 ? 576u : (f == 3 ? 320u : 0u)));
}

// float32 → bf16, round to nearest even; NaN stays NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + (0x7FFFu + ((u >> 16) & 1u))) >> 16);
}

struct Table {
    const uint8_t *packed;
    uint64_t packed_bytes;
    const int8_t *map;
    const uint32_t *offsets;
    int64_t tiles_w;
    int64_t vocab, hidden;
};

template <bool ID64>
__device__ __forceinline__ int64_t token_id(const void *__restrict__ ids, int64_t t)
{
    if constexpr (ID64) return static_cast<const int64_t *>(ids)[t];
    else return static_cast<const int32_t *>(ids)[t];
}

// What a lookup gives: the blob's byte offset and its format, f < 0 for a tile that reads as zeros (an id outside the table, a code that
// is no format, a blob past the end of the buffer).
struct Where {
    uint64_t off;
    int f;
};

__device__ __forceinline__ Where look_up(const Table &tb, int64_t tile)
{
    Where w;
    const int f = tb.map[tile];
    w.off = (uint64_t)tb.offsets[tile] * kUnit;
    const uint32_t size = blob_bytes(f);
    w.f = (size == 0u || w.off + size > tb.packed_bytes) ? -1 : f;
    return w;
}

// One lane's lookup handed to the lanes that share its tile: `from` is the owning lane.
__device__ __forceinline__ Where share(const Where &w, int from)
{
    Where r;
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)w.off, from), hi = (uint32_t)__shfl((int)(uint32_t)(w.off >> 32), from);
    r.off = ((uint64_t)hi << 32) | lo;
    r.f = __shfl(w.f, from);
    return r;
}

// ---- rows

struct RowUnit {
    int64_t t;                                      // token, -1: past the end
    int64_t col0;                                   // the lane's first column
    bool in_table;                                  // the token's id is a row of the table
    Where at;
    int gi;                                         // the lane's group in the blob: 2 * (id & 31) + half
    uint32_t w[8];                                  // the group's code bytes
    uint32_t E;
};

// the codes' width is a constant of each instance, so every word index below is one too and the raw bytes stay in registers
template <int F>
__device__ __forceinline__ void decode_bfp(const RowUnit &u, uint32_t (&y)[kGroup])
{
    constexpr uint32_t M = F == 1 ? 7u : (F == 2 ? 3u : 1u), B = M + 1u;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const uint32_t code = (u.w[(i * B) >> 5] >> ((i * B) & 31u)) & ((1u << B) - 1u);
        y[i] = bfp_code_bits_rt(code, u.E, M);
    }
}

// the group's 16 float32 words from its raw bytes (mtq_packed.hip's decode_group)
__device__ __forceinline__ void decode_row_group(const RowUnit &u, uint32_t (&y)[kGroup])
{
    if (u.at.f == 0) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = (i & 1) ? (u.w[i >> 1] & 0xFFFF0000u) : (u.w[i >> 1] << 16);
    } else if (u.at.f == 1) {
        decode_bfp<1>(u, y);
    } else if (u.at.f == 2) {
        decode_bfp<2>(u, y);
    } else if (u.at.f == 3) {
        decode_bfp<3>(u, y);
    } else {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = 0u;
    }
}

template <bool BF16OUT>
__device__ __forceinline__ void store_row_group(const uint32_t (&y)[kGroup], void *__restrict__ yv, int64_t at, int64_t left, bool vec_ok)
{
    const bool whole = left >= kGroup && vec_ok;
    if constexpr (BF16OUT) {
        uint16_t *yr = static_cast<uint16_t *>(yv) + at;
        if (whole) {
            uint32_t pk[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) pk[i] = (y[2 * i] >> 16) | (y[2 * i + 1] & 0xFFFF0000u);
            reinterpret_cast<uint4 *>(yr)[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            reinterpret_cast<uint4 *>(yr)[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (i < left) yr[i] = (uint16_t)(y[i] >> 16);
        }
    } else {
        uint32_t *yr = static_cast<uint32_t *>(yv) + at;
        if (whole) {
#pragma unroll
            for (int i = 0; i < 4; ++i) reinterpret_cast<uint4 *>(yr)[i] = make_uint4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                if (i < left) yr[i] = y[i];
        }
    }
}

// value · scale in float32; a bf16 output takes the product's one rounding, so the words keep it whole until the store
template <bool BF16OUT>
__device__ __forceinline__ uint32_t scaled_word(uint32_t word, float scale)
{
    const float p = __uint_as_float(word) * scale;
    if constexpr (BF16OUT) return (uint32_t)f32_to_bf16(p) << 16;
    else return __float_as_uint(p);
}

template <bool ID64, bool BF16OUT, bool SCALE>
__global__ __launch_bounds__(64 * kWaves) void packed_gather_rows_kernel(const void *__restrict__ ids, int64_t tokens, int64_t id_first, Table tb,
                                                                         int64_t chunks, float scale, void *__restrict__ yv, int64_t ldy, int vec_ok)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t units = tokens * chunks, waves = (int64_t)gridDim.x * kWaves;
    for (int64_t first = ((int64_t)blockIdx.x * kWaves + wave) * kUnits; first < units; first += waves * kUnits) {
        RowUnit u[kUnits];
        // 1: id → tile → (code, offset), for every unit before any blob is touched
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int64_t unit = first + j;
            u[j].t = unit < units ? unit / chunks : -1;
            const int64_t group = (unit % chunks) * 64 + lane;
            u[j].col0 = group * kGroup;
            int64_t id = -1;
            if (u[j].t >= 0 && u[j].col0 < tb.hidden) id = token_id<ID64>(ids, u[j].t) - id_first;
            else u[j].t = -1;
            u[j].in_table = id >= 0 && id < tb.vocab;
            Where w{0, -1};
            if (u[j].in_table && (lane & 1) == 0) w = look_up(tb, (id >> 5) * tb.tiles_w + (group >> 1));
            u[j].at = share(w, lane & ~1);            // the odd lane's tile is its even neighbour's, which is inside whenever the odd one is
            if (!u[j].in_table) u[j].at.f = -1;
            u[j].gi = 2 * (int)(id & 31) + (lane & 1);
        }
        // 2: the code bytes and the exponent byte
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int gi = u[j].gi, f = u[j].at.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) u[j].w[i] = 0u;
            u[j].E = 0u;
            if (f < 0) continue;
            const uint8_t *blob = tb.packed + u[j].at.off;
            if (f == 0) {
                const uint4 *q = reinterpret_cast<const uint4 *>(blob + gi * 32);
                const uint4 lo = q[0], hi = q[1];
                u[j].w[0] = lo.x; u[j].w[1] = lo.y; u[j].w[2] = lo.z; u[j].w[3] = lo.w;
                u[j].w[4] = hi.x; u[j].w[5] = hi.y; u[j].w[6] = hi.z; u[j].w[7] = hi.w;
                continue;
            }
            u[j].E = blob[gi];
            if (f == 1) {
                const uint4 v = *reinterpret_cast<const uint4 *>(blob + kExpBytes + gi * 16);
                u[j].w[0] = v.x; u[j].w[1] = v.y; u[j].w[2] = v.z; u[j].w[3] = v.w;
            } else if (f == 2) {
                const uint2 v = *reinterpret_cast<const uint2 *>(blob + kExpBytes + gi * 8);
                u[j].w[0] = v.x; u[j].w[1] = v.y;
            } else {
                u[j].w[0] = *reinterpret_cast<const uint32_t *>(blob + kExpBytes + gi * 4);
            }
        }
        // 3: decode, scale, store
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            if (u[j].t < 0) continue;
            uint32_t y[kGroup];
            decode_row_group(u[j], y);
            if constexpr (SCALE) {
                if (u[j].in_table) {                 // a row outside the table is +0 whatever the scale's sign
#pragma unroll
                    for (int i = 0; i < kGroup; ++i) y[i] = scaled_word<BF16OUT>(y[i], scale);
                }
            }
            store_row_group<BF16OUT>(y, yv, u[j].t * ldy + u[j].col0, tb.hidden - u[j].col0, vec_ok != 0);
        }
    }
}

// ---- columns

struct ColUnit {
    int64_t t, h;                                   // token (-1: nothing to store) and hidden index
    bool in_table;
    Where at;
    int row, col;                                   // inside the tile
    uint32_t code, E;
};

template <bool ID64, bool BF16OUT, bool SCALE>
__global__ __launch_bounds__(64 * kWaves) void packed_gather_columns_kernel(const void *__restrict__ ids, int64_t tokens, int64_t id_first, Table tb,
                                                                            int64_t chunks, float scale, void *__restrict__ yv, int64_t ldy)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t units = tokens * chunks, waves = (int64_t)gridDim.x * kWaves;
    for (int64_t first = ((int64_t)blockIdx.x * kWaves + wave) * kUnits; first < units; first += waves * kUnits) {
        ColUnit u[kUnits];
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int64_t unit = first + j;
            u[j].t = unit < units ? unit / chunks : -1;
            u[j].h = (unit % chunks) * 64 + lane;
            int64_t id = -1;
            if (u[j].t >= 0 && u[j].h < tb.hidden) id = token_id<ID64>(ids, u[j].t) - id_first;
            else u[j].t = -1;
            u[j].in_table = id >= 0 && id < tb.vocab;
            u[j].row = (int)(u[j].h & 31);
            u[j].col = (int)(id & 31);
            Where w{0, -1};
            if (u[j].in_table && (lane & 31) == 0) w = look_up(tb, (u[j].h >> 5) * tb.tiles_w + (id >> 5));
            u[j].at = share(w, lane & 32);            // lanes 0 and 32 hold the first h of their tiles: inside whenever a later lane is
            if (!u[j].in_table) u[j].at.f = -1;
        }
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int f = u[j].at.f;
            u[j].code = 0u;
            u[j].E = 0u;
            if (f < 0) continue;
            const uint8_t *blob = tb.packed + u[j].at.off;
            const int e = 32 * u[j].row + u[j].col;
            if (f == 0) {
                u[j].code = reinterpret_cast<const uint16_t *>(blob)[e];
                continue;
            }
            u[j].E = blob[2 * u[j].row + (u[j].col >> 4)];
            if (f == 1) u[j].code = blob[kExpBytes + e];
            else if (f == 2) u[j].code = (blob[kExpBytes + (e >> 1)] >> (4 * (e & 1))) & 0xFu;
            else u[j].code = (blob[kExpBytes + (e >> 2)] >> (2 * (e & 3))) & 0x3u;
        }
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            if (u[j].t < 0) continue;
            const int f = u[j].at.f;
            uint32_t word = 0u;
            if (f == 0) word = u[j].code << 16;
            else if (f > 0) word = bfp_code_bits_rt(u[j].code, u[j].E, f == 1 ? 7u : (f == 2 ? 3u : 1u));
            if constexpr (SCALE) {
                if (u[j].in_table) word = scaled_word<BF16OUT>(word, scale);
            }
            const int64_t at = u[j].t * ldy + u[j].h;
            if constexpr (BF16OUT) static_cast<uint16_t *>(yv)[at] = (uint16_t)(word >> 16);
            else static_cast<uint32_t *>(yv)[at] = word;
        }
    }
}

template <bool ID64, bool BF16OUT, bool SCALE>
void launch(bool columns, unsigned blocks, hipStream_t st, const void *ids, int64_t tokens, int64_t id_first, const Table &tb, int64_t chunks,
            float scale, void *y, int64_t ldy, int vec_ok)
{
    if (columns)
        hipLaunchKernelGGL((packed_gather_columns_kernel<ID64, BF16OUT, SCALE>), dim3(blocks), dim3(64 * kWaves), 0, st, ids, tokens, id_first, tb,
                           chunks, scale, y, ldy);
    else
        hipLaunchKernelGGL((packed_gather_rows_kernel<ID64, BF16OUT, SCALE>), dim3(blocks), dim3(64 * kWaves), 0, st, ids, tokens, id_first, tb,
                           chunks, scale, y, ldy, vec_ok);
}

template <bool ID64, bool BF16OUT, typename... A>
void launch_scale(bool has_scale, A... a)
{
    if (has_scale) launch<ID64, BF16OUT, true>(a...);
    else launch<ID64, BF16OUT, false>(a...);
}

template <bool ID64, typename... A>
void launch_out(bool bf16, bool has_scale, A... a)
{
    if (bf16) launch_scale<ID64, true>(has_scale, a...);
    else launch_scale<ID64, false>(has_scale, a...);
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" int mtq_packed_embedding(const void *ids, int id_dtype, int64_t tokens, int64_t id_first, const void *packed, size_t packed_bytes,
                                    const int8_t *map, const uint32_t *offsets, int64_t rows, int64_t cols, int stored, int has_scale, double scale,
                                    void *y, int out_dtype, int64_t ldy, void *stream)
{
    if (!ids || !packed || !map || !offsets || !y) return fail(MTQ_ERR_INVALID, "null argument");
    if (id_dtype != MTQ_IDS_I32 && id_dtype != MTQ_IDS_I64) return fail(MTQ_ERR_INVALID, "id_dtype must be MTQ_IDS_I32 or MTQ_IDS_I64");
    if (out_dtype != MTQ_DTYPE_BF16 && out_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "out_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (stored != MTQ_GATHER_ROWS && stored != MTQ_GATHER_TRANSPOSE)
        return fail(MTQ_ERR_INVALID, "stored must be MTQ_GATHER_ROWS or MTQ_GATHER_TRANSPOSE");
    if (tokens <= 0) return fail(MTQ_ERR_INVALID, "tokens must be positive (an empty ids is handled by the caller)");
    if (tokens > (int64_t)1 << 40) return fail(MTQ_ERR_INVALID, "too many tokens");
    if (rows <= 0 || cols <= 0) return fail(MTQ_ERR_INVALID, "rows and cols must be positive");
    if (rows > (int64_t)1 << 30 || cols > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t tiles_h = (rows + kTile - 1) / kTile, tiles_w = (cols + kTile - 1) / kTile;
    if (tiles_h * tiles_w > (int64_t)1 << 31) return fail(MTQ_ERR_INVALID, "too many tiles for 32-bit offsets");
    const bool columns = stored == MTQ_GATHER_TRANSPOSE;
    const int64_t vocab = columns ? cols : rows, hidden = columns ? rows : cols;
    if (ldy < hidden) return fail(MTQ_ERR_INVALID, "ldy is below the hidden size");
    if (ldy > (int64_t)1 << 40) return fail(MTQ_ERR_INVALID, "ldy too large");
    if (reinterpret_cast<uintptr_t>(packed) % 16 != 0) return fail(MTQ_ERR_INVALID, "packed must be 16-byte aligned");
    if (packed_bytes < (uint64_t)(tiles_h * tiles_w) * blob_bytes(MTQ_FMT_BFP2)) return fail(MTQ_ERR_INVALID, "packed_bytes is smaller than the stream");
    const bool id64 = id_dtype == MTQ_IDS_I64, bf16 = out_dtype == MTQ_DTYPE_BF16;
    if (reinterpret_cast<uintptr_t>(ids) % (id64 ? 8 : 4) != 0) return fail(MTQ_ERR_INVALID, "ids is not aligned to its type");
    if (reinterpret_cast<uintptr_t>(y) % (bf16 ? 2 : 4) != 0) return fail(MTQ_ERR_INVALID, "y is not aligned to its type");
    if (int rc = require_device()) return rc;

    const Table tb{static_cast<const uint8_t *>(packed), (uint64_t)packed_bytes, map, offsets, tiles_w, vocab, hidden};
    // a wave's span of one token: 64 groups of 16 columns (rows), 64 elements (columns)
    const int64_t span = columns ? 64 : 64 * kGroup, chunks = (hidden + span - 1) / span;
    const int64_t units = tokens * chunks, per_block = (int64_t)kWaves * kUnits;
    const unsigned blocks = (unsigned)std::min<int64_t>((units + per_block - 1) / per_block, kMaxBlocks);
    const int64_t esz = bf16 ? 2 : 4;
    const int vec_ok = reinterpret_cast<uintptr_t>(y) % 16 == 0 && (ldy * esz) % 16 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (id64) launch_out<true>(bf16, has_scale != 0, columns, blocks, st, ids, tokens, id_first, tb, chunks, (float)scale, y, ldy, vec_ok);
    else launch_out<false>(bf16, has_scale != 0, columns, blocks, st, ids, tokens, id_first, tb, chunks, (float)scale, y, ldy, vec_ok);
    return check_launch("mtq_packed_embedding");
}
