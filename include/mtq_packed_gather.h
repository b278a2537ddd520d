/* mtq_packed_gather.h - the input embedding over a packed table: token rows gathered straight from the packed stream, without an
 * unpacked copy of the table.  Part of the C ABI of libmtq_hip.so: mtq.h includes this file at its end, after mtq_wide_split.h, and a
 * program includes mtq.h.  The entry stands in a header of its own for mtq_packed_pre.h's reason; what it refuses is in
 * tests/test_packed_embedding_host.py. */
#ifndef MTQ_PACKED_GATHER_H
#define MTQ_PACKED_GATHER_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* `stored`: which way round the table lies in the stream (the index.json words "rows" and "transpose"). */
enum { MTQ_GATHER_ROWS = 0, MTQ_GATHER_TRANSPOSE = 1 };

/* mtq_packed_embedding: y[i, :] = table[ids[i] - id_first, :] (· scale) for `tokens` ids, the table read from its packed stream
 * ("PACKED mixed-tile weights" in mtq.h; nothing about the bytes changes).
 *
 * rows x cols is the shape of the STORED stream, map and offsets over its tile grid: MTQ_GATHER_ROWS, the (vocab, hidden) table itself,
 * token i its row i; MTQ_GATHER_TRANSPOSE, the (hidden, vocab) transpose as mtq_pack_tiles_transposed writes it, token i its column i.
 * ids: device, contiguous, int32 or int64 (id_dtype MTQ_IDS_I32 / MTQ_IDS_I64, read in their own width).  id_first is subtracted from
 * every id in 64 bits before the lookup (a vocabulary-parallel rank holds rows [id_first, id_first + vocab)); an id outside [0, vocab)
 * after that gives a row of +0, mtq_moe_plan's convention for another rank's experts, and a padding index.
 * y: tokens x hidden, out_dtype MTQ_DTYPE_F32 or MTQ_DTYPE_BF16, row pitch ldy >= hidden; nothing is stored outside tokens x hidden.
 *
 * Kernels (csrc/mtq_packed_gather.hip).  Rows: a lane is one 16-value group of one token's row, a wave 64 consecutive groups (1024
 * columns, 32 tiles of one tile row).  With gi = 2 * (id & 31) + half, the row's slice of tile (id >> 5, tc) is
 *     bf16  32 bytes at 32 * gi                          bfp8  16 bytes at 64 + 16 * gi, exponent blob[gi]
 *     bfp4   8 bytes at 64 + 8 * gi, exponent blob[gi]   bfp2   4 bytes at 64 + 4 * gi,  exponent blob[gi]
 * and every lane stores 32 contiguous bytes of bf16 (64 of f32).  A wave holds four units at a time and issues the id, map and offset
 * loads of all of them before any code load, and all code loads before it decodes; the two lanes of a tile share one lookup.
 * Transpose: a lane is one element, hidden index h, row h & 31 of tile (h >> 5, id >> 5): the exponent byte
 * blob[2 * row + ((id & 31) >> 4)] and the code at element e = 32 * row + (id & 31) - a byte, a nibble, a crumb or a bf16 half-word.
 * Each element costs a 32-byte sector of the stream, which is inherent to a column of a row-major blob; consecutive lanes store
 * consecutive outputs.  The grid is capped at 2048 workgroups of four waves; more work loops.
 *
 * Guards.  A tile whose map code is outside 0..3, or whose blob passes packed_bytes, reads as zeros (mtq_unpack_tiles's guard, taken
 * before the blob is touched).
 *
 * Bit contract.  has_scale == 0: no multiply; y is bit for bit the rows ids[i] - id_first of what mtq_unpack_tiles writes for the
 * stream (the columns, for MTQ_GATHER_TRANSPOSE), in both output types.  has_scale != 0: y = value * (float)scale, the product formed
 * in float32 and, for a bf16 y, rounded once, to nearest even; a row outside the table stays +0.  No atomics, no workspace, no LDS: two
 * calls give the same bits.  Asynchronous on `stream`.
 *
 * Refused, MTQ_ERR_INVALID with a message before a device is looked for: a null ids, packed, map, offsets or y; an id_dtype, out_dtype
 * or stored that is none of the above; tokens, rows or cols <= 0; ldy below the hidden size; a stream that is not 16-byte aligned; a
 * buffer below 320 bytes per tile; ids or y not aligned to their types.  With no device the call returns MTQ_ERR_NO_DEVICE.  Optional symbol. */
int mtq_packed_embedding(const void *ids, int id_dtype, int64_t tokens, int64_t id_first, const void *packed, size_t packed_bytes,
                         const int8_t *map, const uint32_t *offsets, int64_t rows, int64_t cols, int stored, int has_scale, double scale,
                         void *y, int out_dtype, int64_t ldy, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTQ_PACKED_GATHER_H */
