/* mtq_packed_pre.h - the skinny packed products with the activation prologue (block Hadamard rotation, per-channel shifts) inside the
 * kernel.  Part of the C ABI of libmtq_hip.so: mtq.h includes this file at its end, after mtq_glu_chunked.h, and a program includes
 * mtq.h.  The entries stand in a header of their own for mtq_glu_chunked.h's reason: the prototype set of mtq.h is held to a fixed
 * list by the tests that record its refusal ladders; what these entries refuse is in tests/test_packed_prologue_host.py. */
#ifndef MTQ_PACKED_PRE_H
#define MTQ_PACKED_PRE_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mtq_packed_linear_skinny and mtq_packed_glu_skinny with the activation transform of a rotated or channel-shifted weight inside the
 * kernel: the product is taken with X'' in place of x, where
 *   X'  = mtq_hadamard_rows(x, block) as bf16 (float32 butterflies, stride 1 first, one multiply by float32(2^(-log2(block)/2)), RNE),
 *         X' = x for block 0;
 *   X'' = bf16 RNE of the exact X'[., j] * 2^-in_exponents[j] (an exponent-field subtract while the result is normal; Inf and NaN stay),
 *         X'' = X' for a null in_exponents.
 * block: 0, or a power of two in [32, 1024] that divides k.  in_exponents: NULL, or k bytes in 0..7 on the device, 16-byte aligned (the
 * low three bits of a byte count).  Every other parameter is the unfused entry's, in its order.
 *
 * Bit contract: at the same EFFECTIVE split, y equals bit for bit the unfused entry's result on an X'' formed by mtq_hadamard_rows and
 * an exact shift - the same MFMA sequence in ascending K, the same workspace layout, the same reduce, the bias last.
 *
 * Kernel: a workgroup covers four tile rows (the gated entry: two tile rows of both projections) of one K slice and walks it in panels
 * of P columns, P the largest multiple of block up to 1024 that divides the slice.  Per panel its waves rotate the m live rows in
 * registers (a lane owns 16 columns; register, DPP and permlane-swap stages as mtq_hadamard_rows), shift, and store them into an LDS
 * image of m x P bf16 (at most 64 KB) with its 32-byte pieces swizzled by the row; one barrier publishes the panel, the skinny wave takes
 * its X operands from it, a second barrier frees it.  block 0: no LDS and no barrier, the lane shifts its own words after its load.
 *
 * Split.  A slice must be whole blocks and the slices equal: with a block, an explicit split s (clamped to the tile columns as in the
 * unfused entry) needs tiles_w % s == 0 and (tiles_w / s) % (block / 32) == 0, else MTQ_ERR_INVALID; split 0 is the largest s up to
 * the unfused entry's own choice that satisfies both.  block 0 keeps the unfused rule.  mtq_packed_skinny_pre_split is that rule as a
 * HOST function: the effective split of (m, n, k, block, split), or -1 (with the message set) for arguments the entries refuse.  The
 * workspace sizes are the unfused entries' at that effective split ((size_t)-1 on refused arguments).
 *
 * Refused besides what the unfused entries refuse, MTQ_ERR_INVALID before a device is looked for: a block that is not 0 or a power of
 * two from 32 on, k % block != 0, block > 1024 (no panel fits the image), a split that breaks the rule above, block 0 with a null
 * in_exponents (nothing to fuse), a misaligned in_exponents.  Deterministic: no atomics.  Optional symbols. */
int mtq_packed_skinny_pre_split(int64_t m, int64_t n, int64_t k, int64_t block, int split);
size_t mtq_packed_linear_skinny_pre_workspace_bytes(int64_t m, int64_t n, int64_t k, int64_t block, int split);
int mtq_packed_linear_skinny_pre(const void *x, int64_t m, int64_t k, int64_t ldx, int64_t block, const uint8_t *in_exponents,
                                 const void *packed, size_t packed_bytes, const int8_t *map, const uint32_t *offsets, int64_t n,
                                 const float *bias, void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t mtq_packed_glu_skinny_pre_workspace_bytes(int64_t m, int64_t n, int64_t k, int64_t block, int split);
int mtq_packed_glu_skinny_pre(const void *x, int64_t m, int64_t k, int64_t ldx, int64_t block, const uint8_t *in_exponents,
                              const void *gate_packed, size_t gate_bytes, const int8_t *gate_map, const uint32_t *gate_offsets,
                              const void *up_packed, size_t up_bytes, const int8_t *up_map, const uint32_t *up_offsets, int64_t n,
                              const float *bias_gate, const float *bias_up, int act, void *y, int out_dtype, int64_t ldy, int split,
                              void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
