/* mtq_grouped_pre.h - the grouped skinny products of an MoE layer's decode route with the activation prologue (block Hadamard rotation,
 * per-expert channel shifts) inside the kernel.  Part of the C ABI of libmtq_hip.so: mtq.h includes this file at its end, after
 * mtq_packed_pre.h, and a program includes mtq.h.  The entries stand in a header of their own for mtq_packed_pre.h's reason; what they
 * refuse is in tests/test_packed_grouped_prologue_host.py. */
#ifndef MTQ_GROUPED_PRE_H
#define MTQ_GROUPED_PRE_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The grouped skinny entries for (n, k) experts (the walking kernel) with mtq_packed_pre.h's operand, per row r of expert e:
 *   X'  = mtq_hadamard_rows(x_row, block) as bf16 (float32 butterflies, stride 1 first, one multiply by float32(2^(-log2(block)/2)), RNE),
 *         X' = x_row for block 0;
 *   X'' = bf16 RNE of the exact X'[j] * 2^-in_exponents[e][j] (an exponent-field subtract while the result is normal; Inf and NaN stay),
 *         X'' = X' for a null in_exponents.
 * block: 0, or a power of two in [32, 1024] that divides k.  in_exponents: NULL, or count rows of k bytes in 0..7 on the device (the low
 * three bits of a byte count), row e the shifts of expert e - shared by its gate and up -, 16-byte aligned, and with it k % 16 == 0 so
 * that every row is.
 *
 * mtq_packed_glu_skinny_grouped_pre: mtq_packed_glu_skinny_grouped_gather's parameters, block and in_exponents behind group_rows.  src
 * non-NULL: x is the (tokens, k) token matrix and row r is x[src[r] / topk] or a row of +0, that entry's rule (mtq_moe_glu's case).
 * src NULL: x holds the tokens * topk rows in expert order themselves (pass topk = 1; mtq_packed_glu_skinny_grouped's case).
 *
 * mtq_packed_linear_skinny_grouped_pre: mtq_packed_linear_skinny_grouped_combine's parameters, block and in_exponents behind
 * group_rows.  row_of and weights non-NULL: that entry's result, y (tokens, n).  row_of, weights and base all NULL: the plain grouped
 * product without bias, y (tokens * topk, n) in out_dtype (pass topk = 1), expert_dtype ignored - mtq_packed_linear_skinny_grouped's
 * result; one of row_of and weights alone, or a base without them, is refused.
 *
 * Bit contract: at the same EFFECTIVE split, y equals bit for bit the unfused grouped entry's result on an X'' formed by
 * mtq_hadamard_rows and an exact per-row shift - the same MFMA sequence in ascending K per 32-row chunk, the same workspace layout, the
 * unfused entry's own reduce kernel (plain, gated or combine), the biases and the combine last.
 *
 * Kernel: a workgroup is four waves on four tile rows (the gated entry: two tile rows of both projections) of ONE expert in ONE K
 * slice.  It walks the expert's clamped rows in 32-row chunks and each chunk in panels of P columns, P the largest multiple of block up
 * to 1024 that divides the slice.  Per chunk a lane looks its row's src up once; per panel the waves load the live rows (through src
 * when gathering), rotate them in registers (a lane owns 16 columns; register, DPP and permlane-swap stages as mtq_hadamard_rows),
 * subtract the expert's exponents and store bf16 into a swizzled LDS image of at most 32 x 1024 bf16; one barrier publishes the panel,
 * every wave takes its MFMA X operands from it, a second barrier frees it.  All four waves form the chunk and panel counts from the same
 * clamped group_rows[e], group_rows[e + 1]; a wave whose tile row is past n / 32 rotates and meets every barrier, and the workgroup of an
 * expert without rows leaves as a whole before the first.  block 0: no LDS and no barrier, a lane shifts its own words after its load.
 * Deterministic: no atomics.
 *
 * Split.  With a block the slices must be equal and made of whole blocks: an explicit split s (clamped to the tile columns) needs
 * tiles_w % s == 0 and (tiles_w / s) % (block / 32) == 0, else MTQ_ERR_INVALID; split 0 is the largest such s up to the unfused grouped
 * entry's own choice for (total_rows, count, n, k).  block 0 keeps the unfused rule.  mtq_packed_grouped_pre_split is that rule as a
 * HOST function: the effective split, or -1 with the message set.  The size functions return the unfused grouped entries' sizes at that
 * effective split ((size_t)-1 on refused arguments): mtq_packed_glu_skinny_grouped_workspace_bytes', and for the linear entry
 * mtq_packed_linear_skinny_grouped_combine_workspace_bytes' (combine != 0) or mtq_packed_linear_skinny_grouped_workspace_bytes'.
 *
 * Refused besides what the unfused entries refuse, MTQ_ERR_INVALID before a device is looked for: a block that is not 0 or a power of
 * two in [32, 1024], k % block != 0, a split that breaks the rule, block 0 with a null in_exponents (nothing to fuse), a misaligned
 * in_exponents, in_exponents with k % 16 != 0.  Optional symbols. */
int mtq_packed_grouped_pre_split(int64_t count, int64_t total_rows, int64_t n, int64_t k, int64_t block, int split);
size_t mtq_packed_glu_skinny_grouped_pre_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int64_t block, int split);
int mtq_packed_glu_skinny_grouped_pre(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                      const int32_t *group_rows, int64_t block, const uint8_t *in_exponents, const void *gate_packed,
                                      size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                      const void *up_packed, size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets,
                                      const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate, const float *bias_up,
                                      int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                      size_t workspace_bytes, void *stream);
size_t mtq_packed_linear_skinny_grouped_pre_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int64_t block, int split,
                                                            int combine);
int mtq_packed_linear_skinny_grouped_pre(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, int64_t block,
                                         const uint8_t *in_exponents, const void *packed, size_t packed_bytes, const int8_t *maps,
                                         const uint32_t *offsets, const uint64_t *bases, int64_t count, int64_t n, int expert_dtype,
                                         const int32_t *row_of, const float *weights, int64_t ldw, const void *base, int base_dtype,
                                         int64_t ldbase, int64_t tokens, int64_t topk, void *y, int out_dtype, int64_t ldy, int split,
                                         void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTQ_GROUPED_PRE_H */
