/* mtq_moe_decode.h - the decode route of an MoE layer on packed experts without the staging copies.  Part of the C ABI of libmtq_hip.so:
 * mtq.h includes this file at its end, and a program includes mtq.h.  The entries stand in a header of their own because mtq.h's set
 * of mtq_packed_* prototypes is the set whose refusal ladders tests/golden/packed_refusals.json records, name for name; the ladders of
 * the entries below are in tests/test_packed_moe_fused_host.py. */
#ifndef MTQ_MOE_DECODE_H
#define MTQ_MOE_DECODE_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ MoE decode without the staging copies (csrc/mtq_packed.hip)
 * The decode route of an MoE layer with the dispatch inside the gated product's X loads and the combine inside the down projection's
 * reduce: mtq_moe_plan, a *_gather entry, a *_combine entry - five launches at every split, and neither the dispatched (S, k) copy of
 * x nor the experts' (S, n) rows ever exist.  Each entry has a twin for (k, n) experts (the *_matmul_* names) with the same arguments,
 * checks and workspace.  S = tokens * topk is formed by the entries; mtq_moe_plan's limits on tokens, topk and S apply.
 *
 * mtq_packed_glu_skinny_grouped_gather / mtq_packed_glu_matmul_skinny_grouped_gather: mtq_packed_glu_skinny_grouped's operands (its
 * matmul twin's) with x the TOKEN matrix (tokens, k) bf16 at pitch ldx, src int32 [S] (the plan's) and total_rows = S.  Row r of the
 * matrix the experts multiply is x[src[r] / topk] when 0 <= src[r] < S, else a row of +0: mtq_moe_dispatch's rule.  The kernel is the
 * grouped skinny GLU wave; a lane looks src[row] up once per 32-row chunk and reads its X groups from that token's row (16-byte
 * loads under the same condition on x and ldx as before).  Whatever src holds, no row of x at or past `tokens` is read; src is read
 * only at rows inside a clamped group.  Workspace, split rule and reduce kernel are mtq_packed_glu_skinny_grouped's, and the
 * *_gather_workspace_bytes functions return its size function's answer for (S, count, n, k, split).
 * Bit contract: y equals bit for bit (1) mtq_moe_dispatch into a contiguous xs, (2) mtq_packed_glu_skinny_grouped (its matmul twin)
 * on xs at the same `split`, in both output types, with or without biases.  Rows of y of no group are not written.
 * Refused (MTQ_ERR_INVALID before a device is looked for): whatever mtq_moe_dispatch or mtq_packed_glu_skinny_grouped refuses of the
 * same operands - a null pointer, tokens / topk / S outside the limits, ldx < k or above 2^40, x or src not aligned to its type, and
 * the grouped entry's own checks; an unknown act is MTQ_ERR_UNSUPPORTED.
 *
 * mtq_packed_linear_skinny_grouped_combine / mtq_packed_matmul_skinny_grouped_combine: x (S, k) bf16 at pitch ldx (the gated product's
 * rows, in expert order), group_rows, the arena and its tables as mtq_packed_linear_skinny_grouped takes them, without bias; then
 * mtq_moe_combine's operands: row_of int32 [S], weights float32 (tokens, topk) at pitch ldw, base NULL or (tokens, n) bf16 / float32
 * (base_dtype, ldbase), and y (tokens, n) in out_dtype at pitch ldy.  expert_dtype (MTQ_DTYPE_F32 or MTQ_DTYPE_BF16) is the rounding
 * the experts' rows would have had as a matrix of that type.
 * The main kernel is the grouped skinny wave and stores float32 partial sums to workspace[slice][S][n] at every split, an effective
 * split of 1 included; the workspace is max(split_eff, 1) * S * n * 4 bytes rounded up to 16, never empty, and nothing in it needs
 * initialising.  The reduce kernel, one workgroup per (token, 256 columns): acc starts at (float) base[t][c] or +0; for j = 0 ..
 * topk - 1 in order, with r = row_of[t * topk + j] inside [0, S): v = ((p0 + p1) + ... + p_{eff-1}) + 0.0f, slices ascending (the
 * + 0.0f is the grouped entry's bias add without a bias: a -0 sum becomes +0); with a bf16 expert_dtype v is rounded to bf16 once and
 * widened; acc = fl32(acc + fl32(w[t][j] * v)), product and sum rounded separately.  A slot with r outside [0, S) is skipped, never
 * multiplied by zero, and rows of the workspace that no kept slot names are never read.  y is stored once, one rounding for bf16.
 * Bit contract: y equals bit for bit (1) mtq_packed_linear_skinny_grouped (its matmul twin) without bias into expert_dtype at the
 * same `split`, (2) mtq_moe_combine of those rows - in both output types, with each kind of base, with dropped slots.
 * Refused (MTQ_ERR_INVALID before a device is looked for): whatever either of those entries refuses of the same operands.
 * Deterministic: no atomics, no counters, nothing waits on another workgroup.
 *
 * All eight symbols are optional: a build of this version may lack them. */
size_t mtq_packed_glu_skinny_grouped_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_skinny_grouped_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                         const int32_t *group_rows, const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                         const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed, size_t up_bytes,
                                         const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                         const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y, int out_dtype,
                                         int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_glu_matmul_skinny_grouped_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_matmul_skinny_grouped_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                                const int32_t *group_rows, const void *gate_packed, size_t gate_bytes,
                                                const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                                const void *up_packed, size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets,
                                                const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                                const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split,
                                                void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_linear_skinny_grouped_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_linear_skinny_grouped_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                             size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                             int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                             int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                             void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                             void *stream);
size_t mtq_packed_matmul_skinny_grouped_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_matmul_skinny_grouped_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                             size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                             int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                             int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk,
                                             void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTQ_MOE_DECODE_H */
