/* mtq_glu_chunked.h - the grouped skinny GLU and the MoE decode entries with a wave per 32-row chunk.  Part of the C ABI of
 * libmtq_hip.so: mtq.h includes this file at its end, after mtq_moe_decode.h, and a program includes mtq.h.  The entries stand in a
 * header of their own for mtq_moe_decode.h's reason: the prototype sets of mtq.h and of mtq_moe_decode.h are held to fixed lists by the
 * tests that record their refusal ladders; the ladders of the entries below are in tests/test_packed_glu_chunked_host.py. */
#ifndef MTQ_GLU_CHUNKED_H
#define MTQ_GLU_CHUNKED_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ grouped skinny GLU and MoE decode, a wave per 32-row chunk
 * (csrc/mtq_packed.hip).  The walking entries - mtq_packed_glu_skinny_grouped, its *_gather form and mtq_packed_linear_skinny_grouped_combine,
 * each with its matmul twin for (k, n) experts - give a whole group to one wave per tile row, which walks the group's rows in 32-row
 * chunks one after another: a group with many rows is the launch's critical path.  The entries below take their parent's parameters in
 * the parent's order and hand every 32-row chunk to a wave of its own, as mtq_packed_linear_skinny_grouped_chunked does for the plain
 * grouped product: the groups' chunk counts are prefix-summed on the device (cstart[0 .. count]) on the same stream, the main kernel's
 * unit axis is the host's slot bound floor((total_rows + 31 min(count, total_rows)) / 32) instead of count, a wave finds its group by
 * a search of cstart, and a wave whose slot is at or past cstart[count] returns before any other load.
 *
 * mtq_packed_glu_skinny_grouped_chunked / mtq_packed_glu_matmul_skinny_grouped_chunked: mtq_packed_glu_skinny_grouped's parameters.  A
 * unit is (slice, projection, chunk slot, tile row); on its chunk the wave does what the walking wave does on that chunk - the same
 * stream, run and stores of float32 partials to workspace[projection][slice][row][n] at every split.  The reduce takes one workgroup per
 * (chunk slot, 256 columns), thread n walking the chunk's at most 32 rows, and forms g, u and the activation as the walking reduce does:
 * slices ascending, bias last.
 * mtq_packed_glu_skinny_grouped_chunked_gather / mtq_packed_glu_matmul_skinny_grouped_chunked_gather: the *_gather entries' parameters
 * (mtq_moe_decode.h); total_rows = S = tokens * topk; the same src rule, read only at rows inside a clamped group.
 * mtq_packed_linear_skinny_grouped_chunked_combine / mtq_packed_matmul_skinny_grouped_chunked_combine: the *_combine entries' parameters;
 * the plan, then mtq_packed_linear_skinny_grouped_chunked's kernel (its matmul twin's) storing float32 partials to
 * workspace[slice][S][n] at every split, then the *_combine entries' reduce kernel, unchanged.
 *
 * Workspace: the plan region, (count + 1) * 4 bytes rounded up to 16, at the head, then the parent's workspace; each
 * *_workspace_bytes function returns the parent's size function's answer plus the plan region, (size_t)-1 where the parent's does.  16-byte
 * aligned, nothing in it needs initialising, and a null, misaligned or short workspace is refused at every split.  The effective split
 * is the parent's for the same arguments, so split = 0 means the same on both.
 * Refused: whatever the parent refuses of the same operands, in the parent's order and words - MTQ_ERR_INVALID before a device is
 * looked for, MTQ_ERR_UNSUPPORTED for an unknown act.
 *
 * Bit contract.  For nondecreasing group_rows, y equals the walking parent's y bit for bit at the same `split`, in both output types,
 * with or without biases, base or dropped slots.  Rows of no group are not written.  Nothing outside y and the workspace is written
 * and nothing outside the operands is read, whatever group_rows, src or row_of hold.  Decreasing group_rows that clamp to overlapping
 * groups leave those groups' rows (for the *_combine entries: the tokens whose slots name them) unspecified inside the allocation, as
 * with mtq_packed_linear_skinny_grouped_chunked: chunks past the slot bound are not computed.
 * Deterministic: cstart is written with plain stores by one workgroup; no atomics, no counters, nothing waits on another workgroup and
 * nothing is read back to the host.
 *
 * All twelve symbols are optional: a build of this version may lack them. */
size_t mtq_packed_glu_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                          const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                          const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                          const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                          const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y, int out_dtype,
                                          int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_glu_matmul_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_matmul_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                                 const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps,
                                                 const uint32_t *gate_offsets, const uint64_t *gate_bases, const void *up_packed,
                                                 size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                 int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb, int act,
                                                 void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                                 void *stream);
size_t mtq_packed_glu_skinny_grouped_chunked_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_skinny_grouped_chunked_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx, const int32_t *src,
                                                 const int32_t *group_rows, const void *gate_packed, size_t gate_bytes,
                                                 const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                                 const void *up_packed, size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets,
                                                 const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                                 const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split,
                                                 void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_glu_matmul_skinny_grouped_chunked_gather_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_matmul_skinny_grouped_chunked_gather(const void *x, int64_t tokens, int64_t topk, int64_t k, int64_t ldx,
                                                        const int32_t *src, const int32_t *group_rows, const void *gate_packed,
                                                        size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                                        const uint64_t *gate_bases, const void *up_packed, size_t up_bytes,
                                                        const int8_t *up_maps, const uint32_t *up_offsets, const uint64_t *up_bases,
                                                        int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb,
                                                        int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                                        size_t workspace_bytes, void *stream);
size_t mtq_packed_linear_skinny_grouped_chunked_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_linear_skinny_grouped_chunked_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                                     size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                                     int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                                     int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens,
                                                     int64_t topk, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                                     size_t workspace_bytes, void *stream);
size_t mtq_packed_matmul_skinny_grouped_chunked_combine_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_matmul_skinny_grouped_chunked_combine(const void *x, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                                     size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                                                     int64_t count, int64_t n, int expert_dtype, const int32_t *row_of, const float *weights,
                                                     int64_t ldw, const void *base, int base_dtype, int64_t ldbase, int64_t tokens,
                                                     int64_t topk, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTQ_GLU_CHUNKED_H */
