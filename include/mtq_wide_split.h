/* mtq_wide_split.h - the wide-block products with a split over K, for the mid range of m where the wide block's 128 x 128 blocks alone
 * leave most of the chip idle.  Part of the C ABI of libmtq_hip.so: mtq.h includes this file at its end, after mtq_grouped_pre.h, and a
 * program includes mtq.h.  The entries stand in a header of their own for mtq_packed_pre.h's reason; what they refuse is in
 * tests/test_packed_wide_split_host.py. */
#ifndef MTQ_WIDE_SPLIT_H
#define MTQ_WIDE_SPLIT_H
#include "mtq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mtq_packed_linear_wide_split: mtq_packed_linear_wide's product Y = X W^T + b for an (n, k) packed weight, its parameters first, then
 * split, workspace, workspace_bytes and stream as mtq_packed_linear_skinny has them.  mtq_packed_matmul_wide_split: the same for a
 * (k, n) packed matrix, Y = X P + b, mtq_packed_matmul_wide's parameters first.
 *
 * Split.  With steps = ceil(k / 64) the effective split is S = min(split, steps); slice s owns the whole steps
 * [s steps / S, (s + 1) steps / S) of K (integer division), so every 16-wide MFMA block and every BFP group lies inside one slice.
 * split 0 is the library's choice, a pure function of (m, n, k): the most slices with which the 128 x 128 blocks times S stay within
 * the chip's workgroup slots (two per CU, 512), no slice shorter than 4 steps, and 1 wherever the blocks alone take more than half of
 * the slots.
 * mtq_packed_wide_split is that rule as a HOST function: the effective split, or -1 with the message set (m <= 0, an n or k the tile
 * grid refuses, a negative split).
 *
 * Workspace.  S > 1 needs S * m * n * 4 bytes rounded up to 16, 16-byte aligned, on the device: the f32 partials ws[s][m][n].  S == 1
 * needs none and touches none.  The size functions return that size, 0 at S == 1, (size_t)-1 on refused arguments.
 *
 * Kernel.  packed_wide_split_kernel runs blocks * S workgroups, the column block fastest, then the row block, the slice slowest; a
 * workgroup is the wide kernel's 128 x 128 block over ONE slice, in the wide kernel's order inside it, and stores its accumulators as
 * f32 with plain stores.  No atomics, no counters, nothing waits on another workgroup.  skinny_reduce_kernel then forms
 * Y = ((p0 + p1) + ... + p_{S-1}) + b: ascending slices, the bias last in f32, one rounding for a bf16 Y.  At S == 1 the call launches
 * mtq_packed_linear_wide's kernel itself.
 *
 * Bit contract.  At an effective split of 1 the result is mtq_packed_linear_wide's (mtq_packed_matmul_wide's) bit for bit.  At any
 * split the same inputs give the same bits.  Results under different splits may differ in the last bits.  The matmul entry at split S
 * equals the linear entry at split S on the all-bf16 packing of unpack(P)^T.
 *
 * Refused, MTQ_ERR_INVALID before a device is looked for: what mtq_packed_linear_wide refuses, with its code and message; then a
 * negative split; blocks * S above INT32_MAX; a null, misaligned or short workspace where S > 1.  Optional symbols. */
int mtq_packed_wide_split(int64_t m, int64_t n, int64_t k, int split);
size_t mtq_packed_linear_wide_split_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
size_t mtq_packed_matmul_wide_split_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
int mtq_packed_linear_wide_split(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes,
                                 const int8_t *map, const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype,
                                 int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);
int mtq_packed_matmul_wide_split(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes,
                                 const int8_t *map, const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype,
                                 int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTQ_WIDE_SPLIT_H */
