/*
 * mtq.h — C ABI of libmtq_hip.so, the MI355X (gfx950) backend of the mixed-tile
 * quantization-format search path.
 *
 * The reference (johanna-rock/quantization_analysis) is pure Python and has no FFI; its seam for
 * this path is the `--backend` selector (wq:57-62) → `Quantizer.quantize` (compression_algorithms/
 * quantizer.py:13-34) and `CompressionAlgorithm.run` (compression_algorithms/base.py:36-44).  Each
 * entry point below names the reference code it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (`stream` is a hipStream_t passed as void*,
 *     NULL = the default stream).
 *   - pointers named x / y / stats / map in the DEVICE section are device pointers owned by the caller;
 *     calls are asynchronous on `stream`.  Pointers in the HOST section are host pointers.
 *   - every function returns MTQ_OK (0) or a negative mtq_status; mtq_last_error() gives a
 *     thread-local message.  Nothing throws across the boundary.  There is NO CPU fallback: device
 *     entry points fail with MTQ_ERR_NO_DEVICE when no gfx950 device is usable.
 *   - matrices are row-major (rows × cols) with a leading dimension `ld` in ELEMENTS; this is the 2-D
 *     flatten of compression_algorithms/tile_utils.py:91-107 (a 1-D vector of n elements is passed as
 *     its zero-filled ceil(n/32) × 32 matrix, an N-D tensor as prod(shape[:-1]) × shape[-1]).
 *     32×32 tiles are numbered tile = tr * tiles_w + tc (mixed_tile_greedy.py:89-93); elements outside
 *     rows × cols read as +0.0 (tile_utils.py:109-113).
 */
#ifndef MTQ_H
#define MTQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTQ_VERSION 143 /* 0.1.4.11 (optional symbols as well, so the number stays 143): + mtq_tile_sq_error_batched, mtq_budget_allocate_device / _scratch_bytes; 0.1.4.10 (optional symbols as well, so the number stays 143): + mtq_pack_tiles_transposed_batched, mtq_unpack_tiles_transposed_batched; 0.1.4.9 (optional symbols as well): + mtq_packed_tile_bytes, mtq_packed_offsets, mtq_pack_tiles, mtq_unpack_tiles, mtq_packed_linear; 0.1.4.8 (optional symbols as well): + mtq_output_error_transposed, mtq_tile_error_tables_transposed; 0.1.4.7 (optional symbols as well): + mtq_gram_full / _scratch_doubles, mtq_gptq_sweep / _scratch_doubles; 0.1.4.6 (optional symbols as well): + mtq_gram_blocks / _scratch_doubles, mtq_tile_error_tables; 0.1.4.5 (optional symbols as well): + mtq_quantize_rows_bf16, mtq_output_error_qx; 0.1.4.4 (the number stays 143: its additions are optional symbols, found by name): + mtq_fp4_proxy_sums / _scratch_doubles, MTQ_FMT_MXFP4 / MTQ_FMT_NVFP4 in mtq_quantize; 0.1.4.3: + ragged batches (MtqMatrix, mtq_tile_stats_ragged, mtq_threshold_enqueue_ragged / _columns_ragged); 0.1.4.2: - chain records, + mtq_threshold_enqueue / _columns; 0.1.4.1: + partial / listed K1 (mtq_tile_stats_partial, mtq_tile_stats_listed), the search in phases with shared visiting orders, mtq_shutdown, mtq_knife_tiles_device */

typedef enum {
    MTQ_OK = 0,
    MTQ_ERR_INVALID = -1,     /* bad argument (shape, dtype, mask, alignment, null pointer) */
    MTQ_ERR_HIP = -2,         /* a HIP runtime call failed; message carries hipGetErrorString */
    MTQ_ERR_NO_DEVICE = -3,   /* no usable gfx950 device */
    MTQ_ERR_UNSUPPORTED = -4  /* recognised but not built (e.g. unknown format code) */
} mtq_status;

/* input element types */
enum { MTQ_DTYPE_BF16 = 0, MTQ_DTYPE_F32 = 1 };

/* format codes = index into MIXED_TILE_FORMATS (tile_utils.py:8) = value stored in assignment maps;
 * FP0 (quantization_formats.py:167-168) and the scalar MXFP4 / NVFP4 proxies (:174-183,257-278) are quantize-only: mtq_quantize
 * takes them, every record and map entry point refuses them. */
enum { MTQ_FMT_BF16 = 0, MTQ_FMT_BFP8 = 1, MTQ_FMT_BFP4 = 2, MTQ_FMT_BFP2 = 3, MTQ_FMT_FP0 = 4, MTQ_FMT_MXFP4 = 5, MTQ_FMT_NVFP4 = 6 };
#define MTQ_NUM_TILE_FORMATS 4
#define MTQ_MASK_ALL 0xFu
/* HOST functions only: "the records hold no bf16 slot; the bf16 candidate is the identity" — true for bf16 STORAGE, where
 * K1's bf16 slot is [Σx, Σx², Σx², |Σx|·0, |Σx|·0].  Set together with a mask WITHOUT bit 0 (records written by K1 for
 * mask & 0xE: 17 instead of 22 doubles per tile cross PCIe); format 0 is then synthesised from Σx, Σx² on the host. */
#define MTQ_MASK_BF16_IDENTITY 0x10u
/* mtq_greedy_* with metric pcc only: "slim" records [Σx, Σx², {Σy, Σy², Σxy} per format bit] — 3 instead of 5 doubles per
 * format (written by mtq_pack_slim_records from K1's records).  Σ|x−y| and max|x−y| feed no pcc decision except the
 * degenerate zero-variance case: a scan that reaches it fails with MTQ_ERR_UNSUPPORTED and the caller repeats that tensor
 * with full records; the mae / atol columns of the result come from mtq_column_sums_device on the full device records. */
#define MTQ_MASK_SLIM 0x20u

/* metrics (compression_algorithms/metrics.py:19-39) */
enum { MTQ_METRIC_PCC = 0, MTQ_METRIC_MAE = 1, MTQ_METRIC_ATOL = 2 };

/* ------------------------------------------------------------------ library */

int mtq_version(void);
const char *mtq_last_error(void);
/* Number of visible HIP devices; MTQ_ERR_NO_DEVICE if the runtime reports none. */
int mtq_device_count(int *count);
/* Releases what the library keeps between calls: joins the scan threads, drains the devices it used and frees its device tables and
 * events.  Idempotent; the library sets itself up again on the next call that needs any of it.  Nothing of this is ever done from a
 * static destructor: call it before the process tears the HIP runtime down (the Python binding registers it with atexit). */
int mtq_shutdown(void);

/* ------------------------------------------------------------------ DEVICE: kernels */

/* Doubles per tile record for a format mask: 2 + 5 * popcount(mask & 0xF); 2 + 3 * popcount under MTQ_MASK_SLIM. */
size_t mtq_stats_record_doubles(uint32_t fmt_mask);

/*
 * K1 tile_stats — fused BFP quantize + per-tile reduction; y never leaves registers.
 * Replaces, per candidate format, quantization_formats.py:84-164 (via quantizer.py:34) plus the
 * per-tile sums of mixed_tile_greedy.py:147-174,192-220,245-254,288-291,313-318 and is the input of the
 * per-tile scores of tile_utils.py:46-57.
 *
 * stats[tile][0..1] = Σx, Σx²; then for each bit set in fmt_mask (ascending: bf16, bfp8, bfp4, bfp2)
 * five doubles Σy, Σy², Σxy, Σ|x−y|, max|x−y|.  Every term is the float32 expression the reference
 * forms (x*x, y*y, x*y, |x−y|) summed in float64; summation order: inside a shared-exponent group the
 * elements within 14 binades of the shared exponent sequentially, the others (zeros included) sequentially,
 * then main + tail; the 4 groups of a row pair (rows 2j, 2j+1) sequentially, the 16 row pairs of a
 * tile by a balanced binary tree over j.
 * Sums run over the zero-padded 1024 elements (pads contribute exactly 0).
 */
int mtq_tile_stats(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld,
                   uint32_t fmt_mask, double *stats, void *stream);

/*
 * Same kernel over `count` equally shaped matrices at x + i*stride_elems (one launch);
 * stats holds count × tiles × record doubles.  Used for model-sized streams of tensors.
 */
int mtq_tile_stats_batched(const void *x, int in_dtype, int64_t count, int64_t stride_elems,
                           int64_t rows, int64_t cols, int64_t ld,
                           uint32_t fmt_mask, double *stats, void *stream);

/*
 * K1 with part of the record left for later (round 3) — same records, same layout (`layout_mask` names the slots that exist), but only
 * the five statistics of the formats in `full_mask` and Σy, Σy², Σxy of the formats in `sums_mask` are promised; every other statistic of
 * the layout is UNSPECIFIED afterwards (the LDS-staged bf16 kernel of csrc/mtq_fast.hip leaves NaN there, the other routes write the whole record).
 * Σx, Σx² are always written.  What the greedy search needs of a format before any tile has ended up in it is Σy, Σy², Σxy
 * (mixed_tile_greedy.py:245-261), and it only looks at format p for the tiles that accepted every earlier format (:227-231): the
 * streamed driver evaluates the last format of the list — and Σ|x−y|, max|x−y| of the one before it — for those tiles alone
 * (mtq_tile_stats_listed) between the search's last two passes.  full_mask and sums_mask are disjoint subsets of layout_mask.
 */
int mtq_tile_stats_partial(const void *x, int in_dtype, int64_t count, int64_t stride_elems,
                           int64_t rows, int64_t cols, int64_t ld,
                           uint32_t layout_mask, uint32_t full_mask, uint32_t sums_mask, double *stats, void *stream);

/* mtq_tile_stats_partial as two launches the caller places itself (bf16 storage in whole 32x128 units with 16-byte aligned rows;
 * MTQ_ERR_UNSUPPORTED otherwise): _begin launches the LDS-staged bf16 kernel alone — it resets its own unit counters, and stores *launch_id
 * (returned to the host) into the device word *mark if it meets a tile it cannot take; _end, given that id, recomputes those tiles by the
 * literal route (it returns at once when *mark holds another value).  The records are complete behind _end.  The streamed driver puts
 * _begin on its K1 stream, where nothing then sits between two K1 launches, and _end on the batch's search stream. */
int mtq_tile_stats_partial_begin(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                 uint32_t layout_mask, uint32_t full_mask, uint32_t sums_mask, double *stats, uint32_t *mark,
                                 uint32_t *launch_id_out, void *stream);
int mtq_tile_stats_partial_end(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                               uint32_t layout_mask, double *stats, const uint32_t *mark, uint32_t launch_id, void *stream);

/*
 * K1 for a list of tiles: what mtq_tile_stats_partial left out, for the tiles that turn out to need it.  listed[0 .. *n_listed) (device;
 * at most `capacity` entries are read) names tiles as tensor * tiles + tile; for each of them the five statistics of the formats in
 * full_mask and Σ|x−y|, max|x−y| of those in err_mask are written into the tile's record (layout `layout_mask`), bit for bit what
 * mtq_tile_stats writes there; nothing else of the record is touched.  BFP formats only.  scratch: device memory of capacity + 1 uint32
 * (bf16 storage goes through the LDS-staged exact kernel, four listed tiles per wave, and parks the few tiles that kernel cannot take
 * there for the one-wave-per-tile kernel), or NULL (every tile through the one-wave-per-tile kernel).  The list comes from phase 1 of a split search
 * (mtq_greedy_scan_device_ex), which is the only reader of these statistics before the map is final.
 */
int mtq_tile_stats_listed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                          uint32_t layout_mask, uint32_t full_mask, uint32_t err_mask, const uint32_t *listed, const uint32_t *n_listed,
                          int64_t capacity, uint32_t *scratch, double *stats, void *stream);

/*
 * K2 quantize — materialise y = quantize→dequantize(x) for one format as float32.
 * Replaces quantize_weight_values (quantization_formats.py:171-194) behind Quantizer.quantize
 * (quantizer.py:34) for fmt in {bf16, bfp8, bfp4, bfp2, fp0, mxfp4, nvfp4}.  Bit-exact, including the
 * reference's saturating round-up, sign-of-zero, denormal→0 and uint32 wrap-around quirks, and for the
 * two proxies its float32 log2 at the binade edges, tie-low fp4 levels and e4m3 with a largest value of 240
 * (csrc/mtq_fp4_proxy.hip).  Other codes: MTQ_ERR_UNSUPPORTED.
 */
int mtq_quantize(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld,
                 int fmt, float *y, int64_t ldy, void *stream);

/*
 * FP4P fp4_proxy_sums — the `none` rows of the MXFP4 / NVFP4 proxies (quantization_formats.py:174-183,257-278: y = sign(x)·g(|x|),
 * elementwise) for `count` equally shaped matrices at x + i*stride_elems, in one read of x; y is never written.  fmt_mask: bit 0 mxfp4,
 * bit 1 nvfp4 (1..3, MTQ_ERR_INVALID otherwise).  sums: device doubles [count][2][7] in the order of mtq_columns_from_sums
 * (Σx, Σx², Σy, Σy², Σxy, Σ|x−y|, max|x−y|; the products and |x−y| formed in float32, summed in float64); the slots of formats outside
 * fmt_mask are left untouched.  Deterministic: per-block partials in a fixed order whose blocking depends on rows × cols alone (a
 * matrix gets the same bits alone or in a batch), then a fixed tree; no float atomics.  scratch: device doubles, at least
 * mtq_fp4_proxy_scratch_doubles(count, rows, cols).  csrc/mtq_fp4_proxy.hip.
 */
size_t mtq_fp4_proxy_scratch_doubles(int64_t count, int64_t rows, int64_t cols);
int mtq_fp4_proxy_sums(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                       uint32_t fmt_mask, double *sums, double *scratch, size_t scratch_doubles, void *stream);

/*
 * K1T tile_stats_transposed — K1 of Xᵀ read from the row-major X, for `count` equally shaped matrices at x + i*stride_elems (one
 * launch).  Replaces, for the `transpose` algorithm, the quantisation of np.transpose(x) per format (compression_algorithms/
 * transpose.py:13-33 → quantization_formats.py:84-164, a shared exponent per 16 consecutive ROWS of one column of X) plus the float32
 * metrics wq forms from it (wq:683-687); no transposed copy of X is made.
 *
 * The records are exactly those mtq_tile_stats writes for a contiguous copy of Xᵀ (cols × rows), bit for bit: the same layout
 * (2 + 5·popcount(fmt_mask) doubles), terms and summation order, applied to Xᵀ.  Tiles are numbered row-major over Xᵀ's grid:
 * element (r, c) of X lies in tile (c/32)·ceil(rows/32) + r/32 of its matrix; matrix i's tiles follow matrix i−1's.
 * fmt_mask: 1..4 of bf16|bfp8|bfp4|bfp2 (MTQ_ERR_INVALID otherwise).
 */
int mtq_tile_stats_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols,
                              int64_t ld, uint32_t fmt_mask, double *stats, void *stream);

/*
 * K2T quantize_transposed — y = (K2 of Xᵀ)ᵀ as float32 into a row-major rows × cols y (leading dimension ldy): bit for bit
 * np.transpose(quantize_weight_values(np.transpose(X), fmt)) (transpose.py:27-28), quirks included, for fmt in
 * {bf16, bfp8, bfp4, bfp2, fp0} (MTQ_ERR_UNSUPPORTED otherwise).  Rows past `rows` count as zero pads of the last group of a column.
 */
int mtq_quantize_transposed(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld,
                            int fmt, float *y, int64_t ldy, void *stream);

/*
 * K3T apply_assignment_transposed — y = (K3 of Xᵀ with `map`)ᵀ as float32 into a row-major rows × cols y (leading dimension ldy) for
 * `count` equally shaped matrices at x + i*stride_elems (y of matrix i at y + i*rows*ldy, its map at map + i*tiles): bit for bit
 * mtq_apply_assignment on a contiguous copy of Xᵀ, transposed back.  map is Xᵀ's grid, ceil(cols/32) × ceil(rows/32), row-major, on
 * device — K1T's tile numbering: element (r, c) of X takes the format of entry (c/32)·ceil(rows/32) + r/32.  A shared exponent covers
 * 16 consecutive rows of one column of X (the mixed-tile searches with params["layout"] = "transpose").
 */
int mtq_apply_assignment_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols,
                                    int64_t ld, const int8_t *map, float *y, int64_t ldy, void *stream);

/*
 * K3 apply_assignment — y where each 32×32 tile uses the format its int8 map entry names.
 * Replaces the tile gather/scatter of mixed_tile_threshold.py:125-132, mixed_tile_greedy.py:273,348-352
 * and scripts/reconstruct_mixed_tile_assignment.py:82-94.  map is tiles_h × tiles_w, row-major, on device.
 */
int mtq_apply_assignment(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld,
                         const int8_t *map, float *y, int64_t ldy, void *stream);

/*
 * LOE output_error — the layer-output error of quantised weights (no reference counterpart: the consumer of the files
 * scripts/generate_deepseek_layer0_io.py records).  x: m × k bf16 activations (ldx), w: n × k weight (w_dtype, ldw, nn.Linear
 * convention), bias: n float32 or NULL.  R = x·wᵀ + b is compared with Y_f = x·Ŵ_fᵀ + b for every format bit of fmt_mask (bits 0..3:
 * Ŵ = K2 of w, row layout), with the map candidate when `map` is not NULL (Ŵ = K3 of w with map: ceil(n/32) × ceil(k/32) int8 codes,
 * row-major, on device), with fp0 (Y = b) always, and with `recorded` (m × n, rec_dtype, ldr) when it is not NULL.  Ŵ and Y are never
 * written.  sums: device doubles [MTQ_OE_SLOTS][7] in the order of mtq_columns_from_sums (Σr, Σr², Σq, Σq², Σrq, Σ|r−q|, max|r−q|),
 * slots bf16, bfp8, bfp4, bfp2, map, fp0, recorded; the call ADDS this chunk's sums to them (max for the last), so a caller zeroes
 * them once and passes m in chunks.  Slots not requested are left untouched.  scratch: device doubles, at least
 * mtq_output_error_scratch_doubles(m, n).  Deterministic: a fixed reduction order, no float atomics.  csrc/mtq_output_error.hip.
 */
#define MTQ_OE_SLOTS 7
enum { MTQ_OE_BF16 = 0, MTQ_OE_BFP8 = 1, MTQ_OE_BFP4 = 2, MTQ_OE_BFP2 = 3, MTQ_OE_MAP = 4, MTQ_OE_FP0 = 5, MTQ_OE_RECORDED = 6 };
size_t mtq_output_error_scratch_doubles(int64_t m, int64_t n);
int mtq_output_error(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                     const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                     double *sums, double *scratch, size_t scratch_doubles, void *stream);

/*
 * LOE with quantised activations — mtq_output_error with the candidates fed Q(X): Y_f = xq·Ŵ_fᵀ + b for every format bit (bf16: Ŵ = bf16(w))
 * and for the map, while R = x·wᵀ + b keeps x; fp0 and `recorded` are unchanged.  xq: m × k bf16 on device (ldxq >= k), normally
 * mtq_quantize_rows_bf16 of x; xq == x gives the sums of mtq_output_error bit for bit.  Same sums, slots, scratch, accumulation and
 * determinism as mtq_output_error; a null xq or ldxq < k is MTQ_ERR_INVALID, the other checks are its own.  csrc/mtq_output_error.hip.
 */
int mtq_output_error_qx(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                        const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                        double *sums, double *scratch, size_t scratch_doubles, void *stream, const void *xq, int64_t ldxq);

/*
 * LOE activation pre-pass — Q(X) of a bf16 rows × cols matrix (ld) in the row layout (groups of 16 consecutive columns of one row),
 * written as bf16 (ldy): the upper 16 bits of mtq_quantize's float32 y for in_dtype bf16, specials included (a BFP value has its low
 * 16 bits zero).  fmt: MTQ_FMT_BF16 (a copy), _BFP8, _BFP4, _BFP2; fp0 and the fp4 proxies are not activation formats
 * (MTQ_ERR_UNSUPPORTED).  x and y must not overlap.  csrc/mtq_output_error.hip.
 */
int mtq_quantize_rows_bf16(const void *x, int64_t rows, int64_t cols, int64_t ld, int fmt, void *y, int64_t ldy, void *stream);

/*
 * LOE in the transposed BFP layout — mtq_output_error (xq == NULL) or mtq_output_error_qx (xq != NULL) with Ŵ_f = K2_f(wᵀ)ᵀ for the
 * bfp8 / bfp4 / bfp2 bits: a group is 16 consecutive rows (n) of one column (k), aligned from row 0, a ragged last group completed with
 * +0.  `map`, when not NULL, is over wᵀ's grid: ceil(k/32) × ceil(n/32) int8 codes, row-major (the code of w[n][k] is
 * map[(k/32) · ceil(n/32) + n/32]).  R, the bf16 candidate, fp0 and `recorded` are layout-free: their sums are bit-identical to
 * mtq_output_error's (mtq_output_error_qx's with xq) for the same inputs.  Same sums, slots, scratch (mtq_output_error_scratch_doubles),
 * checks and determinism.  csrc/mtq_output_error.hip.
 */
int mtq_output_error_transposed(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                                const float *bias, uint32_t fmt_mask, const int8_t *map, const void *recorded, int rec_dtype, int64_t ldr,
                                double *sums, double *scratch, size_t scratch_doubles, void *stream, const void *xq, int64_t ldxq);

/*
 * Budget maps, device half (no reference counterpart; quantization_analysis_amd/budget_maps.py holds the host half and the contract).
 * W is one op's weight, n × k (bf16 or float32, nn.Linear convention); X_cal its calibration activations, m × k bf16; the tiles are the
 * 32 × 32 row-layout tiles of W, zero padded, and c is a tile's column block.
 *
 * Gram blocks — H_c = X[:, 32c : 32c+32]ᵀ · X[:, 32c : 32c+32] as float64 32 × 32 blocks, c = 0 .. ceil(k/32) − 1 (columns past k are zero;
 * only the diagonal blocks of XᵀX are formed).  x: m × k bf16 on device (ldx >= k); h: device doubles [ceil(k/32)][32][32], h_doubles
 * their count.  The call ADDS this chunk's blocks to h, so a caller zeroes h once and passes m in chunks.  bf16 products are exact in
 * f32 and the f32 sums are folded into float64 at least every 256 tokens: an entry is within 2^-16 · (|X|ᵀ|X|)_ab of the exact value.
 * scratch: device doubles, at least mtq_gram_blocks_scratch_doubles(m, k).  Deterministic: a fixed reduction order, no float atomics.
 *
 * Tile error tables — for every tile t = (r, c), t = r · ceil(k/32) + c, and format code f (bf16, bfp8, bfp4, bfp2), with
 * Δ_f = K2_f(w) − w in float64 (row layout: the Ŵ that K3 builds for a tile coded f) and δ_i row i of the tile in Δ_f:
 * e_out[t][f] = Σ_i δ_iᵀ H_c δ_i (the tile's share of ‖X·Δᵀ‖²_F without the cross-block terms) and e_w[t][f] = Σ δ², both float64 in a
 * fixed order.  w: n × k (w_dtype, ldw >= k); h: the Gram blocks of k (h_doubles = ceil(k/32) · 1024); e_out, e_w: device doubles
 * [tiles][4], table_doubles = tiles · 4; e_w may be NULL.
 *
 * A null pointer, m, n or k <= 0, ld < k, a w_dtype that is not BF16 / F32 or a size mismatch returns MTQ_ERR_INVALID before a device
 * is looked for.  csrc/mtq_budget.hip.
 */
size_t mtq_gram_blocks_scratch_doubles(int64_t m, int64_t k);
int mtq_gram_blocks(const void *x, int64_t m, int64_t k, int64_t ldx, double *h, size_t h_doubles, double *scratch, size_t scratch_doubles,
                    void *stream);
int mtq_tile_error_tables(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *h, size_t h_doubles, double *e_out,
                          double *e_w, size_t table_doubles, void *stream);

/*
 * Tile error tables in the transposed layout — mtq_tile_error_tables with Δ_f = K2_f(wᵀ)ᵀ − w (groups of 16 consecutive rows of one
 * column) and the tiles over wᵀ's grid: t = kb · ceil(n/32) + nb pairs column block kb of w with row block nb, and
 * e_out[t][f] = Σ_i δ_iᵀ H_kb δ_i over the rows i of the tile (δ_i = row i of Δ_f restricted to column block kb).  Same arguments, h,
 * table sizes and checks as mtq_tile_error_tables.  csrc/mtq_budget.hip.
 */
int mtq_tile_error_tables_transposed(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *h, size_t h_doubles,
                                     double *e_out, double *e_w, size_t table_doubles, void *stream);

/*
 * Tile maps at a size target (the mixed-tile-budget algorithm; budget_maps.allocate is the contract and the oracle).
 *
 * Weight-space error table, batched — e_w[b][t][f] = Σ (K2_f(x_b) − x_b)² for every tile t of `count` equally shaped resident matrices
 * (matrix b at x + b · stride_elems, rows × cols, ld >= cols, bf16 or float32, row layout, ragged edges zero padded) in one launch:
 * bit for bit the e_w that mtq_tile_error_tables writes for each matrix alone (the same per-tile order), without Gram blocks and
 * without e_out.  e_w: device doubles [count][tiles][4].
 *
 * Allocation — table: device doubles [tiles][4] by format code; segment j is tiles seg_first[j] .. seg_first[j + 1] − 1 (seg_first:
 * n_seg + 1 device entries, non-decreasing from 0 to tiles) with its own budget_bytes[j] (device doubles).  One segment per tensor of a
 * batch gives every tensor its own budget; one segment over everything lets the tensors of a model share one.  For every segment whose
 * table is finite, map (device int8 [tiles], format codes) and counts (device int64 [n_seg][4], tiles per format code) are those of
 * budget_maps.allocate on the segment's rows with the candidates of fmt_mask: every tile walks the lower convex hull of its
 * (bytes, error) points with allocate's float64 operations, the steps are ordered by (slope descending, tile ascending, step
 * ascending) and taken while allocate's size expression stays within the budget.  status (device int32 [n_seg]): 0 done; 1 the budget
 * is below the all-cheapest size; 2 a non-finite entry in the segment's rows (any of the four columns); map and counts of a segment
 * with a non-zero status are unspecified.  scratch: 8-byte aligned device memory of at least mtq_budget_allocate_scratch_bytes bytes for
 * (tiles, n_seg).  Everything is enqueued on `stream`; nothing is read back and no float atomics are used: equal tables give equal maps.
 *
 * A null pointer, count, rows, cols, tiles or n_seg <= 0, ld < cols, a fmt_mask without a tile format or a short scratch returns
 * MTQ_ERR_INVALID before a device is looked for.  csrc/mtq_budget.hip.
 */
int mtq_tile_sq_error_batched(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                              double *e_w, void *stream);
size_t mtq_budget_allocate_scratch_bytes(int64_t tiles, int64_t n_seg);
int mtq_budget_allocate_device(const double *table, int64_t tiles, const int64_t *seg_first, int n_seg, uint32_t fmt_mask,
                               const double *budget_bytes, int8_t *map, int64_t *counts, int32_t *status, void *scratch,
                               size_t scratch_bytes, void *stream);

/*
 * GPTQ's error-compensated BFP weights, device half (no reference counterpart; quantization_analysis_amd/gptq.py holds the host half
 * and the contract).  W is one op's weight, n × k (bf16 or float32, nn.Linear convention); X_cal its calibration activations, m × k bf16.
 *
 * Full Gram — H = XᵀX as k × k float64 (row-major, h_doubles = k · k), ADDED into h: a caller zeroes h once and passes m in chunks.
 * The numerics of mtq_gram_blocks (bf16 MFMA, f32 folded into float64 at least every 256 tokens: an entry within 2^-16 · (|X|ᵀ|X|)_ab);
 * each entry is formed once and written to (a, b) and (b, a), so a symmetric h stays bitwise symmetric.  scratch: device doubles, at
 * least mtq_gram_full_scratch_doubles(m, k), which is 0 when the column-block pairs alone fill the device (k >= 5632); a non-null
 * pointer is still required.  Deterministic: a fixed reduction order, no float atomics.
 *
 * Sweep — for every row and column j in order (float64): at the start of a 16-column group E = the largest exponent field of the float32
 * of the group's current values; q_j = q_E(w_j, code of j's tile) (bf16: RNE of float32(w_j); BFP: the element rule of mtq_quantize with
 * shared exponent E, an exponent above E saturating to ±(2^M − 1)·step); e_j = (w_j − q_j) / U_jj; w_j' −= e_j · U_jj' for j' > j.
 * w: n × k (w_dtype, ldw >= k); u: device doubles k × k (u_doubles = k · k), the upper Cholesky factor of the damped inverse Hessian,
 * only its upper triangle read; codes: int8 [ceil(n/32)][ceil(k/32)] MIXED_TILE_FORMATS codes 0..3 (code_count entries; values are not
 * checked); out: n × k float32 (ldo >= k) receives Ŵ = q; loss: n doubles receive Σ_j e_j² per row; scratch: device doubles, 16-byte
 * aligned, at least mtq_gptq_sweep_scratch_doubles(n, k) (e of every row and column).  The summation order of the updates differs from a
 * column-by-column sweep (a blocked, left-looking update); the rest is the per-element arithmetic above.
 *
 * A null pointer, m, n or k <= 0, ld < k, a w_dtype that is not BF16 / F32 or a size mismatch returns MTQ_ERR_INVALID before a device
 * is looked for.  csrc/mtq_gptq.hip.
 */
size_t mtq_gram_full_scratch_doubles(int64_t m, int64_t k);
int mtq_gram_full(const void *x, int64_t m, int64_t k, int64_t ldx, double *h, size_t h_doubles, double *scratch, size_t scratch_doubles,
                  void *stream);
size_t mtq_gptq_sweep_scratch_doubles(int64_t n, int64_t k);
int mtq_gptq_sweep(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *u, size_t u_doubles, const int8_t *codes,
                   size_t code_count, float *out, int64_t ldo, double *loss, double *scratch, size_t scratch_doubles, void *stream);

/*
 * K5 dequant_fp8_block (loader) — float8-e4m3fn weights × float32 inverse block scales → float32: the on-load
 * dequantisation of DeepSeek-style checkpoints, `w.float() * scale_inv.repeat_interleave(block)` with
 * block = ceil(dim / scale_dim) (hf_model_utils.py:199-215, used at :273-281).  w: rows × cols bytes (ldw),
 * scale_inv: scale_rows × scale_cols float32 (contiguous), out: rows × cols float32 (ldo).  Bit-exact.
 */
int mtq_dequant_fp8_block(const void *w, const float *scale_inv, int64_t rows, int64_t cols, int64_t ldw,
                          int64_t scale_rows, int64_t scale_cols, float *out, int64_t ldo, void *stream);

/*
 * Slim copy of K1's records for the pcc greedy scan (MTQ_MASK_SLIM): out[t] = [Σx, Σx², {Σy, Σy², Σxy} per format bit of
 * fmt_mask], 2 + 3F doubles per tile, for `tiles` records back to back (any number of tensors).  Device to device; what
 * crosses PCIe afterwards is 88 instead of 136 B/tile at F = 3.
 */
int mtq_pack_slim_records(const double *stats, int64_t tiles, uint32_t fmt_mask, double *out, void *stream);

/* ------------------------------------------------------------------ HOST: decisions on stats records */

/*
 * H1 greedy scan — the sequential part of mixed_tile_greedy.py:133-346 on HOST copies of the stats.
 * The visiting order of every pass comes from the caller (numpy's Generator, :222-231), so the
 * NumPy PCG64 stream stays the caller's.
 */
typedef struct mtq_greedy mtq_greedy; /* opaque */

/* elem_count = float(xf.size) (:134).  stats/rec as written by mtq_tile_stats for fmt_mask. */
int mtq_greedy_create(mtq_greedy **out, const double *stats, int64_t tiles, uint32_t fmt_mask,
                      int metric, double threshold, double elem_count, int base_fmt);
/* One `for fmt in tile_formats` iteration (:227-346) over order[0..n). */
int mtq_greedy_pass(mtq_greedy *g, int fmt, const int64_t *order, int64_t n);
/* Copies of the scan state: assignment int8[tiles], fixed uint8[tiles], counts int64[4]. */
int mtq_greedy_assignment(const mtq_greedy *g, int8_t *assign);
int mtq_greedy_fixed(const mtq_greedy *g, uint8_t *fixed);
int mtq_greedy_counts(const mtq_greedy *g, int64_t counts[4]);
/* Current global metric value (pcc_value :176-190, mae :280, atol :305). */
int mtq_greedy_value(const mtq_greedy *g, double *value);
void mtq_greedy_destroy(mtq_greedy *g);

/*
 * NumPy-compatible generator for the visiting order: mtq_rng_create(seed) ≡ np.random.default_rng(seed),
 * successive mtq_rng_permutation(n) ≡ successive rng.permutation(n) (SeedSequence → PCG64 → Fisher–Yates with
 * masked rejection sampling, NumPy ≥ 1.17).  rng.permutation(a) == a[rng.permutation(len(a))].
 */
typedef struct mtq_rng mtq_rng; /* opaque */
int mtq_rng_create(mtq_rng **out, uint64_t seed);
int mtq_rng_permutation(mtq_rng *r, int64_t n, int64_t *out);
/* ≡ rng.integers(0, high, size=n, dtype=np.int64) for 1 <= high < 2^32 − 1 (mixed_tile_random.py:135: Lemire
 * rejection on buffered 32-bit draws; high == 1 draws nothing). */
int mtq_rng_integers(mtq_rng *r, int64_t high, int64_t n, int64_t *out);
void mtq_rng_destroy(mtq_rng *r);

/*
 * The whole greedy search of one tensor on host records (mixed_tile_greedy.py:95-346): passes in `formats`
 * order (formats[0] is the base format), candidates = np.where(~fixed)[0], order = permutation(candidates) from
 * default_rng(seed) (seed != 0).  map: int8[tiles]; counts: per MIXED_TILE_FORMATS entry; out[9] as
 * mtq_columns_from_stats.  Thread-safe; the streamed driver calls it from worker threads.
 */
int mtq_greedy_run(const double *stats, int64_t tiles, uint32_t fmt_mask, const int *formats, int n_formats,
                   int metric, double threshold, double elem_count, uint64_t seed, int8_t *map,
                   int64_t counts[4], double out[9]);

/*
 * mtq_greedy_run over `count` equally sized tensors (records contiguous: count × tiles × record doubles) on up to
 * n_threads host threads.  seeds[count]; maps int8[count][tiles]; counts int64[count][4]; outs double[count][9].
 */
int mtq_greedy_run_batch(const double *stats, int64_t count, int64_t tiles, uint32_t fmt_mask, const int *formats,
                         int n_formats, int metric, double threshold, double elem_count, const uint64_t *seeds,
                         int8_t *maps, int64_t *counts, double *outs, int n_threads);

/*
 * Per-tile scores from the raw sums, n = 1024 (tile_utils.py:46-57 semantics on float64 moments):
 * pcc via the moment formula, mae = Σ|d|/1024, atol = max|d|.  scores is [formats][tiles], formats in ascending
 * code order: popcount(mask & 0xF) rows, plus a leading bf16 row under MTQ_MASK_BF16_IDENTITY.
 */
int mtq_tile_scores(const double *stats, int64_t tiles, uint32_t fmt_mask, int metric, double *scores);


/*
 * K4 threshold_assign — mixed_tile_threshold.py:111-123 / scripts/sweep_mixed_tile_threshold.py:145-155:
 * per tile the lowest-bytes format among `formats` whose score passes, else the highest-bytes one.
 * The reference compares float32 scores with a float32-rounded threshold (NumPy ≥ 2, NEP 50);
 * tiles with a looked-at format whose float64 score lies within `band` of float32(threshold) are listed in knife_ids
 * (capacity knife_cap), with the bit mask of those format codes in knife_near (nullable, same capacity), so the caller
 * can decide exactly those formats of those tiles with the literal float32 expression.  Formats behind the chosen one
 * were not looked at.
 */
int mtq_threshold_assign(const double *stats, int64_t tiles, uint32_t fmt_mask,
                         const int *formats, int n_formats, int metric, double threshold, double band,
                         int8_t *map, int64_t *knife_ids, uint8_t *knife_near, int64_t knife_cap, int64_t *n_knife);

/*
 * Tensor-level columns (pcc, mae, atol) of the reconstruction a map implies, from the raw sums in
 * float64 (replaces wq:683-687 for the hip backend; see DESIGN.md on the float32 column).
 * out[0..2] = pcc, mae, atol; out[3..8] = Σx, Σx², Σy, Σy², Σxy, Σ|d|.
 */
int mtq_columns_from_stats(const double *stats, int64_t tiles, uint32_t fmt_mask, const int8_t *map,
                           double elem_count, double out[9]);
/* The same columns from the seven sums themselves (Σx, Σx², Σy, Σy², Σxy, Σ|d|, max|d|), e.g. those of
 * mtq_column_sums_device copied to the host. */
int mtq_columns_from_sums(const double sums[7], double elem_count, double out[9]);

/* ------------------------------------------------------------------ DEVICE: decisions on device-resident records */

/*
 * The functions above read HOST copies of the records (the greedy scan is sequential and lives there).  The threshold
 * rule, the per-tile scores and the moments of a map are per-tile / reduction work and have DEVICE forms that read the
 * records where K1 wrote them: nothing but maps (1 B/tile), flags and a handful of doubles crosses PCIe.  Same arithmetic
 * (csrc/mtq_decide.hpp), same bits as the host forms — except the column sums, which add in a fixed tree order.
 * All pointers are device pointers; calls are asynchronous on `stream`.
 */

/* mtq_tile_scores on the device: scores[formats][tiles] (device), rows as documented for mtq_tile_scores. */
int mtq_tile_scores_device(const double *stats, int64_t tiles, uint32_t fmt_mask, int metric, double *scores, void *stream);

/* K4: mtq_threshold_assign on the device.  map: int8[tiles]; knife: uint8[tiles], bit c set where looked-at format code c
 * scores within `band` of float32(threshold) (0 for most tiles; the caller decides those formats of those tiles with the
 * literal float32 expression). */
int mtq_threshold_assign_device(const double *stats, int64_t tiles, uint32_t fmt_mask, const int *formats, int n_formats,
                                int metric, double threshold, double band, int8_t *map, uint8_t *knife, void *stream);


/* Σx, Σx², Σy, Σy², Σxy, Σ|d|, max|d| of the reconstruction `map` implies → scratch[0..6] (device), and the map's number of tiles per
 * format code 0..3 → scratch[7..10] (whole numbers as doubles: mixed_tile_threshold.py:133-135's bincount without the map leaving the
 * device first).  scratch must hold mtq_columns_scratch_doubles() doubles.  Σx is NaN when the map names a format that is not
 * available.  The caller turns the seven sums into pcc / mae / atol with the formulas of mtq_columns_from_stats. */
size_t mtq_columns_scratch_doubles(void);
int mtq_column_sums_device(const double *stats, int64_t tiles, uint32_t fmt_mask, const int8_t *map, double *scratch, void *stream);
/* The same for `count` equally sized tensors in one launch pair: records [count][tiles][rec], maps [count][tiles], scratch
 * [count][mtq_columns_scratch_doubles()] — tensor i's seven sums at scratch[i * mtq_columns_scratch_doubles()]. */
int mtq_column_sums_device_batched(const double *stats, int64_t count, int64_t tiles, uint32_t fmt_mask, const int8_t *maps,
                                   double *scratch, void *stream);

/* H1 on the device (csrc/mtq_scan.hip): mtq_greedy_run for `count` equally sized tensors whose FULL records
 * [count][tiles][2+5F] are where K1 wrote them — replaces mixed_tile_greedy.py:133-346 without moving the records: one wave64
 * per tensor performs the initial sums, NumPy's Generator.permutation of every pass (SeedSequence → PCG64, bit-compatible)
 * and the sequential accept / reject scan with the host scan's IEEE operations in the host scan's order, so maps[count][tiles]
 * (device, int8 codes) are the host's maps.  status[count] (device): 0 = done; 1 = a zero denominator turned up (the decision
 * needs Σ|x−y|: run mtq_greedy_run on that tensor's records); 2 = internal budget exhausted (same remedy).  Serves the pcc
 * metric, the mae metric (one running sum, Σ|x−y|: mixed_tile_greedy.py:280-301) and the atol metric (:305-344 — order-independent for
 * finite maxima, a per-tile walk down the format list: csrc/mtq_scan.hip greedy_atol; status 1 when a maximum is NaN), distinct
 * formats (fmt_mask may carry MTQ_MASK_BF16_IDENTITY), tiles <= MTQ_SCAN_DEVICE_MAX_TILES; anything else (repeated formats, more
 * tiles) returns MTQ_ERR_UNSUPPORTED and the caller uses the host scan.  seeds[count]: device array of non-zero seeds.  counts
 * [count][4] (device, may be NULL): tiles per format code of every finished map (np.bincount of the map).  scratch:
 * device memory of mtq_greedy_scan_scratch_bytes(count, tiles) bytes.  Asynchronous on `stream`. */
#define MTQ_SCAN_DEVICE_MAX_TILES (1 << 22)
size_t mtq_greedy_scan_scratch_bytes(int64_t count, int64_t tiles);
int mtq_greedy_scan_device(const double *stats, int64_t count, int64_t tiles, uint32_t fmt_mask, const int *formats, int n_formats,
                           int metric, double threshold, double elem_count, const uint64_t *seeds, int8_t *maps, int32_t *status,
                           int32_t *counts, void *scratch, size_t scratch_bytes, void *stream);

/* The same search with what round 3 added (mtq_greedy_scan_device is this with orders = NULL, phase = 0):
 *   orders  — NULL, or the buffer mtq_scan_orders_device filled for the seed that ALL `count` tensors share (seeds[] must hold that
 *             seed): every tensor of a model run is searched with one seed (mixed_tile_greedy.py:222-226), and a pass's permutation
 *             depends only on the generator state and the number of candidates, so the base pass's draws and the permutations of
 *             range(tiles) of passes 1 and 2 are computed once per launch; a tensor whose pass 1 rejects a tile shuffles its own
 *             candidates from the shared state, as before.  With orders the kernel runs two waves per tensor: the second gathers the
 *             passes' deltas ahead of the first.
 *   phase   — 0: the whole search.  1: every pass but the last, then the last pass's candidates (np.where(~fixed), :228) of every
 *             tensor are appended to listed[] as tensor * tiles + tile (n_listed: device counter, zeroed by the caller) and the
 *             search's state goes to carry (mtq_scan_carry_bytes(count) bytes); maps hold work-in-progress codes.  2: the last pass
 *             from carry, then the finished maps, status and counts.  Between 1 and 2 the caller fills in the statistics of the
 *             last format for the listed tiles (mtq_tile_stats_listed) — the search never reads them for any other tile.  Phases need
 *             n_formats >= 2 and the pcc or mae metric.
 */
size_t mtq_scan_carry_bytes(int64_t count);
int mtq_greedy_scan_device_ex(const double *stats, int64_t count, int64_t tiles, uint32_t fmt_mask, const int *formats, int n_formats,
                              int metric, double threshold, double elem_count, const uint64_t *seeds, int8_t *maps, int32_t *status,
                              int32_t *counts, void *scratch, size_t scratch_bytes, const void *orders, int phase, uint32_t *listed,
                              uint32_t *n_listed, void *carry, void *stream);
/* The visiting orders a launch's tensors share: the generator (SeedSequence(seed) → PCG64) after the base pass's draws, then
 * Generator.permutation(tiles) for pass 1 and — n_orders == 2 — once more for pass 2, with the generator states in between, into
 * `orders` (mtq_scan_orders_bytes(tiles) bytes, device).  Depends on nothing but seed and tiles: it can run beside K1. */
size_t mtq_scan_orders_bytes(int64_t tiles);
int mtq_scan_orders_device(uint64_t seed, int64_t tiles, int n_orders, void *orders, size_t orders_bytes, void *stream);

/* Last-pass candidates finished inside K1 (the lazy route's early form).  Where every tile accepts the first BFP format, the tiles that reach
 * the search's last pass are very nearly the first visits of the pass before it, whose order is one of the shared orders: "rank below a
 * cutoff" predicts them before the search has run, and K1 evaluates their left-out statistics from the rows it holds anyway.
 *   mtq_scan_rank_device: rank[0 .. tiles) (device uint32) = the inverse of order `which` (0: pass 1's, 1: pass 2's) of an orders buffer
 *     mtq_scan_orders_device has filled: rank[order[i]] = i, np.argsort of the reference's permutation; all-ones when the order is not
 *     complete.  Ordered behind mtq_scan_orders_device by the stream.
 *   mtq_tile_stats_partial_begin_early: mtq_tile_stats_partial_begin, and for every tile with rank[tile] < cutoff (tile: index inside its
 *     tensor) also what mtq_tile_stats_listed(full_mask bfp2, err_mask bfp4) writes, bit for bit.  Needs layout bfp8|bfp4|bfp2, full_mask
 *     bfp8, sums_mask bfp4 (MTQ_ERR_UNSUPPORTED otherwise); cutoff 0 is mtq_tile_stats_partial_begin itself.  A ranked tile the kernel
 *     cannot take is marked like any other, and _end writes its whole record.
 *   mtq_greedy_scan_device_early: phase 1 of mtq_greedy_scan_device_ex that keeps the candidates with rank < cutoff off the list (the
 *     same table and cutoff as the K1 launch of these records); the list may come out empty while the last pass still has candidates.
 * The cutoff is a hint: any value gives the same maps.  All three symbols are optional: a build of this version may lack them. */
int mtq_scan_rank_device(const void *orders, int64_t tiles, int which, uint32_t *rank, void *stream);
int mtq_tile_stats_partial_begin_early(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                       uint32_t layout_mask, uint32_t full_mask, uint32_t sums_mask, double *stats, uint32_t *mark,
                                       uint32_t *launch_id_out, const uint32_t *rank, uint32_t cutoff, void *stream);
int mtq_greedy_scan_device_early(const double *stats, int64_t count, int64_t tiles, uint32_t fmt_mask, const int *formats, int n_formats,
                                 int metric, double threshold, double elem_count, const uint64_t *seeds, int8_t *maps, int32_t *status,
                                 int32_t *counts, void *scratch, size_t scratch_bytes, const void *orders, uint32_t *listed,
                                 uint32_t *n_listed, void *carry, const uint32_t *rank, uint32_t cutoff, void *stream);

/* The knife-edge tiles of the threshold rule, prepared on the device for the host's literal float32 score (replaces the gather of
 * tiles and the per-format Quantizer.quantize calls of mixed_tile_threshold.py:97-110 for the tiles whose float64 score fell inside
 * the noise band — `near` is the mask array mtq_threshold_assign_device wrote, one int8 per tile of `count` equally shaped tensors):
 * list[0 .. cap) receives the flat ids (tensor * tiles + tile) of flagged tiles in no particular order, list[cap] their total number
 * (which may exceed cap: the caller then handles the batch another way); tiles_out[(p * cap + slot) * 1024 + r * 32 + c], p = 0 the
 * tile's own values as float32 (pads of ragged edge tiles +0.0, tile_utils.py:109-113), p = 1 + i the reconstruction in formats[i]
 * (codes 0..3, n_formats <= 4), for slot < min(list[cap], cap).  Asynchronous on `stream`; list and tiles_out are device memory
 * (tiles_out 16-byte aligned). */
int mtq_knife_tiles_device(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                           const int8_t *near, const int *formats, int n_formats, int64_t cap, int64_t *list, float *tiles_out, void *stream);

/* mtq_knife_tiles_device applied to Xᵀ, read from the row-major X in place: `near` holds one int8 per tile of Xᵀ's grid (K1T's
 * numbering), list as there, and slot p = 0 of tiles_out holds the 32×32 Xᵀ tile in Xᵀ's row-major order, p = 1 + i its reconstruction
 * in formats[i].  Equal to mtq_knife_tiles_device on a contiguous copy of Xᵀ.  n_formats may be 0 (formats may then be NULL): the tiles alone. */
int mtq_knife_tiles_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                               const int8_t *near, const int *formats, int n_formats, int64_t cap, int64_t *list, float *tiles_out, void *stream);

/* One batch of the streamed threshold driver as ONE call (round 4: behind Python every launch costs the driver 10–20 us, and a model's
 * small tensors — DeepSeek-R1 layer 0: seven tensors, 183 k tiles, 0.45 ms of K1 — were launch-bound at a dozen calls per batch):
 * mtq_tile_stats_batched(k1_mask) → mtq_threshold_assign_device(dec_mask: k1_mask, or k1_mask | MTQ_MASK_BF16_IDENTITY) into
 * both_dev[0 .. T) (maps) and both_dev[T .. 2T) (knife-edge masks), T = count * tiles → both of them into the pinned mirror both_host
 * (mtq_device_copy_2d) on `stream`; then, behind an event, on `side_stream` (NULL: on `stream`): mtq_knife_tiles_device(cap) and the list
 * (cap + 1 int64) into the pinned list_host.  Replaces the per-tensor body of wq:655-706 / mixed_tile_threshold.py:97-123 up to the
 * knife-edge decisions.  scratch and sums_host both non-NULL: mtq_threshold_columns under the maps as K4 left them follows on `stream`
 * at once — the batch's final sums unless its list names a knife-edge tile (the band is 2e-6 wide: rarely), in which case the caller
 * patches the maps and calls mtq_threshold_columns again; the host's look at the list is then off the GPU's critical path.
 * Everything asynchronous; the caller waits for an event of its own behind the call. */
int mtq_threshold_enqueue(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                          uint32_t k1_mask, uint32_t dec_mask, const int *formats, int n_formats, int metric, double threshold, double band,
                          double *stats, int8_t *both_dev, int8_t *both_host, int64_t cap, int64_t *list_dev, float *knife_dev,
                          int64_t *list_host, double *scratch, double *sums_host, void *stream, void *side_stream);
/* mtq_threshold_enqueue for the search of Xᵀ of every matrix (params["layout"] = "transpose"): the same arguments and stages with
 * mtq_tile_stats_transposed as stage one and mtq_knife_tiles_transposed as the listing — records, maps, masks and list ids over Xᵀ's
 * grid (K1T's numbering, as many tiles as X's).  mtq_threshold_columns serves its records unchanged. */
int mtq_threshold_enqueue_transposed(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                     uint32_t k1_mask, uint32_t dec_mask, const int *formats, int n_formats, int metric, double threshold, double band,
                                     double *stats, int8_t *both_dev, int8_t *both_host, int64_t cap, int64_t *list_dev, float *knife_dev,
                                     int64_t *list_host, double *scratch, double *sums_host, void *stream, void *side_stream);
/* … and its second half: mtq_column_sums_device_batched under the (patched) maps, the seven sums of every tensor and behind them the
 * map's tile count per format code 0..3 (mixed_tile_threshold.py:133-135's bincount, as doubles) into the pinned sums_host[count][11]
 * (wq:683-706's columns come from the sums: mtq_columns_from_sums). */
int mtq_threshold_columns(const double *stats, int64_t count, int64_t tiles, uint32_t dec_mask, const int8_t *maps_dev, double *scratch,
                          double *sums_host, void *stream);

/* RAGGED batches (round 4): n <= MTQ_RAGGED_MAX matrices of ONE storage type and ANY shapes as one launch per stage — a model's odd
 * tensors (DeepSeek-R1 layer 0's five float32 projections of five shapes, its two norm vectors as (ceil(n/32), 32) matrices) cost a
 * launch chain each through the calls above, and the chain, not the arithmetic, was their time.  The batch's tiles are numbered
 * through: matrix j's tiles, row-major (tile_utils.py:96-113), follow matrix j-1's; records, maps, masks and list ids use that number.
 * Per tile the kernels, the arithmetic and the summation order are those of the per-matrix calls (mtq_tile_stats on float32 or on bf16
 * storage the LDS-staged kernel does not take: the direct kernel + its fix-up): same records, bit for bit; the column sums of matrix j
 * are formed in the order mtq_column_sums_device uses for that matrix alone.  Replaces the same reference lines as the calls they
 * generalise (wq:655-706, mixed_tile_threshold.py:97-123). */
#define MTQ_RAGGED_MAX 24
typedef struct MtqMatrix { const void *x; int64_t rows, cols, ld; } MtqMatrix;   /* device pointer, leading dimension in elements */
int mtq_tile_stats_ragged(const MtqMatrix *mats, int n, int in_dtype, uint32_t fmt_mask, double *stats, void *stream);
int mtq_knife_tiles_ragged(const MtqMatrix *mats, int n, int in_dtype, const int8_t *near, const int *formats, int n_formats, int64_t cap,
                           int64_t *list, float *tiles_out, void *stream);
int mtq_column_sums_device_ragged(const double *stats, const int64_t *tiles_per, int n, uint32_t fmt_mask, const int8_t *maps, double *scratch,
                                  void *stream);   /* scratch: n * mtq_columns_scratch_doubles(); tensor j's sums at scratch[j * that] */
int mtq_threshold_enqueue_ragged(const MtqMatrix *mats, int n, int in_dtype, uint32_t k1_mask, uint32_t dec_mask, const int *formats, int n_formats,
                                 int metric, double threshold, double band, double *stats, int8_t *both_dev, int8_t *both_host, int64_t cap,
                                 int64_t *list_dev, float *knife_dev, int64_t *list_host, double *scratch, double *sums_host, void *stream,
                                 void *side_stream);
int mtq_threshold_columns_ragged(const double *stats, const int64_t *tiles_per, int n, uint32_t dec_mask, const int8_t *maps_dev, double *scratch,
                                 double *sums_host, void *stream);

/* Results home without a copy engine (no reference counterpart: the reference's arrays are host arrays).  A kernel copies `rows` rows
 * of `width_bytes` bytes from src (pitch src_pitch) to dst (pitch dst_pitch) on `stream`; dst may be pinned host memory
 * (hipHostMalloc / torch pin_memory: mapped into the device's address space), in which case the stores cross PCIe from the kernel
 * and the data are on the host when an event recorded behind the call has completed.  The streamed driver brings maps, counts and
 * column sums back this way: an asynchronous device-to-host memcpy of a few MB was seen to hold the calling thread until the stream
 * had drained.  Pointers device-accessible, pitches >= width_bytes, rows >= 1. */
int mtq_device_copy_2d(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width_bytes, size_t rows, void *stream);

/* Diagnostics (no reference counterpart).  K1's persistent waves claim their units from device counters that come from a
 * per-device ring of slots (csrc/mtq_slot_ring.hpp): a slot is handed out again only behind the event recorded after its
 * previous launch's reset, so any number of launches may be pending on any streams.  This runs that bookkeeping against
 * mock event operations on the host (no GPU): 0 = every property holds, else the number of the first failed check. */
int mtq_selftest_slot_ring(void);
/* Shader-clock ticks the first tensor of the last mtq_greedy_scan_device launch spent per phase (tools/scan_device_bench.py):
 * [0] start-up + initial sums, [1] base pass + draw-only shuffle, then for pass p = 1..3: [2+3(p-1)] candidates + shuffle,
 * [3+3(p-1)] deltas, [4+3(p-1)] visits.  Synchronises the device. */
int mtq_debug_scan_ticks(uint64_t out[16]);
/* The grid K1 launches over `total` work items on a device of `cus` compute units: kind MTQ_K1_BF16 (the LDS-staged bf16 kernel,
 * total in 32x128 units) or MTQ_K1_DIRECT (the direct kernel, uniform or ragged, total in tiles).  A host function: no GPU.
 * out[0] blocks; out[1] the claims a wave makes before it retires, as passed to the kernel (0: no limit; the direct kernel's is
 * 16 x units_per_wave); out[2] the counter groups in use, min(blocks, 64): group g's blocks g, g + groups, ... claim units
 * g, g + groups, ...  waves_per_simd < 0 and units_per_wave < 0 stand for what this process uses (MTQ_K1_WAVES, else what the
 * kernel is compiled for - for MTQ_K1_BF16 that of the instantiations evaluating two or three BFP formats; MTQ_K1_UNITS_PER_WAVE,
 * else 8).  units_per_wave 0: waves never retire.  This is the function both launchers size their grids with. */
#define MTQ_K1_BF16 0
#define MTQ_K1_DIRECT 1
int mtq_debug_k1_grid(int kind, int64_t total, int cus, int waves_per_simd, int units_per_wave, int64_t out[3]);
/* Synchronises the current device and counts the K1 claim counters and wave-completion words of its slot ring that are not zero
 * (the launch-id stamp word of a slot is not counted).  Every K1 launch leaves its slot zeroed, so *nonzero is 0 between launches -
 * also when no launch has allocated the ring yet. */
int mtq_debug_work_counters(int64_t *nonzero);

/* ------------------------------------------------------------------ PACKED mixed-tile weights (csrc/mtq_packed.hip)
 *
 * The bytes a tile map promises (no reference counterpart: the reference only models sizes, tile_utils.py:8-14).  This is THIS
 * project's layout, fixed here because it is an ABI; it does not claim to be TTNN's on-device tile format.
 *
 * Scope: the row layout (a group is 16 consecutive columns of one row) over the 2-D flatten and zero padding of tile_utils.py:91-113;
 * tiles numbered tr * tiles_w + tc; map codes 0..3 (bf16, bfp8, bfp4, bfp2), one int8 per tile.
 *
 *   stream   = the tiles' blobs in tile order.  Blob sizes by code: 2048, 1088, 576, 320 bytes (all multiples of 64).
 *   offsets  = uint32[tiles + 1], the exclusive prefix sum of the blob sizes in units of 64 bytes: tile t's blob starts at byte
 *              64 * offsets[t], and 64 * offsets[tiles] is the stream's length.
 *   BFP blob = 64 shared-exponent bytes, group g = 2 * row + half (row 0..31, half 0..1): the maximum float32 exponent field over
 *              the group's 16 zero-padded elements; then the element codes in row-major order e = 32 * row + col.
 *                bfp8: one byte per element.   bfp4: two per byte, even e in the low nibble.
 *                bfp2: four per byte, element e in bits 2 * (e % 4) .. 2 * (e % 4) + 1.
 *              code = (sign << M) | man, M = 7 / 3 / 1, with man as quantization_formats.py:118-158 forms it (the aligned mantissa
 *              with its hidden bit, rounded to nearest even, saturated at 2^M - 1; 0 for an input whose exponent field is 0) and
 *              the sign cleared when man == 0.  The float32 value K2 / K3 write is a pure function of (exponent byte, code).
 *   bf16 blob = 1024 little-endian uint16, row-major: the upper halves of the bf16 rounding of quantization_formats.py:29-45.
 *   Padding elements of edge tiles encode +0 (code 0); an all-padding group has exponent 0.  Every byte of the stream is written:
 *   two packings of the same input are byte-identical.
 *
 * Real sizes against the reference's size model (which stays as it is): 1.0625 / 0.5625 / 0.3125 bytes per element for bfp8 / bfp4 /
 * bfp2, where the model says 1.088 / 0.50097 / 0.25097.
 *
 * mtq_packed_tile_bytes and mtq_packed_offsets are HOST functions (host pointers, no device).  In the three device entry points x, y,
 * packed, map, offsets and bias are device pointers owned by the caller and the calls are asynchronous on `stream`; packed must be
 * 16-byte aligned.  Argument errors are MTQ_ERR_INVALID before a device is looked for.  A buffer shorter than the smallest stream the
 * tile grid can have (320 bytes per tile) is refused at once; the stream's exact length is 64 * offsets[tiles], which the caller who
 * built the offsets knows, and on the device every blob is checked against the buffer's length before it is touched (a blob that does
 * not fit is not written by pack, not stored by unpack, read as zeros by linear).
 */
/* 2048 / 1088 / 576 / 320 for fmt 0..3, 0 for any other code. */
size_t mtq_packed_tile_bytes(int fmt);
/* offsets[0 .. tiles] of a host map; a code outside 0..3 (or a stream past 2^32 units) is MTQ_ERR_INVALID. */
int mtq_packed_offsets(const int8_t *map, int64_t tiles, uint32_t *offsets);
/* x (in_dtype, rows × cols, ld >= cols, ragged edges zero-padded) → the stream in out[0 .. 64 * offsets[tiles]).  One wave per tile,
 * one lane per group. */
int mtq_pack_tiles(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld, const int8_t *map, const uint32_t *offsets,
                   void *out, size_t out_bytes, void *stream);
/* The stream → y (rows × cols, ldy >= cols).  out_dtype MTQ_DTYPE_F32: bit for bit what mtq_apply_assignment writes for the packed x
 * and map; MTQ_DTYPE_BF16: the upper halves, which is exact (every BFP and bf16 value has its low 16 bits zero). */
int mtq_unpack_tiles(const void *packed, size_t packed_bytes, const int8_t *map, const uint32_t *offsets, int64_t rows, int64_t cols,
                     void *y, int out_dtype, int64_t ldy, void *stream);

/* The transposed pair: a weight stored rows × cols whose packed form is the stream of its TRANSPOSE.  A map over the transposed layout of
 * W (a shared exponent per 16 rows of one column) is by definition a row-layout map of Wᵀ over Wᵀ's tile grid
 * ceil(cols/32) × ceil(rows/32), numbered row-major as mtq_tile_stats_transposed numbers it (element (r, c) of W lies in tile
 * (c / 32) * ceil(rows / 32) + r / 32).  So the packed transposed weight is the format above of the cols × rows matrix Wᵀ: no new byte
 * format, no new layout value.  These entries read and write W's own orientation; no transposed copy is made.
 *
 * mtq_pack_tiles_transposed: w (in_dtype, rows × cols as stored, pitch ld >= cols), map and offsets over Wᵀ's grid → out, byte for byte
 * what mtq_pack_tiles writes for a contiguous copy of Wᵀ with the same map.  One wave per tile, one lane per group; a lane's 16 values
 * are 16 consecutive rows of one column of w, rows and columns past the edge read +0; the blob checks against out_bytes are
 * mtq_pack_tiles's.
 * mtq_unpack_tiles_transposed: the mirror image, the stream of Wᵀ → y (rows × cols, ldy >= cols).  MTQ_DTYPE_F32: bit for bit what
 * mtq_apply_assignment_transposed writes for the packed w and map; MTQ_DTYPE_BF16: the upper halves.  Nothing is stored outside
 * rows × cols, nor for a tile whose blob passes packed_bytes.
 * Argument errors (null pointers, a dtype, rows or cols <= 0, ld < cols, a buffer below 320 bytes per tile, a stream that is not 16-byte
 * aligned) are MTQ_ERR_INVALID before a device is looked for.  Optional symbols. */
int mtq_pack_tiles_transposed(const void *w, int in_dtype, int64_t rows, int64_t cols, int64_t ld, const int8_t *map, const uint32_t *offsets,
                              void *out, size_t out_bytes, void *stream);
int mtq_unpack_tiles_transposed(const void *packed, size_t packed_bytes, const int8_t *map, const uint32_t *offsets, int64_t rows, int64_t cols,
                                void *y, int out_dtype, int64_t ldy, void *stream);

/* The batch: `count` tensors of one shape into ONE arena, tensor i's stream at byte 64 * bases[i], with no host work per tensor.  All
 * pointers are device pointers and the calls are asynchronous on `stream`.
 *
 * The offsets entry is the device counterpart of the host offsets function for `count` maps of `tiles` int8 codes each, contiguous:
 * offsets[count][tiles + 1] uint32, row i the same numbers the host function gives for map i; bases[count + 1] uint64, the exclusive
 * prefix sum over tensors of offsets[i][tiles] (units of 64 bytes; 64 * bases[count] is the arena's length); bad[count] int32, the
 * number of codes outside 0..3 in map i.  Such a tile counts 0 units (the host function refuses it: read `bad` before trusting row i).
 * Two kernels on `stream` (one workgroup per tensor, then one workgroup over the totals); plain stores, no atomics, no waiting between
 * workgroups: deterministic.  tiles > MTQ_PACKED_BATCH_MAX_TILES (a tensor's stream must fit 32-bit units) is MTQ_ERR_INVALID.
 *
 * The pack entry: x holds `count` rows × cols matrices (in_dtype, row pitch ld >= cols), matrix i starting i * stride elements in
 * (stride >= (rows - 1) * ld + cols when count > 1).  One wave per (tensor, tile); tile t of tensor i goes to
 * out + 64 * (bases[i] + offsets[i][t]), byte for byte what the single-tensor entry writes for matrix i.  Every blob is checked
 * against out_bytes on the device before it is written and a tile whose code is outside 0..3 is skipped.  The 16-byte loads are taken
 * only when x, ld and stride keep every matrix 16-byte aligned.
 *
 * The unpack entry is the mirror image: the arena → y[count][rows][cols] (out_dtype, row pitch ldy, matrix stride in elements), with
 * the edge handling of the single-tensor entry: nothing is stored outside rows × cols, nor for a tile whose blob does not fit
 * packed_bytes.
 *
 * Argument errors (null pointers, count <= 0, ld < cols, a buffer below 320 bytes per tile, an arena that is not 16-byte aligned) are
 * MTQ_ERR_INVALID before a device is looked for. */
#define MTQ_PACKED_BATCH_MAX_TILES ((int64_t)(0xFFFFFFFFu / 32u))
int mtq_packed_offsets_batched(const int8_t *maps, int64_t count, int64_t tiles, uint32_t *offsets, uint64_t *bases, int32_t *bad, void *stream);
int mtq_pack_tiles_batched(const void *x, int in_dtype, int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
                           const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, void *out, size_t out_bytes, void *stream);
int mtq_unpack_tiles_batched(const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases,
                             int64_t count, int64_t rows, int64_t cols, void *y, int out_dtype, int64_t ldy, int64_t stride, void *stream);
/* The batch in the transposed layout: the two entries above with the transposed pair's meaning.  w (y) holds `count` matrices, each
 * rows × cols AS STORED (row pitch ld / ldy >= cols, matrix i starting i * stride elements in); maps[count][tiles] and
 * offsets[count][tiles + 1] with tiles = ceil(cols/32) * ceil(rows/32) are over the grid of the TRANSPOSE, numbered as
 * mtq_pack_tiles_transposed numbers it; mtq_packed_offsets_batched produces offsets and bases for them as for any maps.
 *
 * mtq_pack_tiles_transposed_batched: tile t of tensor i goes to out + 64 * (bases[i] + offsets[i][t]), byte for byte what
 * mtq_pack_tiles_transposed writes for matrix i alone.  One wave per (tensor, tile) under the launch cap of the batched entries
 * (a grid-stride loop); plain stores, no atomics: deterministic.  The wave reads the tile's 32 × 32 region of w by rows - 16-byte loads
 * when w, ld and stride keep every matrix 16-byte aligned and the region lies inside rows × cols, element by element otherwise (ragged
 * edges, unaligned views), +0 past rows or cols - into a wave-private padded LDS image, and each lane gathers its group's 16 values down a column of the image.
 * mtq_unpack_tiles_transposed_batched: the arena → y[count][rows][cols] in W's orientation.  MTQ_DTYPE_F32: bit for bit what
 * mtq_apply_assignment_transposed writes; MTQ_DTYPE_BF16: the upper halves.
 *
 * The guards are the batched entries': every blob is checked against the buffer's length on the device before it is touched, a tile
 * whose code is outside 0..3 is skipped alone, nothing is stored outside rows × cols.  Argument errors (null pointers, a dtype,
 * count <= 0, ld < cols, a stride below one matrix when count > 1, a buffer below 320 bytes per tile, an arena that is not 16-byte
 * aligned) are MTQ_ERR_INVALID before a device is looked for.  Optional symbols (0.1.4.10; the number stays 143). */
int mtq_pack_tiles_transposed_batched(const void *w, int in_dtype, int64_t count, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
                                      const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, void *out, size_t out_bytes,
                                      void *stream);
int mtq_unpack_tiles_transposed_batched(const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                        const uint64_t *bases, int64_t count, int64_t rows, int64_t cols, void *y, int out_dtype, int64_t ldy,
                                        int64_t stride, void *stream);
/* Y = X·Ŵᵀ + b: x m × k bf16 (ldx), Ŵ the packed n × k weight (nn.Linear convention; map grid ceil(n/32) × ceil(k/32)), bias n
 * float32 or NULL, y m × n float32 or bf16 (out_dtype, ldy).  The weight is decoded into a bf16 LDS image (exact) and multiplied by
 * mfma_f32_32x32x16_bf16 with f32 accumulation in a fixed K order; bias is added in f32, a bf16 y is rounded to nearest even once.
 * No atomics: two calls give the same bits.  Any m >= 1. */
int mtq_packed_linear(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                      const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream);
/* The same product from a wider block, for m above the decode range (prefill): mtq_packed_linear's parameters, argument checks and
 * refusals.  A workgroup of 4 waves (2 x 2) owns 128 (M) x 128 (N) outputs and walks K in steps of 64, a wave 64 x 64 outputs in four
 * accumulators, two workgroups to a CU; a wave decodes whole tiles of the weight (one format per wave, no divergence).  Two LDS images
 * and two register sets: while one step multiplies, the next is decoded into the other image, and the loads of the step after that
 * are issued two steps ahead in program order, the map codes and offsets a step further (how far the compiler's waits let them run
 * beside the MFMAs: DESIGN.md A.6k; today a step still waits for the loads it has just issued).
 *
 * Bit contract: for every input the result equals mtq_packed_linear's bit for bit, in both output types, with and without bias.  An
 * output has one accumulator that starts at +0 and takes mfma_f32_32x32x16_bf16 over ascending blocks of 16 K positions, x as the A
 * operand and the decoded weight as B, K zero-filled to the step, the bias added once in f32, a bf16 y rounded once: the block
 * kernel's sequence for that output.  The guards are the block kernel's too: a tile whose blob passes packed_bytes or whose map code is
 * outside 0..3 multiplies as zeros, rows at or past m and columns at or past k of x are never read, nothing outside m x n of y is
 * written, any ldx / ldy (x is read by 16-byte loads when it is 16-byte aligned with ldx % 8 == 0 and k % 8 == 0, element by element
 * otherwise).  No atomics, no workspace, nothing waits on another workgroup: two calls give the same bits.
 *
 * Correct for any m >= 1 and measured faster than mtq_packed_linear from m = 64 on (below that nothing was measured; m <= 32 is the
 * skinny entry's).  m = 0 and n = 0 are refused as by the block entry: an empty product is the caller's, and the Python binding
 * returns it without a call. */
int mtq_packed_linear_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                           const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream);

/* Y = X·P̂ + b for a packed k × n matrix P̂ (input-major weights, y = x @ W; and the transposed layout of an n × k weight, whose stream
 * is that of its k × n transpose: mtq_pack_tiles_transposed): x m × k bf16 (ldx), map grid ceil(k/32) × ceil(n/32), bias n float32 or
 * NULL, y m × n (out_dtype, ldy).  Argument checks, refusals and device guards are mtq_packed_linear's: a tile whose blob passes
 * packed_bytes or whose map code is outside 0..3 multiplies as zeros in its own tile only, rows at or past m and columns at or past k of
 * x are never read, k-rows of P̂ at or past k count as zeros, nothing outside m x n of y is written.
 *
 * mtq_packed_linear's frame (4 waves, 128 (M) x 64 (N), K steps of 64, the fetch one step ahead, mfma_f32_32x32x16_bf16 into two
 * accumulators per wave, its epilogue).  A group's 16 values run along n at one k here, so a lane stores its decoded group as it lies
 * into a [k][n] LDS image and the B operand (8 consecutive k at one n) is read from it with the transposed LDS read of gfx950, two
 * reads per operand.
 *
 * Bit contract: for every input, y equals bit for bit what mtq_packed_linear gives for the same x and bias with the all-bf16 row-layout
 * packing of unpack(P̂)ᵀ (n × k; lossless, every decoded value is a bf16), in both output types, with or without bias.  The operand
 * positions are the block kernel's: the same k at the same lane half and element, the same order of 16-blocks, the same K step.
 * No atomics, no workspace: two calls give the same bits.  Any m >= 1.  Optional symbol. */
int mtq_packed_matmul(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                      const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream);

/* mtq_packed_matmul's product from the wide block of mtq_packed_linear_wide, for m above the decode range: the same parameter list,
 * argument checks, error texts and device guards (m = 0 and n = 0 are refused there: an empty product is the caller's, and the Python
 * binding returns it without a call).  A workgroup of 4 waves, 2 x 2, owns 128 (M) x 128 (N) outputs and walks K in steps of 64; a
 * step's block of P̂ is 2 tile rows x 4 tile columns, wave w decodes whole tiles of tile column n0 / 32 + w (a lane the group of its own
 * number, the format uniform over the wave) and stores each group as it lies into its own [64 k][32 n] LDS sub-image; the B operand is
 * read from two sub-images with the transposed LDS read of gfx950, two reads per operand.  X staging, two register sets, two LDS
 * images, loads two steps ahead and one barrier per step are the wide linear kernel's.
 *
 * Bit contract: for every input, y equals mtq_packed_matmul's bit for bit, in both output types, with and without bias.  By that
 * entry's contract it is also mtq_packed_linear_wide / mtq_packed_linear on the all-bf16 packing of unpack(P̂)ᵀ.  It holds by
 * construction: the same k at the same lane half and element, ascending blocks of 16 K positions, the same K step, zeros at and past k
 * (in the image, whatever the stream holds there).  No atomics, no workspace, nothing waits on another workgroup: two calls give the
 * same bits.  Correct for any m >= 1.  Optional symbol: a build of this version may lack it. */
int mtq_packed_matmul_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                           const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, void *stream);

/* The same product for decode, 1 <= m <= MTQ_PACKED_SKINNY_MAX_M: a split over K.  One wave takes the run of tiles of one tile row over
 * one K slice (a contiguous byte range of the stream), loads it straight to registers several tiles ahead, decodes each lane's group to
 * the same bf16 words as the block kernel and feeds them to mfma_f32_32x32x16_bf16 directly (no LDS).  The K range is cut into `split`
 * slices of whole tile columns (a split above tiles_w acts as tiles_w; split 0 is the library's choice, a pure function of (m, n, k));
 * with an effective split above 1 each slice writes its f32 partial into `workspace` and a second kernel on `stream` sums the partials
 * of an output in ascending slice order from slice 0, adds the bias last in f32 and rounds a bf16 y to nearest even once.  An effective
 * split of 1 writes y directly and touches no workspace.
 *
 * Numerics: a fixed order, no atomics - the same inputs and the same split give the same bits.  |Y - Y64| <= (k + 2) * 2^-24 *
 * (sum |x||w^| + |b|), the block kernel's bound, which holds for any summation order.  The skinny and the block kernel sum in different
 * orders: their results may differ in the last bits, and so may results under different splits.
 *
 * Arguments are checked as for the block kernel, and m > MTQ_PACKED_SKINNY_MAX_M, a negative split, and - when the size function's
 * answer is nonzero - a workspace that is null, not 16-byte aligned or shorter than that answer are MTQ_ERR_INVALID before a device is
 * looked for.  The workspace's contents on entry mean nothing and nothing the call leaves there is needed by a later call; calls that
 * share a workspace must be ordered on one stream. */
#define MTQ_PACKED_SKINNY_MAX_M 32
/* HOST function: bytes of workspace the skinny linear needs for (m, n, k, split); split 0 = the library's choice.  0 when the effective
 * split is 1.  MTQ_ERR_INVALID arguments give (size_t)-1. */
size_t mtq_packed_linear_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
int mtq_packed_linear_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                             const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, int split,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The skinny product with a packed k × n matrix P̂, Y = X·P̂ + b for 1 <= m <= MTQ_PACKED_SKINNY_MAX_M: mtq_packed_matmul's operands (x
 * m × k bf16, map grid ceil(k/32) × ceil(n/32), bias n float32 or NULL, y m × n) with mtq_packed_linear_skinny's parameter list, split
 * and workspace, one for one.  One wave takes one tile column of P̂ (32 outputs) over one K slice of whole tile rows; the map codes and
 * offsets of up to 64 tiles of the run come with one strided load, the loads of W and X run several tiles ahead.  A group's 16 values
 * run along n at one k here, so a lane stores its decoded group as it lies into a wave-private [32 k][32 n] LDS image and the two B
 * operands of the tile are read from it with the transposed LDS read of gfx950, two reads per operand; two images per wave, no
 * workgroup barrier.  Split, partials, reduce, bias and rounding are the skinny linear's with tiles_h = ceil(n/32), tiles_w = ceil(k/32):
 * a split above ceil(k/32) acts as ceil(k/32), split 0 is the same pure function of (m, n, k), an effective split of 1 writes y directly.
 *
 * Bit contract: for every input, y equals bit for bit what mtq_packed_linear_skinny gives, at the same split (split 0 included), for
 * the same x and bias with the all-bf16 row-layout packing of unpack(P̂)ᵀ (n × k; lossless, every decoded value is a bf16), in both
 * output types, with or without bias.  It holds by construction: the same k at the same lane half and element of each MFMA, the same
 * tile order, the same slices (the linear kernel's tile columns are this kernel's tile rows), the same split rule and the same reduce.
 * No atomics, no counters: the same inputs and the same split give the same bits.
 *
 * Argument checks and refusals are the skinny linear entry's (m > MTQ_PACKED_SKINNY_MAX_M, a negative split, a workspace that is null,
 * not 16-byte aligned or short) with mtq_packed_matmul's grid check for a k × n tensor, all before a device is looked for.  Device
 * guards: a tile whose blob passes packed_bytes or whose map code is outside 0..3 multiplies as zeros in its own tile only, k-rows of P̂
 * at or past k count as zeros whatever their bytes hold, rows at or past m and columns at or past k of x are never read, nothing outside
 * m x n of y is written.  The size function equals the skinny linear's for the same (m, n, k, split): n outputs, k contraction.
 * Both symbols are optional: a build of this version may lack them. */
size_t mtq_packed_matmul_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
int mtq_packed_matmul_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *packed, size_t packed_bytes, const int8_t *map,
                             const uint32_t *offsets, int64_t n, const float *bias, void *y, int out_dtype, int64_t ldy, int split,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The grouped form: `count` experts of one (n, k) shape in ONE arena (the batch entries' maps / offsets / bases), each multiplied with
 * its own rows of x, in one launch: y[rows of group e] = x[rows of group e] · Ŵ[e]ᵀ (+ bias[e]).
 *
 * group_rows is a DEVICE array of count + 1 int32: group e owns rows [group_rows[e], group_rows[e + 1]) of x and of y (both
 * total_rows rows).  The kernels clamp before any use, r0 = clamp(group_rows[e], 0, total_rows), r1 = clamp(group_rows[e + 1], r0,
 * total_rows): whatever the array holds, no row at or past total_rows is read or written.  A group without rows reads nothing of its
 * expert.  Rows of y that belong to no group are not written.  Nondecreasing group_rows give disjoint groups, and then the same inputs
 * and the same split give the same bits.  An array that decreases can clamp to groups that OVERLAP: several waves then write the
 * overlapped rows of y (and of the workspace) without an order among them, so the values left in those rows are unspecified - inside
 * the allocation, and every other row as stated.  Group e reads maps[e * tiles ..], offsets[e * (tiles + 1) ..] and the
 * stream at byte 64 * bases[e]; a blob is checked on the device against its group's own stream [64 * bases[e], 64 * bases[e + 1]) and
 * against packed_bytes and reads as zeros when it passes either, as does a tile whose map code is outside 0..3.
 *
 * One wave per (slice, group, tile row); a group above 32 rows is walked in chunks of 32 rows by the same wave, which reads the weight
 * again for every chunk: the entry is for decode-sized groups, and mtq_packed_linear per expert is the route for large m (for all
 * experts in one launch: mtq_packed_linear_wide_grouped, below).  For every
 * group and every 32-row chunk of it the result is bit for bit what mtq_packed_linear_skinny gives for that chunk and that expert's
 * stream and tables at the same effective split.  An effective split above 1 writes f32 partials to workspace[slice][total_rows][n]
 * with plain stores and a second kernel on `stream` sums them in ascending slice order, adds the group's bias last and rounds a bf16 y
 * once; it writes only rows inside a clamped group.  No atomics, no counters, no waiting between workgroups; nothing in the workspace
 * needs initialising.  split 0 is the library's choice: the single-tensor rule with count * tiles_h tile rows (for count == 1 the same
 * split).  bias: NULL, or count rows of n floats at pitch ldb.
 *
 * Arguments are checked as for the skinny entry (null pointers, total_rows, count, n, k positive, the tile grid, a negative split, an
 * arena below 320 bytes per tile or not 16-byte aligned, a workspace that is null, misaligned or too small when the size function's
 * answer is nonzero): MTQ_ERR_INVALID before a device is looked for. */
/* HOST function: bytes of workspace for (total_rows, count, n, k, split): 0 when the effective split is 1, else
 * split_eff * total_rows * n * 4 rounded up to 16.  MTQ_ERR_INVALID arguments give (size_t)-1. */
size_t mtq_packed_linear_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_linear_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                     size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, int64_t count,
                                     int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, int split,
                                     void *workspace, size_t workspace_bytes, void *stream);
/* The grouped form with a wave per 32-row CHUNK, for routings with hot experts: the same product, parameters (in the same order),
 * argument checks and refusals as mtq_packed_linear_skinny_grouped, and the same bits.  The entry above gives a group's chunks to one
 * wave, one after another, so an expert of hundreds of rows is the critical path of the launch; here a unit is (slice, 32-row chunk of a
 * group, tile row), a wave each.  The chunk list comes from group_rows ON THE DEVICE: a one-workgroup plan kernel on `stream` clamps
 * the groups as above, forms chunks_e = ceil((r1 - r0) / 32) and writes their exclusive prefix sum, count + 1 int32, into the head of
 * the workspace; the main kernel follows on `stream`, and each of its waves finds its chunk's group by a search of that prefix.  Nothing
 * is read back: the grid covers U = floor((total_rows + 31 * min(count, total_rows)) / 32) chunk slots, a bound that holds for disjoint
 * groups (a group with rows adds at most 31/32 of a chunk) and is formed from the arguments alone; a wave whose slot is past the last
 * chunk returns before any other load.
 *
 * Contract.  For nondecreasing group_rows the result equals mtq_packed_linear_skinny_grouped's bit for bit at the same `split` (the
 * effective split of every (count, n, k, split), 0 included, is that entry's), in both output types, with and without bias: the wave
 * does on its chunk what that entry's wave does on it.  Rows of y that belong to no group are not written.  Whatever group_rows holds,
 * nothing outside total_rows x n of y or outside the workspace is written and no row of x at or past total_rows is read.  An array
 * that decreases can clamp to groups that overlap; their chunks can then number more than U, the chunks past U are not computed, and
 * the rows of the overlapping groups are unspecified, as above, inside the allocation; every row of a group that overlaps no other
 * and whose chunks lie below U is as stated.  Deterministic: no atomics, no counters, no waiting between workgroups; nothing in the
 * workspace needs initialising and nothing the call leaves there is needed by a later call (calls that share a workspace must be
 * ordered on one stream).
 *
 * The workspace is NEVER empty: the size function's answer is the entry above's for the same arguments plus a plan region of
 * (count + 1) * 4 bytes rounded up to 16 (a function of count alone), the plan first and the f32 partials behind it.  A workspace that
 * is null, not 16-byte aligned or shorter than that answer is MTQ_ERR_INVALID before a device is looked for, at every split.
 *
 * Both symbols are optional: a build of this version may lack them. */
/* HOST function: bytes of workspace for (total_rows, count, n, k, split), never 0.  MTQ_ERR_INVALID arguments give (size_t)-1. */
size_t mtq_packed_linear_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_linear_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                             const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                             const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                             int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);
/* The grouped form of mtq_packed_linear_wide, for experts that hold hundreds of rows (MoE prefill): the parameters of
 * mtq_packed_linear_skinny_grouped_chunked in its order, without `split` - there is no split over K and there are no partial sums.  The
 * two entries above run the skinny kernel's wave on 32 rows at a time, so an expert's stream is read and decoded once per 32 rows; here a
 * workgroup owns 128 rows x 128 columns of ONE group and does on them what mtq_packed_linear_wide's workgroup does, so the stream is
 * decoded once per 128 rows.  The block list comes from group_rows ON THE DEVICE, as the chunked entry's chunk list does: a one-workgroup
 * plan kernel on `stream` clamps the groups as above, forms blocks_e = ceil((r1 - r0) / 128) and writes their exclusive prefix sum,
 * count + 1 int32 saturated at INT32_MAX, into the head of the workspace; the main kernel follows on `stream` and each of its
 * workgroups finds its block's group by the chunked kernel's search of that prefix.  Nothing is read back: the grid covers
 * U = floor((total_rows + 127 * min(count, total_rows)) / 128) row-block slots (times ceil(n / 128) column blocks, the column block
 * fastest), a bound that holds for disjoint groups (a group with rows adds at most 127/128 of a block) and is formed from the arguments
 * alone; a workgroup whose slot is past the last block returns before any other load and before any barrier.
 *
 * Bit contract.  For nondecreasing group_rows and every group with rows, y[r0:r1] equals bit for bit what mtq_packed_linear gives for
 * x[r0:r1] with expert e's stream and tables (and bias row e); mtq_packed_linear_wide gives the same bits.  This holds in both output
 * types, with and without bias, and for any ldx / ldy (x is read by 16-byte loads when it is 16-byte aligned with ldx % 8 == 0 and
 * k % 8 == 0, element by element otherwise).  These are the BLOCK family's bits, not the skinny family's: the two families sum in
 * different orders, so this entry and the two grouped entries above may differ in the last bits, which is why it is an entry of its own.
 * Rows of y that belong to no group are not written.  Whatever group_rows holds, nothing outside total_rows x n of y or outside the
 * workspace is written and no row of x at or past total_rows is read: every row limit of a block is its group's clamped end.  A blob is
 * checked on the device against its group's own stream [64 * bases[e], 64 * bases[e + 1]) and against packed_bytes and multiplies as
 * zeros when it passes either, as does a tile whose map code is outside 0..3; what the kernel loads for such a tile comes from the
 * arena's first 320 bytes.  An array that decreases can clamp to groups that overlap; their blocks can then number more than U, the
 * blocks past U are not computed, and the rows of the overlapping groups are unspecified inside the allocation; every row of a group
 * that overlaps no other and whose blocks lie below U is as stated.  Deterministic: no atomics, no counters, nothing waits on another
 * workgroup; nothing in the workspace needs initialising and nothing the call leaves there is needed by a later call (calls that share
 * a workspace must be ordered on one stream).
 *
 * The workspace holds the plan only: (count + 1) * 4 bytes rounded up to 16, a function of count alone, never 0.  Arguments are
 * checked as by the chunked entry, minus the split (null pointers, total_rows, count, n, k positive, the tile grid, ldx / ldy / ldb, an
 * arena below 320 bytes per tile or not 16-byte aligned, a workspace that is null, not 16-byte aligned or too short):
 * MTQ_ERR_INVALID before a device is looked for.
 *
 * Both symbols are optional: a build of this version may lack them. */
/* HOST function: bytes of workspace for (total_rows, count, n, k): the plan region, never 0.  MTQ_ERR_INVALID arguments give (size_t)-1. */
size_t mtq_packed_linear_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k);
int mtq_packed_linear_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                   size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, int64_t count,
                                   int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ grouped matmul: (k, n) experts of one arena in one launch
 * The three grouped entries above for experts stored as packed k x n tensors (mtq_packed_matmul's weight: the transposed BFP layout, or
 * an input-major weight): `count` experts of one (k, n) shape in ONE arena (mtq_pack_tiles_transposed_batched's or
 * mtq_pack_tiles_batched's maps / offsets / bases), each multiplied with its own rows of x:
 *   y[r0:r1] = x[r0:r1] · P̂[e] (+ bias[e]),   P̂[e] the packed k x n expert e.
 * n is the output width and k the contraction.  The map grid of an expert is ceil(k/32) x ceil(n/32), tiles_kh x tiles_nw;
 * tiles = tiles_kh * tiles_nw is the stride of maps and tiles + 1 that of offsets.  The parameter list of each entry is that of the
 * mtq_packed_linear_*_grouped* entry of the same name, one for one and in the same order, and group_rows, its clamping, overlapping
 * groups (unspecified rows inside the allocation), rows of no group (not written), bias, ldb and the workspace rules are as stated
 * there.
 *
 * mtq_packed_matmul_skinny_grouped: mtq_packed_matmul_skinny's wave, one per (slice, group, tile column) - 32 output columns over
 * one K slice of whole tile rows of expert e's tables, through two wave-private [32 k][32 n] LDS images and the transposed LDS read; a
 * group above 32 rows is walked in chunks of 32 rows by the same wave.  The effective split and the size function are
 * mtq_packed_linear_skinny_grouped's for the same (total_rows, count, n, k, split): the single-tensor rule with count * ceil(n/32)
 * output tile rows and ceil(k/32) contraction tiles.  An effective split above 1 writes f32 partials to
 * workspace[slice][total_rows][n] and the grouped linear entry's reduce kernel finishes.
 *
 * mtq_packed_matmul_skinny_grouped_chunked: the same wave per (slice, 32-row chunk slot, tile column); the chunk list, the slot bound
 * U, the early return of surplus waves, the search and the never-empty workspace (plan first, partials behind) are
 * mtq_packed_linear_skinny_grouped_chunked's, and so is the size function's answer.
 *
 * mtq_packed_matmul_wide_grouped: mtq_packed_matmul_wide's 128 x 128 block in mtq_packed_linear_wide_grouped's frame - the block plan
 * on the device, U x ceil(n/128) workgroups with the column block fastest, every row limit the group's clamped end; the workspace holds
 * the plan only.
 *
 * Bit contracts.  For nondecreasing group_rows and every group with rows:
 *  - both skinny entries equal, bit for bit, what mtq_packed_matmul_skinny gives for each 32-row chunk of the group with expert e's
 *    stream and tables (and bias row e) at the same effective split; they therefore equal each other, and they equal
 *    mtq_packed_linear_skinny_grouped on the arena of the all-bf16 row-layout packings of unpack(P̂[e])ᵀ at the same `split`, 0 included
 *    (mtq_packed_matmul_skinny's contract, chunk by chunk; the split rules are the same function of the same arguments);
 *  - the wide entry equals what mtq_packed_matmul gives for x[r0:r1] with expert e's stream and tables, which mtq_packed_matmul_wide
 *    gives too: the block family's bits, not the skinny family's.
 * In both output types, with and without bias, for any ldx / ldy.  Deterministic: no atomics, no counters, nothing waits on another
 * workgroup, nothing in a workspace needs initialising.
 *
 * Device guards: a tile whose blob passes its group's [64 * bases[e], 64 * bases[e + 1]) or packed_bytes, or whose map code is outside
 * 0..3, multiplies as zeros in its own tile only; k-rows of P̂[e] at or past k count as zeros whatever their bytes hold; a chunk's (a
 * block's) rows end at its group's clamped end for every load of x; columns at or past n are never stored.
 *
 * Argument checks are the grouped linear entries', with mtq_packed_matmul's grid check for a k x n tensor (null pointers, total_rows,
 * count, n, k positive, a negative split, ldx < k, ldy < n, ldb < n, an arena below 320 bytes per tile or not 16-byte aligned, a
 * workspace that is null, not 16-byte aligned or too short where one is needed): MTQ_ERR_INVALID before a device is looked for.
 *
 * All six symbols are optional: a build of this version may lack them. */
/* HOST functions: bytes of workspace, equal to the mtq_packed_linear_*_grouped* answer for the same arguments; (size_t)-1 for
 * MTQ_ERR_INVALID arguments. */
size_t mtq_packed_matmul_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_matmul_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                     size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, int64_t count,
                                     int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, int split,
                                     void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_matmul_skinny_grouped_chunked_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_matmul_skinny_grouped_chunked(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                             const void *packed, size_t packed_bytes, const int8_t *maps, const uint32_t *offsets,
                                             const uint64_t *bases, int64_t count, int64_t n, const float *bias, int64_t ldb, void *y,
                                             int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_matmul_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k);
int mtq_packed_matmul_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows, const void *packed,
                                   size_t packed_bytes, const int8_t *maps, const uint32_t *offsets, const uint64_t *bases, int64_t count,
                                   int64_t n, const float *bias, int64_t ldb, void *y, int out_dtype, int64_t ldy, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ gated MLP (SwiGLU) on packed weights
 * h = act(x·Ŵgᵀ + bg) * (x·Ŵuᵀ + bu), the first half of down(act(gate(x)) * up(x)), with the gate and the up projection as two
 * packed (n, k) weights of the format above (nothing is repacked: the tile rows of a packed weight are independent blobs).
 *
 * The activation is one device function (csrc/mtq_glu.hpp, glu_value) that every entry below calls, all in separately rounded float32
 * operations, no contraction:
 *   MTQ_ACT_SILU  h = (g / (1 + expf(-g))) * u, the accurate expf
 *   MTQ_ACT_NONE  h = g * u, one rounding (the bilinear GLU)
 * Inf, NaN and -0 get no special case: what the sequence gives is the definition.  Any other code is MTQ_ERR_UNSUPPORTED.
 * All four symbols are optional: a build of this version may lack them. */
enum { MTQ_ACT_SILU = 0, MTQ_ACT_NONE = 1 };

/* y[r][c] = act(g[r][c]) * u[r][c] for float32 device matrices g and u of rows x cols at pitches ldg, ldu → y float32 or bf16
 * (out_dtype, pitch ldy; a bf16 y is rounded to nearest even once).  Asynchronous on `stream`; nothing outside rows x cols of y is
 * written.  Null pointers, rows or cols not positive, a pitch below cols and an out_dtype that is neither are MTQ_ERR_INVALID before a
 * device is looked for.  The second half of the unfused route, and the yardstick of the bit contract below. */
int mtq_glu_combine(const float *g, int64_t ldg, const float *u, int64_t ldu, int64_t rows, int64_t cols, int act, void *y, int out_dtype,
                    int64_t ldy, void *stream);

/* The gated product in one launch from mtq_packed_linear_wide's step: x, m, k, ldx as there; (gate_packed, gate_bytes, gate_map,
 * gate_offsets) and the same four for up, both n x k; bias_gate, bias_up float32 [n], each may be NULL; y m x n (out_dtype, ldy).  A
 * workgroup of 4 waves owns 128 rows x 64 HIDDEN columns (the grid is ceil(m / 128) x ceil(n / 64)); the four tile-row slots of its
 * weight image alternate between the two streams, so each lane holds the gate's and the up's accumulator of the same output and
 * applies the activation itself: the two float32 (m, n) intermediates never reach memory and x is read once.
 *
 * Bit contract: for every input, y equals bit for bit the result of (1) mtq_packed_linear on the gate stream with bias_gate into
 * float32, (2) the same on the up stream with bias_up, (3) mtq_glu_combine of the two.  This holds in both output types, with or
 * without either bias, and for any ldx / ldy.  The guards are the wide kernel's, per stream: a tile whose blob passes its own stream's
 * packed_bytes or whose map code is outside 0..3 multiplies as zeros in its own projection only; rows at or past m and columns at or
 * past k of x are never read; nothing outside m x n of y is written.  No atomics, no workspace, nothing waits on another workgroup: two
 * calls give the same bits.
 *
 * Arguments are checked as by mtq_packed_linear_wide, for each stream (null pointers, m, n, k positive, the tile grid, ldx / ldy, a
 * stream below 320 bytes per tile or not 16-byte aligned): MTQ_ERR_INVALID before a device is looked for.  m = 0 and n = 0 are
 * refused as there; the Python binding returns the empty result without a call.  Correct for any m >= 1; m <= 32 is better served by
 * the split-K entries: two skinny calls and the combine, or mtq_packed_glu_skinny below, which is that sequence in two launches. */
int mtq_packed_glu_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes, const int8_t *gate_map,
                        const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes, const int8_t *up_map, const uint32_t *up_offsets,
                        int64_t n, const float *bias_gate, const float *bias_up, int act, void *y, int out_dtype, int64_t ldy, void *stream);

/* The same block in mtq_packed_linear_wide_grouped's frame, for the experts of an MoE layer: x, total_rows, k, ldx, group_rows as
 * there; two arenas (packed, bytes, maps, offsets, bases), one with the `count` gate experts and one with the `count` up experts, all
 * n x k; bias_gate, bias_up float32 (count, n) at pitch ldb, each may be NULL.  The plan kernel, the slot bound U, the early return of
 * surplus workgroups before any other load or barrier, the clamping of group_rows and the workspace (its size included) are that
 * entry's; the grid is U x ceil(n / 64).
 *
 * Bit contract: for nondecreasing group_rows and every group with rows, y[r0:r1] equals bit for bit the three-step sequence above on
 * x[r0:r1] with expert e's gate and up streams and tables (and bias rows e).  Rows of y that belong to no group are not written.  A
 * blob is checked against its own group's range [64 * bases[e], 64 * bases[e + 1]) of its OWN arena and against that arena's bytes,
 * and multiplies as zeros in its own projection only when it passes either.  Whatever group_rows holds, nothing outside
 * total_rows x n of y or outside the workspace is written and no row of x at or past total_rows is read.  Deterministic, as there.
 * Arguments are checked as by that entry, for each arena. */
size_t mtq_packed_glu_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k);
int mtq_packed_glu_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows, const void *gate_packed,
                                size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets, const uint64_t *gate_bases,
                                const void *up_packed, size_t up_bytes, const int8_t *up_maps, const uint32_t *up_offsets,
                                const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate, const float *bias_up, int64_t ldb,
                                int act, void *y, int out_dtype, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream);

/* The gated product for decode, 1 <= m <= MTQ_PACKED_SKINNY_MAX_M: mtq_packed_linear_skinny's split over K with one more unit axis,
 * the projection.  Operands are mtq_packed_glu_wide's, followed by split, workspace and workspace_bytes as in the skinny entries.  A
 * wave takes one (slice, projection, tile row) unit, reads its own projection's stream exactly as the skinny linear wave does and
 * writes its float32 partial to the workspace; a second kernel on the same stream sums each projection's slices in ascending order
 * from slice 0, adds that projection's bias last, applies glu_value and stores y (one rounding for a bf16 y).  Two launches at every
 * split, against five for the two skinny calls and the combine; the two float32 (m, n) intermediates are not formed.
 *
 * split: 0 is the library's choice, mtq_packed_linear_skinny's rule for (m, n, k) unchanged (the projection axis is not counted
 * into it); any other value is clamped to the number of tile columns.  The workspace is never empty: 2 * max(split_eff, 1) * m * n
 * float32, rounded up to 16 bytes, the gate's partials first and the up's behind them; mtq_packed_glu_skinny_workspace_bytes gives
 * the size ((size_t)-1 on bad arguments).  Nothing in it needs initialising and nothing a call leaves there is needed later.
 *
 * Bit contract: for every input and every split (0 included), y equals bit for bit the result of (1) mtq_packed_linear_skinny on the
 * gate stream with bias_gate into float32 at that split, (2) the same on the up stream with bias_up, (3) mtq_glu_combine of the two.
 * This holds in both output types, with or without either bias, and for any ldx / ldy.  Guards: a tile whose blob passes its own
 * stream's packed_bytes or whose map code is outside 0..3 multiplies as zeros in its own projection only; rows at or past m and
 * columns at or past k of x are never read; nothing outside m x n of y or outside the workspace is written.  No atomics, no
 * counters, nothing waits on another workgroup: two calls give the same bits.
 *
 * Everything mtq_packed_linear_skinny refuses is refused here, for each stream, and so are m > MTQ_PACKED_SKINNY_MAX_M, a negative
 * split, and - at every split - a workspace that is NULL, not 16-byte aligned or shorter than the size function's answer:
 * MTQ_ERR_INVALID before a device is looked for.  An unknown act is MTQ_ERR_UNSUPPORTED.  Optional symbols, as the wide ones. */
size_t mtq_packed_glu_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
int mtq_packed_glu_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes, const int8_t *gate_map,
                          const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes, const int8_t *up_map,
                          const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up, int act, void *y, int out_dtype,
                          int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);

/* The same step on mtq_packed_linear_skinny_grouped, for the experts of an MoE layer at decode: mtq_packed_glu_wide_grouped's
 * operands with `split` in front of the workspace.  A unit is (slice, projection, group, tile row); a group's rows are clamped as
 * there and a group above 32 rows is walked in 32-row chunks by the same wave.  split 0 is mtq_packed_linear_skinny_grouped's rule
 * for (count, n, k) unchanged.  The workspace is 2 * max(split_eff, 1) * total_rows * n float32 rounded up to 16 bytes, laid out and
 * treated as above.
 *
 * Bit contract: for nondecreasing group_rows and every group with rows, y[r0:r1] equals bit for bit (1) mtq_packed_linear_skinny_grouped
 * on the gate arena with bias_gate into float32 at that split, (2) the same on the up arena with bias_up, (3) mtq_glu_combine of the
 * two.  Rows of y that belong to no group are not written.  A blob is checked against its own group's range
 * [64 * bases[e], 64 * bases[e + 1]) of its OWN arena and against that arena's bytes, and multiplies as zeros in its own projection
 * only when it passes either.  Whatever group_rows holds, nothing outside total_rows x n of y or outside the workspace is written
 * and no row of x at or past total_rows is read.  Deterministic, as above.  Arguments are checked as by
 * mtq_packed_linear_skinny_grouped, for each arena; the workspace and act as above. */
size_t mtq_packed_glu_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                  const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                  const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                  const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n, const float *bias_gate,
                                  const float *bias_up, int64_t ldb, int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ gated MLP on packed (k, n) weights
 * h = act(x·P̂g + bg) * (x·P̂u + bu) with the gate and the up projection as two packed k x n tensors (mtq_packed_matmul's weight: the
 * transposed BFP layout, an input-major weight, what the transposed pack entries write).  The four gated entries above with
 * the matmul family's feed: the parameter list of each entry is that of the mtq_packed_glu_* entry of the same name, one for one and in
 * the same order; n is the output (hidden) width, k the contraction, and the map grid of each tensor is ceil(k/32) x ceil(n/32),
 * tiles_kh x tiles_nw.  act, biases, group_rows and its clamping, rows of no group (not written), ldb and the workspace rules are as
 * stated there.
 *
 * mtq_packed_glu_matmul_wide: mtq_packed_matmul_wide's block on 128 rows x 64 hidden columns.  Wave w stages sub-image w of the
 * [64 k][32 n] weight part of the LDS image: hidden tile COLUMN n0/32 + (w >> 1), from the gate stream when w is even and from the up
 * stream when w is odd; wave (wm, wn) reads sub-images 2 wn and 2 wn + 1 through the transposed LDS read and so holds the gate's and
 * the up's accumulator of the same output: the activation is lane-local, the two float32 (m, n) intermediates never reach memory.  The
 * grid is ceil(m / 128) x ceil(n / 64); no workspace.
 * mtq_packed_glu_matmul_wide_grouped: the same block in mtq_packed_matmul_wide_grouped's frame over a gate arena and an up arena; the
 * grid is U x ceil(n / 64), the workspace holds the plan only.
 * mtq_packed_glu_matmul_skinny (1 <= m <= MTQ_PACKED_SKINNY_MAX_M): mtq_packed_matmul_skinny's wave, one per (slice, projection, tile
 * column), through two wave-private [32 k][32 n] LDS images; float32 partials to workspace[projection][slice][m][n] at every split,
 * mtq_packed_glu_skinny's reduce kernel finishes.  Two launches at every split, against five for the unfused route.
 * mtq_packed_glu_matmul_skinny_grouped: that wave per (slice, projection, group, tile column) in mtq_packed_matmul_skinny_grouped's
 * frame, a group above 32 rows walked in 32-row chunks; mtq_packed_glu_skinny_grouped's reduce kernel finishes.
 *
 * split: mtq_packed_matmul_skinny's and mtq_packed_matmul_skinny_grouped's rules for the same arguments; the projection axis is not
 * counted.  The size functions return the mtq_packed_glu_* answer for the same arguments ((size_t)-1 on bad arguments).
 *
 * Bit contracts, in both output types, with or without either bias, for any ldx / ldy:
 *  - wide: y equals bit for bit (1) mtq_packed_matmul on the gate stream with bias_gate into float32, (2) the same on the up stream
 *    with bias_up, (3) mtq_glu_combine of the two.  The grouped entry holds this per group with rows, on x[r0:r1] with expert e's gate
 *    and up streams and tables (and bias rows e), for nondecreasing group_rows.
 *  - skinny: the same with mtq_packed_matmul_skinny at the same effective split (0 included); the grouped entry per 32-row chunk of a
 *    group, i.e. with mtq_packed_matmul_skinny_grouped on each arena.
 *  - across the families: each entry equals the mtq_packed_glu_* entry of the same name on the all-bf16 row-layout packings of
 *    unpack(P̂g)ᵀ and unpack(P̂u)ᵀ, the skinny entries at the same `split` (the split rules are the same function of the same arguments).
 * Deterministic: no atomics, no counters, nothing waits on another workgroup, nothing in a workspace needs initialising.
 *
 * Device guards: a tile whose map code is outside 0..3 or whose blob passes its own stream's bytes - for an arena, its own group's
 * [64 * bases[e], 64 * bases[e + 1]) of its OWN arena, or that arena's bytes - multiplies as zeros in its own projection only; k-rows
 * at or past k count as zeros whatever their bytes hold; rows of x at or past m (a group's clamped end) are never read; columns at or
 * past n are never stored.
 *
 * Argument checks are the mtq_packed_glu_* entries', for each stream, with mtq_packed_matmul's grid check for a k x n tensor:
 * MTQ_ERR_INVALID before a device is looked for; an unknown act is MTQ_ERR_UNSUPPORTED.
 *
 * All seven symbols are optional: a build of this version may lack them. */
int mtq_packed_glu_matmul_wide(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                               const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                               const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up,
                               int act, void *y, int out_dtype, int64_t ldy, void *stream);
size_t mtq_packed_glu_matmul_wide_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k);
int mtq_packed_glu_matmul_wide_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                       const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                       const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                       const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                       const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y, int out_dtype,
                                       int64_t ldy, void *workspace, size_t workspace_bytes, void *stream);
size_t mtq_packed_glu_matmul_skinny_workspace_bytes(int64_t m, int64_t n, int64_t k, int split);
int mtq_packed_glu_matmul_skinny(const void *x, int64_t m, int64_t k, int64_t ldx, const void *gate_packed, size_t gate_bytes,
                                 const int8_t *gate_map, const uint32_t *gate_offsets, const void *up_packed, size_t up_bytes,
                                 const int8_t *up_map, const uint32_t *up_offsets, int64_t n, const float *bias_gate, const float *bias_up,
                                 int act, void *y, int out_dtype, int64_t ldy, int split, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t mtq_packed_glu_matmul_skinny_grouped_workspace_bytes(int64_t total_rows, int64_t count, int64_t n, int64_t k, int split);
int mtq_packed_glu_matmul_skinny_grouped(const void *x, int64_t total_rows, int64_t k, int64_t ldx, const int32_t *group_rows,
                                         const void *gate_packed, size_t gate_bytes, const int8_t *gate_maps, const uint32_t *gate_offsets,
                                         const uint64_t *gate_bases, const void *up_packed, size_t up_bytes, const int8_t *up_maps,
                                         const uint32_t *up_offsets, const uint64_t *up_bases, int64_t count, int64_t n,
                                         const float *bias_gate, const float *bias_up, int64_t ldb, int act, void *y, int out_dtype,
                                         int64_t ldy, int split, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ MoE routing: plan, dispatch, combine (csrc/mtq_moe.hip)
 * From what a router emits, topk_ids and topk_weights of (tokens, topk), to the row layout the grouped entries above take, and from
 * the experts' rows back to token order with the weighted sum.  Slot s = t * topk + j; S = tokens * topk.
 *
 * Plan.  A slot is live when 0 <= id < count; every other id (the INT32 / INT64 extremes included) is dropped: that is how expert
 * parallelism passes the ids of experts of another rank.  A token may name one expert twice: both slots are live and get a row each.
 *   group_rows  int32 [count + 1], the exclusive prefix sum of the live counts per expert; R = group_rows[count] <= S.
 *   row_of      int32 [S]: a live slot's row in expert order, stable (within an expert rows ascend with s); -1 for a dropped slot.
 *   src         int32 [S]: the inverse, src[row_of[s]] = s for live slots, and src[r] = -1 for every r in [R, S).
 * So src[0 .. R) is the stable argsort of the slots by expert with the dropped slots last.
 * Dispatch.  xs (S, k) bf16: xs[r] = x[src[r] / topk] when 0 <= src[r] < S, else the row is all +0: a bit copy.  Every one of the S
 * rows is written, so xs goes to the grouped entries with total_rows = S and the device group_rows as it is (rows at or past R belong
 * to no group); nothing is read back to the host.
 * Combine.  For token t and column c an accumulator of float32 starts at (float) base[t][c] when base is given (a shared expert's
 * output), else at +0; for j = 0 .. topk - 1 in that order, with r = row_of[t * topk + j]: if 0 <= r < S,
 * acc = fl32(acc + fl32(w[t][j] * (float) ys[r][c])), product and sum rounded separately (no contraction).  A slot with r outside
 * [0, S) is skipped, not multiplied by zero: an Inf in an unused row cannot reach y.  y is float32, or bf16 rounded to nearest even once.
 *
 * Limits: 1 <= topk <= MTQ_MOE_MAX_TOPK, 1 <= count <= MTQ_MOE_MAX_EXPERTS, tokens >= 1, S < 2^31; outside them, and for a null
 * pointer (base may be NULL), a pitch below its row, a pointer not aligned to its type or a dtype code that is none:
 * MTQ_ERR_INVALID before a device is looked for.  All launches are asynchronous on `stream`.  Deterministic: the only atomics are
 * integer LDS adds of a histogram, no kernel waits on another workgroup, and two calls give the same words.  The four symbols are
 * optional: a build of this version may lack them. */
enum { MTQ_IDS_I32 = 0, MTQ_IDS_I64 = 1 };
#define MTQ_MOE_MAX_TOPK 64
#define MTQ_MOE_MAX_EXPERTS 4096
#define MTQ_MOE_RUN 1024        /* slots one workgroup of the plan owns */

/* HOST function: bytes of workspace for a plan, ceil(S / MTQ_MOE_RUN) * count * 4 rounded up to 16 (the runs' histograms); never 0.
 * Arguments outside the limits give (size_t)-1. */
size_t mtq_moe_plan_workspace_bytes(int64_t tokens, int64_t topk, int64_t count);

/* topk_ids: device, int32 or int64 (id_dtype MTQ_IDS_I32 / MTQ_IDS_I64, read in their own width) at a row pitch of ld_ids >= topk
 * elements → group_rows, row_of, src (device, as above).  A stable counting sort: a one-wave workgroup owns a run of MTQ_MOE_RUN
 * consecutive slots; one kernel stores every run's histogram, one turns the histograms' columns into prefixes over the runs and
 * writes group_rows, one places the slots and fills src[R .. S) with -1.  S <= MTQ_MOE_RUN, every decode call, is ONE launch of one
 * workgroup that does all three and does not touch the workspace.  Nothing in the workspace needs initialising and nothing a call
 * leaves there is needed later; a workspace that is NULL, not 16-byte aligned or shorter than the size function's answer is
 * MTQ_ERR_INVALID at every size.  Nothing outside the three outputs and the first size-function bytes of the workspace is written; no
 * id is used as an index before it is checked against [0, count). */
int mtq_moe_plan(const void *topk_ids, int id_dtype, int64_t ld_ids, int64_t tokens, int64_t topk, int64_t count, int32_t *group_rows,
                 int32_t *row_of, int32_t *src, void *workspace, size_t workspace_bytes, void *stream);

/* x (tokens, k) bf16 at pitch ldx, src int32 [S] → xs (S, k) bf16 at pitch ldxs.  16-byte loads and stores when x and xs are 16-byte
 * aligned, ldx % 8 == 0, ldxs % 8 == 0 and k % 8 == 0; element by element otherwise, the same bits.  Whatever src holds, no row of x
 * at or past `tokens` is read and nothing outside S x k of xs is written (the pad of a pitched xs is left alone). */
int mtq_moe_dispatch(const void *x, int64_t tokens, int64_t k, int64_t ldx, const int32_t *src, int64_t topk, void *xs, int64_t ldxs,
                     void *stream);

/* ys (S, n) bf16 or float32 (ys_dtype) at pitch ldys, row_of int32 [S], weights float32 (tokens, topk) at pitch ldw, base NULL or
 * (tokens, n) bf16 / float32 (base_dtype, pitch ldbase; base_dtype and ldbase mean nothing without a base) → y (tokens, n) float32 or
 * bf16 (out_dtype, pitch ldy).  A lane owns 8 consecutive columns of one token; 16-byte accesses when n % 8 == 0 and every operand's
 * rows start 16-byte aligned, element by element otherwise, the same bits.  row_of is clamped as stated whatever it holds: no row of
 * ys outside [0, S) is read, a row of ys that no kept slot names is never read, and nothing outside tokens x n of y is written. */
int mtq_moe_combine(const void *ys, int ys_dtype, int64_t ldys, const int32_t *row_of, const float *weights, int64_t ldw, const void *base,
                    int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk, int64_t n, void *y, int out_dtype, int64_t ldy,
                    void *stream);

/* The MoE decode entries without the staging copies - the gather inside the gated product's X loads, the combine inside the down
 * projection's reduce - are declared in mtq_moe_decode.h, included at the end of this header: their contracts stand there, beside
 * this section's, which they refer to.  Their forms with a wave per 32-row chunk, for routings with hot experts, are declared in
 * mtq_glu_chunked.h, included after it. */

/* ------------------------------------------------------------------ MoE router: scoring and group-limited top-k (csrc/mtq_moe_route.hip)
 * From the router's logits (tokens, count), bf16 or float32 (logits_dtype, MTQ_DTYPE_*) at pitch ld_logits, to what the plan and the
 * combine above take: topk_ids int32 (tokens, topk) at pitch ld_ids and topk_weights float32 (tokens, topk) at pitch ld_w, in ONE
 * launch.  The router GEMM (x · W_routerᵀ) stays the model's.  The rule for one token, every operation rounded once to float32:
 *
 * Score.  s[e] = softmax(logits)[e] (MTQ_ROUTE_SOFTMAX) or sigmoid(logits[e]) (MTQ_ROUTE_SIGMOID) in float32; a bf16 logit is widened
 *   exactly.  How exp and the softmax denominator are formed is the kernel's business (the hardware exp2 of one product, the row
 *   maximum subtracted, a per-lane sum then a butterfly); s is the one float32 value that selection, the weights and `scores` use, and
 *   it does not depend on whether `scores` is given.  scores: NULL, or float32 (tokens, count) at pitch ld_scores: s, written only then.
 * Key.    key[e] = fl32(s[e] + bias[e]) with a bias (float32 [count], a selection-only correction: DeepSeek's
 *   e_score_correction_bias), else s[e].  a ranks before b iff key_a > key_b, or key_a == key_b and a < b, where a NaN key counts as
 *   -Inf: -0 and +0 tie, NaN ties with -Inf, and ties go to the lower id.
 * Groups  (n_group > 1).  Group g is the experts [g * count / n_group, (g + 1) * count / n_group).  Its score is its best key
 *   (group_top = 1, DeepSeek-V2) or fl32(best key + second-best key) (group_top = 2, DeepSeek-V3), the keys as the ranking sees them
 *   (NaN as -Inf).  The topk_group best groups stay, by the same ranking with the group index as id; the experts of the others are out.
 * Select. ids[j], j = 0 .. topk - 1: the topk best remaining experts in rank order; distinct and in [0, count) whatever the logits hold.
 * Weights. v[j] = s[ids[j]] (the score, not the key).  renormalize = 0: w[j] = fl32(v[j] * scale).  renormalize = 1: d = v[0];
 *   d = fl32(d + v[j]) for j = 1 .. topk - 1 in that order; d = fl32(d + eps); w[j] = fl32(fl32(v[j] / d) * scale), the division
 *   IEEE-correct.  eps and scale are rounded to float32 once, on the host.
 * Special values.  A -Inf logit scores +0: that is how a caller masks experts.  For a token with a NaN or +Inf logit, or with every
 *   logit -Inf, the ids stay distinct and in range and obey the ranking on whatever `scores` holds; its weights may be any words.  The
 *   other tokens of the call are unaffected.
 *
 * Limits: 1 <= count <= MTQ_MOE_MAX_EXPERTS, 1 <= topk <= min(count, MTQ_MOE_MAX_TOPK), 1 <= n_group <= MTQ_MOE_MAX_GROUPS,
 * count % n_group == 0, 1 <= topk_group <= n_group, topk <= topk_group * count / n_group, group_top 1 or 2 and at most count / n_group,
 * renormalize 0 or 1, eps and scale finite (as float32 too), tokens >= 1.  Outside them, and for a null pointer (bias and scores may
 * be NULL), a pitch below its row, a pointer not aligned to its type or a code that is none: MTQ_ERR_INVALID before a device is
 * looked for.  Asynchronous on `stream`; no workspace, no atomics, and two calls give the same words.  A token is one wave's work:
 * up to 256 experts the scores and keys stay in registers (one kernel each for count <= 64, <= 128, <= 256; four tokens a
 * workgroup), above that they live in LDS (one token a workgroup); the grid stops at 2048 workgroups and strides on.  The symbol is
 * optional: a build of this version may lack it. */
enum { MTQ_ROUTE_SOFTMAX = 0, MTQ_ROUTE_SIGMOID = 1 };
#define MTQ_MOE_MAX_GROUPS 64

int mtq_moe_route(const void *logits, int logits_dtype, int64_t ld_logits, int64_t tokens, int64_t count, int64_t topk, int score,
                  const float *bias, int64_t n_group, int64_t topk_group, int group_top, int renormalize, double eps, double scale,
                  int32_t *topk_ids, int64_t ld_ids, float *topk_weights, int64_t ld_w, float *scores, int64_t ld_scores, void *stream);

/* Test hook: the skinny kernel's decode (a cheaper form of the block kernel's for exponent bytes M..254, the same code elsewhere)
 * beside the reference decode, for fmt MTQ_FMT_BFP8 / BFP4 / BFP2.  got, want: device uint32 [16][256][16][16] = [rot][E][q][i], the
 * float32 word of code (16 q + (i + rot) % 16) mod 2^(M + 1) at element i of a group with exponent byte E: every (E, code) at every
 * position. */
int mtq_debug_packed_decode(int fmt, uint32_t *got, uint32_t *want, void *stream);

#ifdef __cplusplus
}
#endif
#include "mtq_moe_decode.h"
#include "mtq_glu_chunked.h"
#endif /* MTQ_H */
