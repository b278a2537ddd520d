// mtq_moe.hip — the glue of an MoE layer on packed experts: from a router's (tokens, top_k) expert ids to the row layout the grouped
// kernels of mtq_packed.hip take ("group e owns rows [group_rows[e], group_rows[e + 1])"), and from the experts' rows back to token
// order with the weighted sum.  include/mtq.h ("MoE routing") is the contract; DESIGN.md §A.6w the layout and the bytes.
//
//   moe_plan_one_kernel                       S = tokens * top_k <= 1024, every decode call: ONE workgroup of one wave makes the whole
//       plan - an LDS histogram of the expert ids (integer LDS adds: the only atomics of this file, and their result does not depend on
//       their order), its exclusive scan (group_rows), then the placement of the slots, 64 at a time in ascending order.
//   moe_plan_count_kernel, moe_plan_scan_kernel, moe_plan_place_kernel
//                                             the same stable counting sort above 1024 slots: a one-wave workgroup owns a run of 1024
//       consecutive slots.  count stores hist[run][expert] with plain stores, every entry; scan (one workgroup) turns each column of
//       hist into exclusive prefixes over the runs and writes group_rows; place starts each expert's counter at
//       group_rows[e] + hist[run][e] and walks its run as the one-launch kernel does.  Nothing in the workspace needs initialising.
//   moe_dispatch_kernel                       xs[r] = x[src[r] / top_k], a bit copy; a row whose src is no slot is all +0.
//   moe_combine_kernel                        y[t] = base[t] + sum over j, in that order, of w[t][j] * ys[row_of[t * top_k + j]], float32
//       product and sum rounded separately; a slot whose row is outside [0, S) is skipped.
//
// A lane's rank inside a 64-slot step is the LDS running counter of its expert plus the number of lower lanes with the same id; the
// mask of the lanes with its id comes from a loop that takes the lowest unmatched lane's id, ballots the equal ones and strikes them
// off.  The steps of a run follow each other inside one wave and the runs' counters start at the prefixes over the runs before them,
// so rows ascend with the slot inside every expert: the sort is stable, and two calls give the same words.
//
// No kernel waits on another workgroup and nothing is read back to the host.  Every index that comes from memory (an id, a src, a
// row_of) is checked against its range before it is used as one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kRun = MTQ_MOE_RUN;                   // slots a one-wave workgroup owns
constexpr int kWave = 64;
constexpr int kMaxCount = MTQ_MOE_MAX_EXPERTS;      // the LDS counters: 16 KiB
constexpr int kMaxTopk = MTQ_MOE_MAX_TOPK;
constexpr int kScanThreads = 256;
constexpr int kCopyThreads = 256;
constexpr int kMaxBlocks = 8192;    // the copy kernels' grids stop here and stride on

// float32 → bf16, round to nearest even; NaN stays NaN: mtq_packed.hip's f32_to_bf16, the rounding of every packed entry's bf16 output
__device__ __forceinline__ uint16_t f32_to_bf16(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + (0x7FFFu + ((u >> 16) & 1u))) >> 16);
}

__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// The expert of slot s as the router wrote it, in the ids' own width; the caller decides whether it is one.
template <bool ID64>
__device__ __forceinline__ int64_t slot_id(const void *__restrict__ ids, int64_t ld_ids, int K, int s)
{
    const int t = s / K;
    const int64_t at = (int64_t)t * ld_ids + (s - t * K);
    if constexpr (ID64) return static_cast<const int64_t *>(ids)[at];
    else return static_cast<const int32_t *>(ids)[at];
}

// cnt[e] += slots of [s0, s1) that name expert e, for the calling wave (the workgroup)
template <bool ID64>
__device__ __forceinline__ void count_run(const void *__restrict__ ids, int64_t ld_ids, int K, int count, int s0, int s1, int *cnt)
{
    for (int s = s0 + (int)threadIdx.x; s < s1; s += kWave) {
        const int64_t id = slot_id<ID64>(ids, ld_ids, K, s);
        if (id >= 0 && id < count) atomicAdd(&cnt[(int)id], 1);
    }
}

// Exclusive scan over the workgroup (WAVES waves) of one value per thread; *total: the sum over all threads.  part: LDS [WAVES].
template <int WAVES>
__device__ __forceinline__ int block_exclusive_scan(int v, int *part, int *total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += up;
    }
    if (lane == kWave - 1) part[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int p = part[w];
        if (w < wave) before += p;
        all += p;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// cnt[0 .. count) → its exclusive prefix sums in place, also stored as group_rows[0 .. count), and the total as group_rows[count];
// returns the total.  Every thread of the workgroup calls it; cnt is complete before and after (barriers inside).
template <int WAVES>
__device__ __forceinline__ int scan_counts(int *cnt, int count, int *part, int32_t *__restrict__ group_rows)
{
    const int threads = WAVES * kWave, per = (count + threads - 1) / threads;
    const int e0 = std::min((int)threadIdx.x * per, count), e1 = std::min(e0 + per, count);
    int sum = 0;
    for (int e = e0; e < e1; ++e) sum += cnt[e];
    int total;
    int run = block_exclusive_scan<WAVES>(sum, part, &total);
    for (int e = e0; e < e1; ++e) {
        const int v = cnt[e];
        cnt[e] = run;
        group_rows[e] = run;
        run += v;
    }
    if (threadIdx.x == 0) group_rows[count] = total;
    __syncthreads();
    return total;
}

// The slots [s0, s1) of one wave's run, 64 at a time in ascending order: cnt[e] is expert e's next row on entry and is moved on.
// Writes row_of[s] for every slot of the run and src[row] for every live one.
template <bool ID64>
__device__ __forceinline__ void place_run(const void *__restrict__ ids, int64_t ld_ids, int K, int count, int S, int s0, int s1, int *cnt,
                                          int32_t *__restrict__ row_of, int32_t *__restrict__ src)
{
    const int lane = threadIdx.x;
    for (int at = s0; at < s1; at += kWave) {
        const int s = at + lane;
        const bool valid = s < s1;
        const int64_t id = valid ? slot_id<ID64>(ids, ld_ids, K, s) : -1;
        const bool live = valid && id >= 0 && id < count;
        const int e = live ? (int)id : -1;
        uint64_t todo = __ballot(live), mine = 0;
        while (todo) {                               // wave-uniform: the lowest unmatched lane's id, the lanes that share it
            const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
            const int lid = __builtin_amdgcn_readlane(e, leader);
            const uint64_t same = __ballot(live && e == lid);
            if (live && e == lid) mine = same;
            todo &= ~same;
        }
        if (live) {
            const int row = cnt[e] + __popcll(mine & (((uint64_t)1 << lane) - 1));
            row_of[s] = row;
            if (row >= 0 && row < S) src[row] = s;
        } else if (valid) {
            row_of[s] = -1;
        }
        __syncthreads();                             // one wave: every lane has read its counter
        if (live && lane == 63 - __builtin_clzll(mine)) cnt[e] += __popcll(mine);
        __syncthreads();
    }
}

template <bool ID64>
__global__ __launch_bounds__(kWave) void moe_plan_one_kernel(const void *__restrict__ ids, int64_t ld_ids, int S, int K, int count,
                                                            int32_t *__restrict__ group_rows, int32_t *__restrict__ row_of,
                                                            int32_t *__restrict__ src)
{
    __shared__ int cnt[kMaxCount];
    __shared__ int part[1];
    for (int e = threadIdx.x; e < count; e += kWave) cnt[e] = 0;
    __syncthreads();
    count_run<ID64>(ids, ld_ids, K, count, 0, S, cnt);
    __syncthreads();
    const int R = scan_counts<1>(cnt, count, part, group_rows);
    place_run<ID64>(ids, ld_ids, K, count, S, 0, S, cnt, row_of, src);
    for (int r = std::max(R, 0) + (int)threadIdx.x; r < S; r += kWave) src[r] = -1;   // no placement writes a row at or past R
}

template <bool ID64>
__global__ __launch_bounds__(kWave) void moe_plan_count_kernel(const void *__restrict__ ids, int64_t ld_ids, int S, int K, int count,
                                                              int32_t *__restrict__ hist)
{
    __shared__ int cnt[kMaxCount];
    for (int e = threadIdx.x; e < count; e += kWave) cnt[e] = 0;
    __syncthreads();
    const int s0 = (int)blockIdx.x * kRun;
    count_run<ID64>(ids, ld_ids, K, count, s0, std::min(s0 + kRun, S), cnt);
    __syncthreads();
    int32_t *mine = hist + (size_t)blockIdx.x * count;
    for (int e = threadIdx.x; e < count; e += kWave) mine[e] = cnt[e];
}

// hist[run][e] → the slots of expert e in the runs before `run`; group_rows from the columns' totals.  One workgroup.
__global__ __launch_bounds__(kScanThreads) void moe_plan_scan_kernel(int32_t *hist, int runs, int count, int32_t *__restrict__ group_rows)
{
    __shared__ int tot[kMaxCount];
    __shared__ int part[kScanThreads / kWave];
    constexpr int kAhead = 8;                        // loads in flight per column: the sum is sequential, the loads need not be
    for (int e = threadIdx.x; e < count; e += kScanThreads) {
        int run = 0;
        for (int b0 = 0; b0 < runs; b0 += kAhead) {
            int v[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) v[u] = b0 + u < runs ? hist[(size_t)(b0 + u) * count + e] : 0;
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (b0 + u < runs) hist[(size_t)(b0 + u) * count + e] = run;
                run += v[u];
            }
        }
        tot[e] = run;
    }
    __syncthreads();
    scan_counts<kScanThreads / kWave>(tot, count, part, group_rows);
}

template <bool ID64>
__global__ __launch_bounds__(kWave) void moe_plan_place_kernel(const void *__restrict__ ids, int64_t ld_ids, int S, int K, int count,
                                                              const int32_t *__restrict__ hist, const int32_t *__restrict__ group_rows,
                                                              int32_t *__restrict__ row_of, int32_t *__restrict__ src)
{
    __shared__ int cnt[kMaxCount];
    const int32_t *mine = hist + (size_t)blockIdx.x * count;
    for (int e = threadIdx.x; e < count; e += kWave) cnt[e] = group_rows[e] + mine[e];
    __syncthreads();
    const int s0 = (int)blockIdx.x * kRun, s1 = std::min(s0 + kRun, S);
    place_run<ID64>(ids, ld_ids, K, count, S, s0, s1, cnt, row_of, src);
    const int R = group_rows[count];
    for (int r = std::max(std::max(R, 0), s0) + (int)threadIdx.x; r < s1; r += kWave) src[r] = -1;   // this run's share of [R, S)
}

// ---- dispatch: L lanes (a power of two, 1..256) share a row, 256 / L rows per workgroup; VEC: 16 bytes per lane and step
template <bool VEC>
__global__ __launch_bounds__(kCopyThreads) void moe_dispatch_kernel(const uint16_t *__restrict__ x, int64_t ldx, const int32_t *__restrict__ src,
                                                                   int S, int K, int k, uint16_t *__restrict__ xs, int64_t ldxs, int lanes_log2)
{
    const int L = 1 << lanes_log2, lane = threadIdx.x & (L - 1), sub = threadIdx.x >> lanes_log2, per_block = kCopyThreads >> lanes_log2;
    for (int64_t r = (int64_t)blockIdx.x * per_block + sub; r < S; r += (int64_t)gridDim.x * per_block) {
        const int v = src[r];
        const bool from = v >= 0 && v < S;           // v / K < tokens: no row of x at or past tokens is read
        const uint16_t *in = x + (int64_t)(from ? v / K : 0) * ldx;
        uint16_t *out = xs + r * ldxs;
        if constexpr (VEC) {
            for (int c = lane; c < k / 8; c += L)
                reinterpret_cast<uint4 *>(out)[c] = from ? reinterpret_cast<const uint4 *>(in)[c] : make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (int c = lane; c < k; c += L) out[c] = from ? in[c] : (uint16_t)0;
        }
    }
}

// ---- combine: a lane owns 8 consecutive columns of one token; L lanes (64..256) share the token, so its rows and weights are
// wave-uniform.  base_kind: 0 none, 1 bf16, 2 float32.
template <bool YS_BF16, bool VEC>
__device__ __forceinline__ void load8(const void *__restrict__ p, int64_t at, int cols, float (&v)[8])
{
    if constexpr (VEC) {
        if constexpr (YS_BF16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(p) + at);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = bf16_to_f32(w[i] & 0xFFFFu);
                v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
            }
        } else {
            const float4 a = *reinterpret_cast<const float4 *>(static_cast<const float *>(p) + at);
            const float4 b = *reinterpret_cast<const float4 *>(static_cast<const float *>(p) + at + 4);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < cols) {
                if constexpr (YS_BF16) v[i] = bf16_to_f32(static_cast<const uint16_t *>(p)[at + i]);
                else v[i] = static_cast<const float *>(p)[at + i];
            } else {
                v[i] = 0.0f;
            }
        }
    }
}

template <bool YS_BF16, bool OUT_BF16, bool VEC>
__global__ __launch_bounds__(kCopyThreads) void moe_combine_kernel(const void *__restrict__ ys, int64_t ldys, const int32_t *__restrict__ row_of,
                                                                  const float *__restrict__ weights, int64_t ldw, const void *__restrict__ base,
                                                                  int base_kind, int64_t ldbase, int T, int K, int n, void *__restrict__ y,
                                                                  int64_t ldy, int lanes_log2)
{
#pragma clang fp contract(off)
    constexpr int kBatch = 4;                        // rows of ys a lane has in flight
    const int L = 1 << lanes_log2, lane = threadIdx.x & (L - 1), per_block = kCopyThreads >> lanes_log2;
    const int sub = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> lanes_log2));      // L >= 64: one token per wave
    const int64_t S = (int64_t)T * K;
    for (int64_t t = (int64_t)blockIdx.x * per_block + sub; t < T; t += (int64_t)gridDim.x * per_block) {
        const int32_t *rows = row_of + t * K;
        const float *w = weights + t * ldw;
        for (int c0 = lane * 8; c0 < n; c0 += L * 8) {
            const int cols = std::min(8, n - c0);
            float acc[8];
            if (base_kind == 1) load8<true, VEC>(base, t * ldbase + c0, cols, acc);
            else if (base_kind == 2) load8<false, VEC>(base, t * ldbase + c0, cols, acc);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
            }
            for (int j0 = 0; j0 < K; j0 += kBatch) {
                float v[kBatch][8], wj[kBatch];
                bool use[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const int j = j0 + u;
                    const int r = j < K ? rows[j] : -1;
                    use[u] = r >= 0 && r < S;        // skipped, not multiplied by zero: an unused row's Inf cannot reach y
                    wj[u] = use[u] ? w[j] : 0.0f;
                    if (use[u]) load8<YS_BF16, VEC>(ys, (int64_t)r * ldys + c0, cols, v[u]);
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    if (use[u]) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(wj[u], v[u][i]));
                    }
                }
            }
            const int64_t at = t * ldy + c0;
            if constexpr (VEC) {
                if constexpr (OUT_BF16) {
                    uint32_t pk[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) pk[i] = (uint32_t)f32_to_bf16(acc[2 * i]) | ((uint32_t)f32_to_bf16(acc[2 * i + 1]) << 16);
                    *reinterpret_cast<uint4 *>(static_cast<uint16_t *>(y) + at) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                } else {
                    *reinterpret_cast<float4 *>(static_cast<float *>(y) + at) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    *reinterpret_cast<float4 *>(static_cast<float *>(y) + at + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (i < cols) {
                        if constexpr (OUT_BF16) static_cast<uint16_t *>(y)[at + i] = f32_to_bf16(acc[i]);
                        else static_cast<float *>(y)[at + i] = acc[i];
                    }
                }
            }
        }
    }
}

// ---- host side
inline size_t round16(size_t v) { return (v + 15) / 16 * 16; }

// tokens, topk, count within the limits and S = tokens * topk below 2^31, or MTQ_ERR_INVALID with the reason
int moe_shape(int64_t tokens, int64_t topk, int64_t count)
{
    if (tokens <= 0) return fail(MTQ_ERR_INVALID, "tokens must be positive");
    if (topk <= 0 || topk > kMaxTopk) return fail(MTQ_ERR_INVALID, "topk must be 1 .. MTQ_MOE_MAX_TOPK (64)");
    if (count <= 0 || count > kMaxCount) return fail(MTQ_ERR_INVALID, "count must be 1 .. MTQ_MOE_MAX_EXPERTS (4096)");
    if (tokens > (((int64_t)1 << 31) - 1) / topk) return fail(MTQ_ERR_INVALID, "tokens * topk must be below 2^31");
    return MTQ_OK;
}

bool aligned(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

int dtype_ok(int dtype, const char *msg)
{
    if (dtype != MTQ_DTYPE_BF16 && dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, msg);
    return MTQ_OK;
}

// L of the copy kernels: the power of two at or above `chunks`, within [least, 256]
int lanes_log2_of(int64_t chunks, int least_log2)
{
    int lg = least_log2;
    while (lg < 8 && ((int64_t)1 << lg) < chunks) ++lg;
    return lg;
}

unsigned copy_grid(int64_t rows, int lanes_log2)
{
    const int64_t per_block = kCopyThreads >> lanes_log2;
    return (unsigned)std::min<int64_t>((rows + per_block - 1) / per_block, kMaxBlocks);
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_moe_plan_workspace_bytes(int64_t tokens, int64_t topk, int64_t count)
{
    if (moe_shape(tokens, topk, count)) return (size_t)-1;
    const int64_t runs = (tokens * topk + kRun - 1) / kRun;
    return round16((size_t)runs * (size_t)count * sizeof(int32_t));
}

extern "C" int mtq_moe_plan(const void *topk_ids, int id_dtype, int64_t ld_ids, int64_t tokens, int64_t topk, int64_t count, int32_t *group_rows,
                            int32_t *row_of, int32_t *src, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!topk_ids || !group_rows || !row_of || !src) return fail(MTQ_ERR_INVALID, "null argument");
    if (id_dtype != MTQ_IDS_I32 && id_dtype != MTQ_IDS_I64) return fail(MTQ_ERR_INVALID, "id_dtype must be MTQ_IDS_I32 or MTQ_IDS_I64");
    if (int rc = moe_shape(tokens, topk, count)) return rc;
    if (ld_ids < topk) return fail(MTQ_ERR_INVALID, "ld_ids < topk");
    if (ld_ids > (int64_t)1 << 40) return fail(MTQ_ERR_INVALID, "ld_ids too large");
    if (!aligned(topk_ids, id_dtype == MTQ_IDS_I64 ? 8 : 4)) return fail(MTQ_ERR_INVALID, "topk_ids is not aligned to its type");
    if (!aligned(group_rows, 4) || !aligned(row_of, 4) || !aligned(src, 4)) return fail(MTQ_ERR_INVALID, "group_rows, row_of and src must be 4-byte aligned");
    const size_t need = mtq_moe_plan_workspace_bytes(tokens, topk, count);
    if (!workspace) return fail(MTQ_ERR_INVALID, "workspace is null (the plan takes one at every size)");
    if (!aligned(workspace, 16)) return fail(MTQ_ERR_INVALID, "workspace must be 16-byte aligned");
    if (workspace_bytes < need)
        return failf(MTQ_ERR_INVALID, "workspace_bytes %zu is smaller than the %zu bytes this call needs", workspace_bytes, need);
    if (int rc = require_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = (int)(tokens * topk), K = (int)topk, E = (int)count;
    const bool id64 = id_dtype == MTQ_IDS_I64;
    if (S <= kRun) {
        if (id64) hipLaunchKernelGGL(moe_plan_one_kernel<true>, dim3(1), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, group_rows, row_of, src);
        else hipLaunchKernelGGL(moe_plan_one_kernel<false>, dim3(1), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, group_rows, row_of, src);
        return check_launch("mtq_moe_plan");
    }
    const int runs = (S + kRun - 1) / kRun;
    int32_t *hist = static_cast<int32_t *>(workspace);
    if (id64) hipLaunchKernelGGL(moe_plan_count_kernel<true>, dim3(runs), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, hist);
    else hipLaunchKernelGGL(moe_plan_count_kernel<false>, dim3(runs), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, hist);
    if (int rc = check_launch("mtq_moe_plan (count)")) return rc;
    hipLaunchKernelGGL(moe_plan_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, hist, runs, E, group_rows);
    if (int rc = check_launch("mtq_moe_plan (scan)")) return rc;
    if (id64) hipLaunchKernelGGL(moe_plan_place_kernel<true>, dim3(runs), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, hist, group_rows, row_of, src);
    else hipLaunchKernelGGL(moe_plan_place_kernel<false>, dim3(runs), dim3(kWave), 0, st, topk_ids, ld_ids, S, K, E, hist, group_rows, row_of, src);
    return check_launch("mtq_moe_plan (place)");
}

extern "C" int mtq_moe_dispatch(const void *x, int64_t tokens, int64_t k, int64_t ldx, const int32_t *src, int64_t topk, void *xs, int64_t ldxs,
                                void *stream)
{
    if (!x || !src || !xs) return fail(MTQ_ERR_INVALID, "null argument");
    if (int rc = moe_shape(tokens, topk, 1)) return rc;
    if (k <= 0) return fail(MTQ_ERR_INVALID, "k must be positive");
    if (k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldxs < k) return fail(MTQ_ERR_INVALID, "ldxs < k");
    if (ldx > (int64_t)1 << 40 || ldxs > (int64_t)1 << 31) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (!aligned(x, 2) || !aligned(xs, 2) || !aligned(src, 4)) return fail(MTQ_ERR_INVALID, "x, xs or src is not aligned to its type");
    if (int rc = require_device()) return rc;
    const int64_t S = tokens * topk;
    const bool vec = aligned(x, 16) && aligned(xs, 16) && ldx % 8 == 0 && ldxs % 8 == 0 && k % 8 == 0;
    const int lg = lanes_log2_of(vec ? k / 8 : k, 0);
    const dim3 grid(copy_grid(S, lg));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(moe_dispatch_kernel<true>, grid, dim3(kCopyThreads), 0, st, static_cast<const uint16_t *>(x), ldx, src, (int)S,
                                (int)topk, (int)k, static_cast<uint16_t *>(xs), ldxs, lg);
    else hipLaunchKernelGGL(moe_dispatch_kernel<false>, grid, dim3(kCopyThreads), 0, st, static_cast<const uint16_t *>(x), ldx, src, (int)S,
                            (int)topk, (int)k, static_cast<uint16_t *>(xs), ldxs, lg);
    return check_launch("mtq_moe_dispatch");
}

extern "C" int mtq_moe_combine(const void *ys, int ys_dtype, int64_t ldys, const int32_t *row_of, const float *weights, int64_t ldw,
                               const void *base, int base_dtype, int64_t ldbase, int64_t tokens, int64_t topk, int64_t n, void *y, int out_dtype,
                               int64_t ldy, void *stream)
{
    if (!ys || !row_of || !weights || !y) return fail(MTQ_ERR_INVALID, "null argument");
    if (int rc = dtype_ok(ys_dtype, "ys_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32")) return rc;
    if (int rc = dtype_ok(out_dtype, "out_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32")) return rc;
    if (base)
        if (int rc = dtype_ok(base_dtype, "base_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32")) return rc;
    if (int rc = moe_shape(tokens, topk, 1)) return rc;
    if (n <= 0) return fail(MTQ_ERR_INVALID, "n must be positive");
    if (n > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (ldys < n) return fail(MTQ_ERR_INVALID, "ldys < n");
    if (ldw < topk) return fail(MTQ_ERR_INVALID, "ldw < topk");
    if (base && ldbase < n) return fail(MTQ_ERR_INVALID, "ldbase < n");
    if (ldy < n) return fail(MTQ_ERR_INVALID, "ldy < n");
    if (ldys > (int64_t)1 << 31 || ldw > (int64_t)1 << 31 || ldy > (int64_t)1 << 31 || (base && ldbase > (int64_t)1 << 31))
        return fail(MTQ_ERR_INVALID, "matrix too large");
    const size_t ys_el = ys_dtype == MTQ_DTYPE_BF16 ? 2 : 4, y_el = out_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    const size_t base_el = base_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    if (!aligned(ys, ys_el) || !aligned(y, y_el) || !aligned(row_of, 4) || !aligned(weights, 4) || (base && !aligned(base, base_el)))
        return fail(MTQ_ERR_INVALID, "an operand is not aligned to its type");
    if (int rc = require_device()) return rc;
    // 16-byte accesses of a lane's 8 columns: every operand's rows start 16-byte aligned
    const bool vec = n % 8 == 0 && aligned(ys, 16) && (ldys * ys_el) % 16 == 0 && aligned(y, 16) && (ldy * y_el) % 16 == 0 &&
                     (!base || (aligned(base, 16) && (ldbase * base_el) % 16 == 0));
    const int lg = lanes_log2_of((n + 7) / 8, 6);
    const dim3 grid(copy_grid(tokens, lg)), block(kCopyThreads);
    const int base_kind = !base ? 0 : (base_dtype == MTQ_DTYPE_BF16 ? 1 : 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MTQ_MOE_COMBINE(YSB, OUTB, VEC)                                                                                                    \
    hipLaunchKernelGGL((moe_combine_kernel<YSB, OUTB, VEC>), grid, block, 0, st, ys, ldys, row_of, weights, ldw, base, base_kind, ldbase, \
                       (int)tokens, (int)topk, (int)n, y, ldy, lg)
    const bool ysb = ys_dtype == MTQ_DTYPE_BF16, outb = out_dtype == MTQ_DTYPE_BF16;
    if (vec) {
        if (ysb && outb) MTQ_MOE_COMBINE(true, true, true);
        else if (ysb) MTQ_MOE_COMBINE(true, false, true);
        else if (outb) MTQ_MOE_COMBINE(false, true, true);
        else MTQ_MOE_COMBINE(false, false, true);
    } else {
        if (ysb && outb) MTQ_MOE_COMBINE(true, true, false);
        else if (ysb) MTQ_MOE_COMBINE(true, false, false);
        else if (outb) MTQ_MOE_COMBINE(false, true, false);
        else MTQ_MOE_COMBINE(false, false, false);
    }
#undef MTQ_MOE_COMBINE
    return check_launch("mtq_moe_combine");
}
