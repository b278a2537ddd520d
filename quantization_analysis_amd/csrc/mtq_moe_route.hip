// mtq_moe_route.hip — the router of an MoE layer in one launch: from the router's logits (tokens, count) to (topk_ids, topk_weights),
// what mtq_moe_plan and mtq_moe_combine take.  include/mtq.h ("MoE router") is the contract: the score, the key, the ranking, the
// groups and the weight arithmetic are stated there operation by operation; DESIGN.md §A.6z the layout and the measurements.
//
//   moe_route_kernel<PER, BF16>   a token is one wave's work; lane l owns experts l, l + 64, ... (coalesced loads).
//       PER = 1, 2, 4   count <= 64 * PER: scores and keys live in registers, four tokens (waves) a workgroup.
//       PER = 0         count > 256: scores and keys live in the workgroup's LDS (32 KiB), one token (wave) a workgroup.
//
// A key is carried as one 64-bit word, (orderable key word << 32) | ~id: the larger word ranks first, so a tie of keys goes to the
// lower id.  The orderable word of a float maps NaN to -Inf and -0 to +0 first; an expert that is out (past count, in a group that
// was not kept, or already selected) is the word 0, below every expert that is in.  Top-k is K rounds of a wave arg-max of those
// words (a butterfly of 64-bit shuffles: every lane ends with the same word); lane j keeps round j's winner, so the K results sit in
// lanes 0 .. K - 1 in rank order.
//
// Groups.  The orderable words go through LDS; group g is reduced by 64 / P lanes (P the power of two at or above n_group), each
// taking a strided share of the group's words and keeping the two largest, then a butterfly inside the group's lanes.  A group's
// rank is the number of groups whose (score word, ~g) is larger; the kept groups are a ballot.
//
// The grid is capped (kRouteMaxBlocks) and strides on.  The token loop is uniform over the workgroup, so the barriers around the
// LDS words are reached by every wave.  No atomics, no workspace; two calls give the same words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kWave = 64;
constexpr int kRouteMaxCount = MTQ_MOE_MAX_EXPERTS;
constexpr int kRouteRegWaves = 4;       // tokens a workgroup of the register kernels holds
constexpr int kRouteRegMaxCount = 256;  // above it: the LDS kernel
constexpr int kRouteMaxBlocks = 2048;   // the grid stops here and strides on
constexpr float kLog2e = 1.4426950408889634f;

struct RouteArgs {
    const void *logits;
    const float *bias;
    int32_t *ids;
    float *weights;
    float *scores;
    int64_t ld_logits, ld_ids, ld_w, ld_scores;
    int T, count, K;
    int score, renormalize;
    int n_group, topk_group, group_top;
    int gs;            // count / n_group
    int per_log2;      // log2 of the lanes that share a group: 64 / P
    int q64, r64;      // 64 / gs, 64 % gs: a lane's group from one slot to the next
    float eps, scale;
};

// float → a word whose unsigned order is the ranking's: NaN counts as -Inf, -0 as +0.  Never 0: -Inf is 0x007FFFFF.
__device__ __forceinline__ uint32_t ord_of(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0xFF800000u;
    if ((u << 1) == 0u) u = 0u;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float float_of_ord(uint32_t o) { return __uint_as_float((o >> 31) ? (o ^ 0x80000000u) : ~o); }

__device__ __forceinline__ uint64_t pack_key(uint32_t ord, uint32_t id) { return ((uint64_t)ord << 32) | (uint32_t)~id; }

__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float wave_max32(float v)
{
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, kWave));
    return v;
}

// every lane gets the same word: both lanes of a pair add the same two terms
__device__ __forceinline__ float wave_sum32(float v)
{
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kWave);
    return v;
}

template <bool BF16>
__device__ __forceinline__ float load_logit(const void *__restrict__ p, int64_t at)
{
    if constexpr (BF16) return __uint_as_float((uint32_t) static_cast<const uint16_t *>(p)[at] << 16);
    else return static_cast<const float *>(p)[at];
}

__device__ __forceinline__ float sigmoid_of(float x) { return 1.0f / (1.0f + __builtin_amdgcn_exp2f(-x * kLog2e)); }

// The kept groups of one token from its orderable words keys[0 .. count), complete in LDS: bit (g << per_log2) of the result is set
// iff group g is among the topk_group best.  Called by every lane of the wave.
__device__ __forceinline__ uint64_t kept_groups(const uint32_t *keys, const RouteArgs &a, int lane)
{
    const int per = 1 << a.per_log2, g = lane >> a.per_log2, r = lane & (per - 1);
    uint32_t a1 = 0, a2 = 0;                       // the two largest words of this lane's share (0: none)
    if (g < a.n_group) {
        const uint32_t *mine = keys + g * a.gs;
        for (int j = r; j < a.gs; j += per) {
            const uint32_t u = mine[j];
            if (u > a1) a2 = a1, a1 = u;
            else if (u > a2) a2 = u;
        }
    }
    for (int d = 1; d < per; d <<= 1) {            // wave-uniform trip count; partners stay inside the group's lanes
        const uint32_t b1 = __shfl_xor(a1, d, kWave), b2 = __shfl_xor(a2, d, kWave);
        const uint32_t lo = a1 < b1 ? a1 : b1, hi2 = a2 > b2 ? a2 : b2;
        a1 = a1 > b1 ? a1 : b1;
        a2 = lo > hi2 ? lo : hi2;
    }
    uint64_t gp = 0;
    if (g < a.n_group && r == 0) {
        const float best = float_of_ord(a1);
        const float sc = a.group_top == 2 ? best + float_of_ord(a2) : best;
        gp = pack_key(ord_of(sc), (uint32_t)g);
    }
    int above = 0;
    for (int g2 = 0; g2 < a.n_group; ++g2) {
        const int from = g2 << a.per_log2;         // wave-uniform
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gp, from);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(gp >> 32), from);
        above += (((uint64_t)hi << 32) | lo) > gp;
    }
    return __ballot(gp != 0 && above < a.topk_group);
}

// lanes 0 .. K - 1 hold the selected ids and their scores v → the weights, by the contract's sequence
__device__ __forceinline__ float weight_of(float v, const RouteArgs &a)
{
#pragma clang fp contract(off)
    if (!a.renormalize) return v * a.scale;
    float d = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), 0));
    for (int j = 1; j < a.K; ++j) d = d + __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
    d = d + a.eps;
    const float q = v / d;
    return q * a.scale;
}

template <int PER, bool BF16>
__global__ __launch_bounds__(PER ? kRouteRegWaves *kWave : kWave) void moe_route_kernel(const RouteArgs a)
{
#pragma clang fp contract(off)
    constexpr int kWaves = PER ? kRouteRegWaves : 1;
    constexpr int kKeys = PER ? PER * kWave : kRouteMaxCount;
    __shared__ uint32_t key_words[kWaves][kKeys];
    __shared__ float score_words[PER ? 1 : kRouteMaxCount];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t *keys = key_words[wave];
    const int count = a.count, K = a.K;
    const bool grouped = a.n_group > 1;
    const int lane_g = lane / a.gs, lane_rem = lane - lane_g * a.gs;

    for (int64_t t0 = (int64_t)blockIdx.x * kWaves; t0 < a.T; t0 += (int64_t)gridDim.x * kWaves) {   // uniform over the workgroup
        const bool active = t0 + wave < a.T;
        const int64_t t = active ? t0 + wave : a.T - 1;     // an idle wave of the last pass redoes the last token and stores nothing
        const int64_t row = t * a.ld_logits;
        uint64_t mine = 0;                                   // lane j: the winner of round j
        float v = 0.0f;                                      // lane j: its score

        if constexpr (PER > 0) {
            float s[PER];
            uint64_t packed[PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int e = lane + i * kWave;
                s[i] = e < count ? load_logit<BF16>(a.logits, row + e) : -INFINITY;
            }
            if (a.score == MTQ_ROUTE_SIGMOID) {
#pragma unroll
                for (int i = 0; i < PER; ++i) s[i] = sigmoid_of(s[i]);
            } else {
                float m = s[0];
#pragma unroll
                for (int i = 1; i < PER; ++i) m = fmaxf(m, s[i]);
                m = wave_max32(m);
                float sum = 0.0f;
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    s[i] = __builtin_amdgcn_exp2f((s[i] - m) * kLog2e);
                    if (lane + i * kWave < count) sum = sum + s[i];
                }
                sum = wave_sum32(sum);
#pragma unroll
                for (int i = 0; i < PER; ++i) s[i] = s[i] / sum;
            }
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int e = lane + i * kWave;
                packed[i] = 0;
                if (e < count) {
                    const float key = a.bias ? s[i] + a.bias[e] : s[i];
                    packed[i] = pack_key(ord_of(key), (uint32_t)e);
                    if (a.scores && active) a.scores[t * a.ld_scores + e] = s[i];
                }
            }
            if (grouped) {
                __syncthreads();                             // the last token's words have been read
#pragma unroll
                for (int i = 0; i < PER; ++i)
                    if (lane + i * kWave < count) keys[lane + i * kWave] = (uint32_t)(packed[i] >> 32);
                __syncthreads();
                const uint64_t kept = kept_groups(keys, a, lane);
                int g = lane_g, rem = lane_rem;
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (!((kept >> ((g << a.per_log2) & 63)) & 1)) packed[i] = 0;
                    g += a.q64, rem += a.r64;
                    if (rem >= a.gs) rem -= a.gs, ++g;
                }
            }
            for (int j = 0; j < K; ++j) {
                uint64_t local = packed[0];
#pragma unroll
                for (int i = 1; i < PER; ++i) local = packed[i] > local ? packed[i] : local;
                const uint64_t best = wave_max64(local);
                if (lane == j) mine = best;
#pragma unroll
                for (int i = 0; i < PER; ++i)
                    if (packed[i] == best) packed[i] = 0;
            }
            const uint32_t id = ~(uint32_t)mine;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const float from = __shfl(s[i], (int)(id & (kWave - 1)), kWave);
                if ((int)(id >> 6) == i) v = from;
            }
        } else {
            float *sc = score_words;
            __syncthreads();                                 // the last token's words have been read
            if (a.score == MTQ_ROUTE_SIGMOID) {
                for (int e = lane; e < count; e += kWave) sc[e] = sigmoid_of(load_logit<BF16>(a.logits, row + e));
            } else {
                float m = -INFINITY;
                for (int e = lane; e < count; e += kWave) m = fmaxf(m, load_logit<BF16>(a.logits, row + e));
                m = wave_max32(m);
                float sum = 0.0f;
                for (int e = lane; e < count; e += kWave) {
                    const float p = __builtin_amdgcn_exp2f((load_logit<BF16>(a.logits, row + e) - m) * kLog2e);
                    sc[e] = p;
                    sum = sum + p;
                }
                sum = wave_sum32(sum);
                for (int e = lane; e < count; e += kWave) sc[e] = sc[e] / sum;      // a lane reads back its own words
            }
            for (int e = lane; e < count; e += kWave) {
                const float s = sc[e];
                keys[e] = ord_of(a.bias ? s + a.bias[e] : s);
                if (a.scores && active) a.scores[t * a.ld_scores + e] = s;
            }
            __syncthreads();
            if (grouped) {
                const uint64_t kept = kept_groups(keys, a, lane);
                __syncthreads();                             // every lane has read the groups' words
                int g = lane_g, rem = lane_rem;
                for (int e = lane; e < count; e += kWave) {
                    if (!((kept >> ((g << a.per_log2) & 63)) & 1)) keys[e] = 0;
                    g += a.q64, rem += a.r64;
                    if (rem >= a.gs) rem -= a.gs, ++g;
                }
            }
            for (int j = 0; j < K; ++j) {                    // a lane reads and strikes off its own words only
                uint64_t local = 0;
                for (int e = lane; e < count; e += kWave) {
                    const uint32_t u = keys[e];
                    const uint64_t p = u ? pack_key(u, (uint32_t)e) : 0;
                    local = p > local ? p : local;
                }
                const uint64_t best = wave_max64(local);
                if (lane == j) mine = best;
                const uint32_t won = ~(uint32_t)best;
                if (won < (uint32_t)count && (int)(won & (kWave - 1)) == lane) keys[won] = 0;
            }
            const uint32_t id = ~(uint32_t)mine;
            if (lane < K && id < (uint32_t)count) v = sc[id];
        }

        const float w = weight_of(v, a);
        if (active && lane < K) {
            a.ids[t * a.ld_ids + lane] = (int32_t)~(uint32_t)mine;
            a.weights[t * a.ld_w + lane] = w;
        }
    }
}

bool route_aligned(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" int mtq_moe_route(const void *logits, int logits_dtype, int64_t ld_logits, int64_t tokens, int64_t count, int64_t topk, int score,
                             const float *bias, int64_t n_group, int64_t topk_group, int group_top, int renormalize, double eps, double scale,
                             int32_t *topk_ids, int64_t ld_ids, float *topk_weights, int64_t ld_w, float *scores, int64_t ld_scores,
                             void *stream)
{
    if (!logits || !topk_ids || !topk_weights) return fail(MTQ_ERR_INVALID, "null argument");
    if (logits_dtype != MTQ_DTYPE_BF16 && logits_dtype != MTQ_DTYPE_F32)
        return fail(MTQ_ERR_INVALID, "logits_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (score != MTQ_ROUTE_SOFTMAX && score != MTQ_ROUTE_SIGMOID) return fail(MTQ_ERR_INVALID, "score must be MTQ_ROUTE_SOFTMAX or MTQ_ROUTE_SIGMOID");
    if (renormalize != 0 && renormalize != 1) return fail(MTQ_ERR_INVALID, "renormalize must be 0 or 1");
    if (tokens <= 0) return fail(MTQ_ERR_INVALID, "tokens must be positive");
    if (tokens > ((int64_t)1 << 31) - 1) return fail(MTQ_ERR_INVALID, "tokens must be below 2^31");
    if (count <= 0 || count > kRouteMaxCount) return fail(MTQ_ERR_INVALID, "count must be 1 .. MTQ_MOE_MAX_EXPERTS (4096)");
    if (topk <= 0 || topk > MTQ_MOE_MAX_TOPK || topk > count) return fail(MTQ_ERR_INVALID, "topk must be 1 .. min(count, MTQ_MOE_MAX_TOPK (64))");
    if (n_group <= 0 || n_group > MTQ_MOE_MAX_GROUPS) return fail(MTQ_ERR_INVALID, "n_group must be 1 .. MTQ_MOE_MAX_GROUPS (64)");
    if (count % n_group != 0) return fail(MTQ_ERR_INVALID, "count must be a multiple of n_group");
    if (topk_group <= 0 || topk_group > n_group) return fail(MTQ_ERR_INVALID, "topk_group must be 1 .. n_group");
    const int64_t gs = count / n_group;
    if (topk > topk_group * gs) return fail(MTQ_ERR_INVALID, "topk must be at most topk_group * count / n_group");
    if (group_top != 1 && group_top != 2) return fail(MTQ_ERR_INVALID, "group_top must be 1 or 2");
    if (group_top > gs) return fail(MTQ_ERR_INVALID, "group_top must be at most count / n_group");
    if (!std::isfinite(eps) || !std::isfinite(scale)) return fail(MTQ_ERR_INVALID, "eps and scale must be finite");
    const float eps32 = (float)eps, scale32 = (float)scale;
    if (!std::isfinite(eps32) || !std::isfinite(scale32)) return fail(MTQ_ERR_INVALID, "eps and scale must be finite in float32");
    if (ld_logits < count) return fail(MTQ_ERR_INVALID, "ld_logits < count");
    if (ld_ids < topk) return fail(MTQ_ERR_INVALID, "ld_ids < topk");
    if (ld_w < topk) return fail(MTQ_ERR_INVALID, "ld_w < topk");
    if (scores && ld_scores < count) return fail(MTQ_ERR_INVALID, "ld_scores < count");
    if (ld_logits > (int64_t)1 << 31 || ld_ids > (int64_t)1 << 31 || ld_w > (int64_t)1 << 31 || (scores && ld_scores > (int64_t)1 << 31))
        return fail(MTQ_ERR_INVALID, "matrix too large");
    if (!route_aligned(logits, logits_dtype == MTQ_DTYPE_BF16 ? 2 : 4) || !route_aligned(topk_ids, 4) || !route_aligned(topk_weights, 4) ||
        (bias && !route_aligned(bias, 4)) || (scores && !route_aligned(scores, 4)))
        return fail(MTQ_ERR_INVALID, "an operand is not aligned to its type");
    if (int rc = require_device()) return rc;

    RouteArgs a{};
    a.logits = logits, a.bias = bias, a.ids = topk_ids, a.weights = topk_weights, a.scores = scores;
    a.ld_logits = ld_logits, a.ld_ids = ld_ids, a.ld_w = ld_w, a.ld_scores = scores ? ld_scores : 0;
    a.T = (int)tokens, a.count = (int)count, a.K = (int)topk;
    a.score = score, a.renormalize = renormalize;
    a.n_group = (int)n_group, a.topk_group = (int)topk_group, a.group_top = group_top;
    a.gs = (int)gs;
    int p_log2 = 0;
    while ((1 << p_log2) < n_group) ++p_log2;
    a.per_log2 = 6 - p_log2;
    a.q64 = kWave / a.gs, a.r64 = kWave % a.gs;
    a.eps = eps32, a.scale = scale32;

    const bool bf16 = logits_dtype == MTQ_DTYPE_BF16;
    const int per = count <= 64 ? 1 : count <= 128 ? 2 : count <= kRouteRegMaxCount ? 4 : 0;
    const int64_t waves = per ? kRouteRegWaves : 1;
    const dim3 grid((unsigned)std::min<int64_t>((tokens + waves - 1) / waves, kRouteMaxBlocks)), block((unsigned)(waves * kWave));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MTQ_MOE_ROUTE(PER)                                                                              \
    do {                                                                                                \
        if (bf16) hipLaunchKernelGGL((moe_route_kernel<PER, true>), grid, block, 0, st, a);            \
        else hipLaunchKernelGGL((moe_route_kernel<PER, false>), grid, block, 0, st, a);                \
    } while (0)
    if (per == 1) MTQ_MOE_ROUTE(1);
    else if (per == 2) MTQ_MOE_ROUTE(2);
    else if (per == 4) MTQ_MOE_ROUTE(4);
    else MTQ_MOE_ROUTE(0);
#undef MTQ_MOE_ROUTE
    return check_launch("mtq_moe_route");
}
