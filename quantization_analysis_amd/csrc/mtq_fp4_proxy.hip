// mtq_fp4_proxy.hip — the reference's scalar MXFP4 / NVFP4 proxies (quantization_formats.py:174-183,257-278) on gfx950:
// y = sign(x) · g(|x|), one element at a time, g as quantization_formats.py (this package) restates it.  Two entry points:
//   mtq_fp4_proxy_sums     — one read of a batch of matrices → per matrix and proxy the seven float64 sums of
//                            mtq_columns_from_sums; y is never written.  Two launches: per-block partials, then one wave per
//                            matrix adds them in a fixed tree (no float atomics: the same input gives the same bits).
//   fp4_proxy_quantize     — y as float32, behind mtq_quantize's MTQ_FMT_MXFP4 / MTQ_FMT_NVFP4.
// The arithmetic is IEEE float32 with subnormals kept and correctly rounded division (hipcc's defaults; the Makefile adds
// -ffp-contract=off).  gfx950's scaled fp4 / fp8 conversions are not used: they round to nearest-even with OCP saturation, the
// reference picks the lower level on a tie and has its own e4m3 (largest value 240).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mtq.h"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kProxyThreads = 256;
constexpr int64_t kProxyElemsPerBlock = 32768;   // elements of one matrix per block of the sums launch
constexpr int kProxyAcc = 12;                    // Σx, Σx², then Σy, Σy², Σxy, Σ|x−y|, max|x−y| per proxy

__device__ __forceinline__ double nan_max(double m, double d) { return (d > m || d != d) ? d : m; }

// floor(2^j · ln 2) for j = -2..7: how many mantissa steps (2^-23 relative) next to a power of two 2^K have a float32 log2 that
// rounds to the integer K (the float32 half-ulp of K there is 2^(j-24) with j as the callers pick it).
__device__ __forceinline__ uint32_t log2_edge(int j) { return (uint32_t)ldexpf(0.6931472f, j); }

__device__ __forceinline__ int ilog2_abs(int k) { return 31 - __clz(k < 0 ? -k : k); }
__device__ __forceinline__ bool pow2_abs(int k) { const int a = k < 0 ? -k : k; return (a & (a - 1)) == 0; }

// s = 2^k · (1 + mn · 2^-23) for finite float32 s > 0 (subnormals normalised).
__device__ __forceinline__ void split_pos(float s, int &k, uint32_t &mn)
{
    const uint32_t u = __float_as_uint(s), eb = u >> 23, man = u & 0x7FFFFFu;
    if (eb == 0u) {
        const int p = 31 - __clz(man);
        k = p - 149;
        mn = (man ^ (1u << p)) << (23 - p);
    } else {
        k = (int)eb - 127;
        mn = man;
    }
}

// floor(np.float32 log2(s)): k, or k + 1 for the last mantissas below 2^(k+1) whose log2 rounds up to it.
__device__ __forceinline__ int log2_floor(int k, uint32_t mn)
{
    const int K = k + 1;
    if (K == 0) return k;
    const int j = ilog2_abs(K) - ((K > 0 && pow2_abs(K)) ? 1 : 0);   // approached from below: K > 0 meets the finer spacing under it
    return (0x800000u - mn) <= log2_edge(j) ? K : k;
}

// ceil(np.float32 log2(s)): k for a power of two and for the first mantissas above 2^k whose log2 rounds down to k, else k + 1.
__device__ __forceinline__ int log2_ceil(int k, uint32_t mn)
{
    if (mn == 0u) return k;
    if (k == 0) return 1;
    const int j = ilog2_abs(k) - ((k < 0 && pow2_abs(k)) ? 1 : 0);   // moving away from k: k < 0 meets the finer spacing under |k|
    return mn <= log2_edge(j - 1) ? k : k + 1;
}

// quantize_fp4_e2m1 (reference :21-26,197-202) for v >= 0 or NaN: sign(v) · the level of least float32 |v − level|, the lower on a
// tie.  Below 2^22 every difference that decides is exact, so the level is the count of midpoints under v; above it (and for NaN,
// Inf) the eight differences are formed as the reference forms them.
__device__ __noinline__ float fp4_level_literal(float v)
{
    const float lv[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
    float best = fabsf(v), l = 0.0f;
    for (int i = 1; i < 8; ++i) {
        const float d = fabsf(v - lv[i]);
        if (d < best) { best = d; l = lv[i]; }
    }
    const float sg = v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : (v == 0.0f ? 0.0f : v));
    return sg * l;
}

__device__ __forceinline__ float fp4_level(float v)
{
    if (!(v < 4194304.0f)) return fp4_level_literal(v);
    float l = v > 0.25f ? 0.5f : 0.0f;
    l = v > 0.75f ? 1.0f : l;
    l = v > 1.25f ? 1.5f : l;
    l = v > 1.75f ? 2.0f : l;
    l = v > 2.5f ? 3.0f : l;
    l = v > 3.5f ? 4.0f : l;
    l = v > 5.0f ? 6.0f : l;
    return l;
}

// simulate_mxfp4_amax (:257-266): a = |x|, s = a / 6 in float32 (equal to the reference's float32(a / 6.0 in double): a / 6 has the
// repeating binary expansion of a third, which never lies next to a float32 rounding midpoint), s_q = 2^ceil(log2 s), 0 for s = 0.
__device__ __forceinline__ float mxfp4_g(float a, float s)
{
    if (s == 0.0f) return 0.0f;                               // a = 0 (:260), or s underflows: a / 0 = Inf picks level 0
    if (!(s < INFINITY)) return __uint_as_float(0x7FC00000u); // NaN or Inf: 0 · Inf or NaN
    int k;
    uint32_t mn;
    split_pos(s, k, mn);
    const int c = log2_ceil(k, mn);                           // -149 <= c <= 126
    const float sq = c >= -126 ? __uint_as_float((uint32_t)(c + 127) << 23) : __uint_as_float(1u << (c + 149));
    return fp4_level(ldexpf(a, -c)) * sq;                     // a / 2^c is exact (v lies in [3, 8]); the product rounds as :265
}

// simulate_nvfp4_amax (:269-278) with quantize_fp8_e4m3 (:205-246): s = a / 6 in float32 (0 unless a > 0), e = floor(log2 s);
// e > 7 → 240, e < -6 → the 2^-9 grid, else 1 + round-half-even(8 · (s / 2^e − 1)) / 8 times 2^e with the bump kept at e <= 7.
__device__ __forceinline__ float nvfp4_g(float a, float s)
{
    if (!(a > 0.0f) || s == 0.0f) return 0.0f;               // NaN a takes s = 0 (:272) and returns 0 (:274-275)
    if (!(s < INFINITY)) return __uint_as_float(0x7FC00000u); // Inf: s_q = Inf, a / s_q = NaN
    int k;
    uint32_t mn;
    split_pos(s, k, mn);
    int e = log2_floor(k, mn);
    float sq;
    if (e > 7) {
        sq = 240.0f;
    } else if (e < -6) {
        sq = __builtin_rintf(s * 512.0f) * 0.001953125f;      // exact scalings; rint is round-half-even like np.round
        if (sq == 0.0f) return 0.0f;
    } else {
        float fq = __builtin_rintf((ldexpf(s, -e) - 1.0f) * 8.0f) * 0.125f;   // every step exact (s / 2^e lies in [1 − 2^-20, 2))
        if (fq >= 1.0f) { fq = 0.0f; e = e + 1 < 7 ? e + 1 : 7; }
        sq = ldexpf(1.0f + fq, e);
    }
    return fp4_level(a / sq) * sq;                            // correctly rounded division, exact product
}

__device__ __forceinline__ float with_sign(float x, float g)
{
    return x > 0.0f ? g : (x < 0.0f ? -g : (x == 0.0f ? 0.0f * g : x));   // np.sign(x) · g; np.sign(±0) = +0, NaN stays NaN
}

template <typename T> __device__ __forceinline__ float load_elem(const T *p);
template <> __device__ __forceinline__ float load_elem<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_elem<uint16_t>(const uint16_t *p) { return __uint_as_float((uint32_t)*p << 16); }

template <int MASK>
__device__ __forceinline__ void accumulate(float x, double acc[kProxyAcc])
{
    const float a = fabsf(x), s = a / 6.0f;
    acc[0] += (double)x;
    acc[1] += (double)(x * x);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        if (!(MASK & (1 << f))) continue;
        const float y = with_sign(x, f == 0 ? mxfp4_g(a, s) : nvfp4_g(a, s));
        const float d = fabsf(x - y);
        double *t = acc + 2 + 5 * f;
        t[0] += (double)y;
        t[1] += (double)(y * y);
        t[2] += (double)(x * y);
        t[3] += (double)d;
        t[4] = nan_max(t[4], (double)d);
    }
}

// One wave's accumulators, combined in a fixed xor tree (every lane ends with the same values).
__device__ __forceinline__ void wave_reduce(double acc[kProxyAcc])
{
#pragma unroll
    for (int k = 0; k < kProxyAcc; ++k) {
        const bool is_max = k >= 2 && (k - 2) % 5 == 4;
#pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) {
            const double o = __shfl_xor(acc[k], sh, 64);
            acc[k] = is_max ? nan_max(acc[k], o) : acc[k] + o;
        }
    }
}

// Phase 1: block (b, m) reads rows b, b + G, b + 2G, ... of matrix m; a thread takes 16-byte pieces of a row (8 bf16 / 4 float32 elements)
// at a stride of the block, in order.  vec: rows and matrices start 16-byte aligned, so a whole piece is one load.
template <typename T, int MASK>
__global__ __launch_bounds__(kProxyThreads) void fp4_proxy_partials(const T *__restrict__ x, int64_t stride, int64_t rows, int64_t cols, int64_t ld,
                                                                   int vec, double *__restrict__ partial)
{
    constexpr int V = 16 / sizeof(T);
    const int64_t m = blockIdx.y, G = gridDim.x;
    const T *xm = x + m * stride;
    double acc[kProxyAcc];
#pragma unroll
    for (int k = 0; k < kProxyAcc; ++k) acc[k] = 0.0;
    const int64_t pieces = (cols + V - 1) / V;
    for (int64_t r = blockIdx.x; r < rows; r += G) {
        const T *xr = xm + r * ld;
        for (int64_t p = threadIdx.x; p < pieces; p += kProxyThreads) {
            const int64_t c0 = p * V;
            if (vec && c0 + V <= cols) {
                const uint4 w = *reinterpret_cast<const uint4 *>(xr + c0);
                const uint32_t q[4] = {w.x, w.y, w.z, w.w};
                if constexpr (sizeof(T) == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        accumulate<MASK>(__uint_as_float(q[i] << 16), acc);
                        accumulate<MASK>(__uint_as_float(q[i] & 0xFFFF0000u), acc);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) accumulate<MASK>(__uint_as_float(q[i]), acc);
                }
            } else {
                for (int64_t c = c0; c < cols && c < c0 + V; ++c) accumulate<MASK>(load_elem<T>(xr + c), acc);
            }
        }
    }
    wave_reduce(acc);
    __shared__ double lds[kProxyThreads / 64][kProxyAcc];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kProxyAcc; ++k) lds[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kProxyAcc) {
        const int k = threadIdx.x;
        const bool is_max = k >= 2 && (k - 2) % 5 == 4;
        double v = lds[0][k];
        for (int w = 1; w < kProxyThreads / 64; ++w) v = is_max ? nan_max(v, lds[w][k]) : v + lds[w][k];
        partial[(m * G + blockIdx.x) * kProxyAcc + k] = v;
    }
}

// Phase 2: one wave per matrix: lane ℓ adds the partials of blocks ℓ, ℓ + 64, ... in order, then the xor tree; lane 0 writes
// sums[m][f][0..6] = Σx, Σx², Σy, Σy², Σxy, Σ|x−y|, max|x−y| for every proxy f in the mask.
__global__ __launch_bounds__(64) void fp4_proxy_finish(const double *__restrict__ partial, int64_t G, uint32_t mask, double *__restrict__ sums)
{
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x;
    double acc[kProxyAcc];
#pragma unroll
    for (int k = 0; k < kProxyAcc; ++k) acc[k] = 0.0;
    for (int64_t b = lane; b < G; b += 64) {
        const double *p = partial + (m * G + b) * kProxyAcc;
#pragma unroll
        for (int k = 0; k < kProxyAcc; ++k) {
            const bool is_max = k >= 2 && (k - 2) % 5 == 4;
            acc[k] = is_max ? nan_max(acc[k], p[k]) : acc[k] + p[k];
        }
    }
    wave_reduce(acc);
    if (lane == 0) {
        for (int f = 0; f < 2; ++f) {
            if (!(mask & (1u << f))) continue;
            double *o = sums + (m * 2 + f) * 7;
            o[0] = acc[0];
            o[1] = acc[1];
            for (int j = 0; j < 5; ++j) o[2 + j] = acc[2 + 5 * f + j];
        }
    }
}

template <typename T, int FMT>
__global__ __launch_bounds__(256) void fp4_proxy_quantize_kernel(const T *__restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                                 float *__restrict__ y, int64_t ldy)
{
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (c >= cols) continue;
        const float xv = load_elem<T>(x + r * ld + c), a = fabsf(xv), s = a / 6.0f;
        y[r * ldy + c] = with_sign(xv, FMT == MTQ_FMT_MXFP4 ? mxfp4_g(a, s) : nvfp4_g(a, s));
    }
}

int64_t blocks_per_matrix(int64_t rows, int64_t cols)
{
    const int64_t want = (rows * cols + kProxyElemsPerBlock - 1) / kProxyElemsPerBlock;
    return std::max<int64_t>(1, std::min<int64_t>(rows, want));
}

template <typename T>
void launch_partials(const void *x, int64_t count, int64_t stride, int64_t rows, int64_t cols, int64_t ld, uint32_t mask, int vec, int64_t G,
                     double *partial, hipStream_t s)
{
    const dim3 grid((unsigned)G, (unsigned)count);
    const T *xt = static_cast<const T *>(x);
    if (mask == 1u)
        hipLaunchKernelGGL((fp4_proxy_partials<T, 1>), grid, dim3(kProxyThreads), 0, s, xt, stride, rows, cols, ld, vec, partial);
    else if (mask == 2u)
        hipLaunchKernelGGL((fp4_proxy_partials<T, 2>), grid, dim3(kProxyThreads), 0, s, xt, stride, rows, cols, ld, vec, partial);
    else
        hipLaunchKernelGGL((fp4_proxy_partials<T, 3>), grid, dim3(kProxyThreads), 0, s, xt, stride, rows, cols, ld, vec, partial);
}

} // namespace

// mtq_quantize's MTQ_FMT_MXFP4 / MTQ_FMT_NVFP4 (arguments checked by mtq_quantize).
int fp4_proxy_quantize(const void *x, int in_dtype, int64_t rows, int64_t cols, int64_t ld, int fmt, float *y, int64_t ldy, void *stream)
{
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool bf = in_dtype == MTQ_DTYPE_BF16, mx = fmt == MTQ_FMT_MXFP4;
    if (bf && mx)
        hipLaunchKernelGGL((fp4_proxy_quantize_kernel<uint16_t, MTQ_FMT_MXFP4>), grid, dim3(256), 0, s, static_cast<const uint16_t *>(x), rows, cols, ld, y, ldy);
    else if (bf)
        hipLaunchKernelGGL((fp4_proxy_quantize_kernel<uint16_t, MTQ_FMT_NVFP4>), grid, dim3(256), 0, s, static_cast<const uint16_t *>(x), rows, cols, ld, y, ldy);
    else if (mx)
        hipLaunchKernelGGL((fp4_proxy_quantize_kernel<float, MTQ_FMT_MXFP4>), grid, dim3(256), 0, s, static_cast<const float *>(x), rows, cols, ld, y, ldy);
    else
        hipLaunchKernelGGL((fp4_proxy_quantize_kernel<float, MTQ_FMT_NVFP4>), grid, dim3(256), 0, s, static_cast<const float *>(x), rows, cols, ld, y, ldy);
    return check_launch("mtq_quantize (fp4 proxy)");
}

} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_fp4_proxy_scratch_doubles(int64_t count, int64_t rows, int64_t cols)
{
    if (count <= 0 || rows <= 0 || cols <= 0) return 0;
    return (size_t)(count * blocks_per_matrix(rows, cols) * kProxyAcc);
}

extern "C" int mtq_fp4_proxy_sums(const void *x, int in_dtype, int64_t count, int64_t stride_elems, int64_t rows, int64_t cols, int64_t ld,
                                  uint32_t fmt_mask, double *sums, double *scratch, size_t scratch_doubles, void *stream)
{
    if (!x || !sums || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (in_dtype != MTQ_DTYPE_BF16 && in_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "in_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (rows <= 0 || cols <= 0 || count <= 0) return fail(MTQ_ERR_INVALID, "count, rows and cols must be positive");
    if (ld < cols) return fail(MTQ_ERR_INVALID, "ld < cols");
    if (count > 1 && stride_elems < (rows - 1) * ld + cols) return fail(MTQ_ERR_INVALID, "stride_elems is smaller than one matrix");
    if (fmt_mask == 0u || (fmt_mask & ~3u) != 0u) return fail(MTQ_ERR_INVALID, "fmt_mask must be 1..3 (bit 0 mxfp4, bit 1 nvfp4)");
    if (rows > (int64_t)1 << 40 || cols > (int64_t)1 << 30 || count > 65535) return fail(MTQ_ERR_INVALID, "batch too large for one launch");
    const int64_t G = blocks_per_matrix(rows, cols);
    if (G > INT32_MAX || scratch_doubles < (size_t)(count * G * kProxyAcc)) return fail(MTQ_ERR_INVALID, "scratch is smaller than mtq_fp4_proxy_scratch_doubles");
    if (int rc = require_device()) return rc;
    const int64_t esz = in_dtype == MTQ_DTYPE_BF16 ? 2 : 4;
    const int vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && (ld * esz) % 16 == 0 && (count == 1 || (stride_elems * esz) % 16 == 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_dtype == MTQ_DTYPE_BF16)
        launch_partials<uint16_t>(x, count, stride_elems, rows, cols, ld, fmt_mask, vec, G, scratch, s);
    else
        launch_partials<float>(x, count, stride_elems, rows, cols, ld, fmt_mask, vec, G, scratch, s);
    if (int rc = check_launch("mtq_fp4_proxy_sums (partials)")) return rc;
    hipLaunchKernelGGL(fp4_proxy_finish, dim3((unsigned)count), dim3(64), 0, s, scratch, G, fmt_mask, sums);
    return check_launch("mtq_fp4_proxy_sums");
}
