// mtq_awq.hip — AWQ for BFP: the search over per-input-channel exponent shifts (quantization_analysis_amd/awq.py holds the contract).
//
// Slot g of the shift table p (int8 [G′, k], 0 .. 7) quantises element (r, j) of W at the exponent E − p[g, j], E = the group's largest
// e_i + p[g, i] over its elements with a non-zero exponent field: the BFP of W·2^p scaled back by 2^−p, with nothing rounded twice.
// mtq_awq_losses forms loss[g] = Σ (fl32(r − q_g))² over all m·n outputs, r = X·Wᵀ and q_g = X·Ŵ_gᵀ, for every slot in one pass over X
// per launch of kS slots; mtq_awq_quantize writes Ŵ of one shift row.
//
// Losses: LOE's block shape (mtq_output_error.hip): 4 waves own 128 (M) × 64 (N) outputs and walk K in steps of 64; the X tile and the
// W images are bf16 in LDS, each wave forms 32 × 64 outputs per accumulator with mfma_f32_32x32x16_bf16, one A fragment per 16 columns
// of K feeding R and every slot.  What is new is the staging: a lane owns one 16-element group of one W row, reads its exponent fields
// ONCE, and per slot only (a) adds the slot's shifts to the fields and takes the maximum (integer), (b) runs the element rule in the
// group's 24-bit window with the shift folded into the two power-of-two constants of the exact-scaling route:
//     a = trunc(w · 2^(150 − E + p))          the aligned mantissa (exact scaling; p moves only the constant's exponent field)
//     q = clamp((a + C) − C, ±ymax)           RNE to M bits with the saturating round-up; C, ymax depend on M alone
//     ŵ = q · 2^(E − 150 − p)                 exact
// which is 9 VALU operations per element and slot against about 25 for the literal rule.  That route holds for E in [48, 200]; a group
// outside it (all-zero groups included) takes bfp_elem_bits_rt with the shared exponent E − p per element.  The shifts are read by each
// lane straight from p (4·kS distinct 16-byte pieces per step, L1-resident), a step ahead, with the lane's W group and X pieces.
// The K loop is LOE's: stage step k → barrier → MFMA step k → barrier, the global loads of step k + 1 in flight behind the MFMAs.  A
// second form with two LDS buffers, step k + 1's images written slot by slot between step k's MFMAs, was built and measured: 1.01× for
// bf16 W, inside the spread, and 0.86× for float32 W, which has room for 3 slots only; it was not kept.
// Epilogue: d = fl32(r − q_s) squared and summed in float64 per lane, a wave butterfly, the 4 waves in order, one record of kS doubles
// per workgroup; awq_reduce adds the records in index order into loss (no float atomics: equal inputs give equal bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kBM = 128, kBN = 64, kBK = 64, kThreads = 256;
constexpr int kLdk = kBK + 8;                      // LDS row pitch in bf16 (144 B, as LOE)
constexpr int kS = 5;                              // slots per launch: R + 5 accumulator pairs (R is two pairs for float32 W)
constexpr int kImgElems = kBN * kLdk;
constexpr uint32_t kFastLo = 48u, kFastSpan = 152u;   // the exact-scaling route: E in [48, 200]
constexpr int kMaxShift = 7;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bits_f(uint32_t v) { return __uint_as_float(v); }

__device__ __forceinline__ void store_image(uint16_t *dst, const uint32_t (&y)[kGroup])
{
    uint32_t pk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pk[i] = (y[2 * i] >> 16) | (y[2 * i + 1] & 0xFFFF0000u);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    d[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    d[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
}

// What a lane keeps of its group across the slots: the exponent fields in place (bits 23..30; an element without one can never win a
// maximum), and its tile's format as the constants of the window rule.
struct GroupPrep {
    int em[kGroup];
    uint32_t M;
    float C, ymax;
    bool is_bf16;
};

__device__ __forceinline__ GroupPrep prep_group(const uint32_t (&u)[kGroup], int code)
{
    GroupPrep g;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const uint32_t e = u[i] & 0x7F800000u;
        g.em[i] = e ? (int)e : -0x40000000;
    }
    g.is_bf16 = code == 0;
    g.M = code == 1 ? 7u : (code == 2 ? 3u : 1u);
    g.C = bits_f(((174u - g.M) << 23) | 0x400000u);                    // 1.5 · 2^(47 − M): rounds to multiples of 2^(24 − M)
    g.ymax = (float)((1u << g.M) - 1u) * bits_f((151u - g.M) << 23);   // (2^M − 1) · 2^(24 − M)
    return g;
}

// The shifts of the lane's 16 columns (bytes of pw, 0 .. 7) as exponent-field increments.
__device__ __forceinline__ void shift_fields(const uint4 &pw, uint32_t (&psh)[kGroup])
{
    const uint32_t w[4] = {pw.x, pw.y, pw.z, pw.w};
#pragma unroll
    for (int i = 0; i < kGroup; ++i) psh[i] = ((w[i >> 2] >> (8 * (i & 3))) & (uint32_t)kMaxShift) << 23;
}

// Ŵ of one slot for the lane's group → y (float32 words; every one has its low 16 bits zero).
__device__ __forceinline__ void quantize_slot(const uint32_t (&u)[kGroup], const GroupPrep &g, const uint4 &pw, uint32_t (&y)[kGroup])
{
    if (g.is_bf16) {                                                   // a bf16 tile ignores p
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
        return;
    }
    uint32_t psh[kGroup];
    shift_fields(pw, psh);
    int emax = 0;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) emax = max(emax, g.em[i] + (int)psh[i]);
    const uint32_t E = (uint32_t)emax >> 23;
    const bool fast = (E - kFastLo) <= kFastSpan;
    const uint32_t Ec = fast ? E : 127u;
    const uint32_t ka = (277u - Ec) << 23, kb = (Ec - 23u) << 23;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const float a = __builtin_truncf(bits_f(u[i]) * bits_f(ka + psh[i]));
        const float r = (a + g.C) - g.C;
        y[i] = __float_as_uint(__builtin_amdgcn_fmed3f(r, -g.ymax, g.ymax) * bits_f(kb - psh[i]));
    }
    if (!fast) {                                                       // rare: the literal rule at the element's own shared exponent
#pragma unroll
        for (int i = 0; i < kGroup; ++i) y[i] = bfp_elem_bits_rt(u[i], E - (psh[i] >> 23), g.M);
    }
}

// hi = bf16(W), and for float32 W mid = bf16(W − hi), lo = bf16(W − hi − mid): the reference images of mtq_output_error.
template <bool F32>
__device__ __forceinline__ void stage_reference(const uint32_t (&u)[kGroup], uint16_t *img0, int img_off)
{
    uint32_t y[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) y[i] = bf16_round_bits(u[i]);
    store_image(img0 + img_off, y);
    if constexpr (F32) {
        uint32_t r1[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const float d1 = bits_f(u[i]) - bits_f(y[i]);                // exact
            r1[i] = bf16_round_bits(__float_as_uint(d1));
            y[i] = bf16_round_bits(__float_as_uint(d1 - bits_f(r1[i])));  // exact, at most 8 significant bits
        }
        store_image(img0 + kImgElems + img_off, r1);
        store_image(img0 + 2 * kImgElems + img_off, y);
    }
}

// kS slots per launch; `slots` (1 .. kS) of them are live, the others run on zero shifts and their records are not read (a branch
// around a slot.s MFMAs costs the accumulators their place in the AGPRs).  p: the first live slot.s row of the table.
template <typename T>
__global__ __launch_bounds__(kThreads) void awq_losses_kernel(const uint16_t *__restrict__ x, int64_t M, int64_t K, int64_t ldx, int x_vec,
                                                              const T *__restrict__ w, int64_t N, int64_t ldw, int w_vec,
                                                              const int8_t *__restrict__ codes, int64_t tw, const int8_t *__restrict__ p,
                                                              int p_vec, int slots, double *__restrict__ partials)
{
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int S = kS, kRef = F32 ? 3 : 1;
    __shared__ __attribute__((aligned(16))) uint16_t lds[(kBM + (kRef + S) * kBN) * kLdk];
    __shared__ double red[4][S];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nblocks = (N + kBN - 1) / kBN;
    const int64_t bm = blockIdx.x / nblocks, bn = blockIdx.x % nblocks;
    const int64_t m0 = bm * kBM, n0 = bn * kBN;

    f32x16 acc[S][2], ref[F32 ? 2 : 1][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int a = 0; a < S; ++a) acc[a][s2][r] = 0.0f;
#pragma unroll
            for (int a = 0; a < (F32 ? 2 : 1); ++a) ref[a][s2][r] = 0.0f;
        }

    // global → registers one K-step ahead: the lane's X pieces, its W group (row tid / 4, columns 16·(tid % 4) ..) and the shifts of
    // those 16 columns in every live slot
    const int wrow = tid >> 2, wc16 = (tid & 3) * kGroup;
    const int img_off = wrow * kLdk + wc16;
    uint4 xr[4], pw[S];
    uint32_t wu[kGroup];
    int code = 0;
    auto load_step = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // X: 128 rows × 64 columns = 1024 pieces of 8 bf16, 4 per thread
            const int pc = tid + kThreads * i, row = pc >> 3, c8 = (pc & 7) * 8;
            const int64_t gm = m0 + row, gk = k0 + c8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gm < M) {
                const uint16_t *src = x + gm * ldx + gk;
                if (x_vec && gk + 8 <= K) {
                    v = *reinterpret_cast<const uint4 *>(src);
                } else {
                    uint32_t h[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) h[j] = gk + j < K ? (uint32_t)src[j] : 0u;
                    v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                }
            }
            xr[i] = v;
        }
        const int64_t gn = n0 + wrow, gk = k0 + wc16;
        Loader<T>::group(w, gn, gk, N, K, ldw, w_vec != 0, wu);
        code = (gn < N && gk < K) ? (int)codes[(gn / kTile) * tw + gk / kTile] : 0;   // the zero padding of a ragged edge stays zero
#pragma unroll
        for (int s = 0; s < S; ++s) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (s < slots && gk < K) {
                const int8_t *src = p + (int64_t)s * K + gk;
                if (p_vec && gk + kGroup <= K) {
                    v = *reinterpret_cast<const uint4 *>(src);
                } else {
                    uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < kGroup; ++j)
                        if (gk + j < K) b[j >> 2] |= (uint32_t)(uint8_t)src[j] << (8 * (j & 3));
                    v = make_uint4(b[0], b[1], b[2], b[3]);
                }
            }
            pw[s] = v;
        }
    };
    const int koff = 8 * (lane >> 5);
    const int aoff = (wave * 32 + (lane & 31)) * kLdk + koff;
#define MTQ_AWQ_MFMA(ACC, IMG)                                                                                                       \
    _Pragma("unroll") for (int kk = 0; kk < kBK / 16; ++kk) _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2)                        \
        ACC[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                                                                           \
            a[kk], *reinterpret_cast<const bf16x8 *>(img0 + (IMG) * kImgElems + (s2 * 32 + (lane & 31)) * kLdk + kk * 16 + koff), ACC[s2], 0, 0, 0)

    load_step(0);
    uint16_t *xs = lds, *img0 = lds + kBM * kLdk;
    for (int64_t k0 = 0; k0 < K; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pc = tid + kThreads * i;
            *reinterpret_cast<uint4 *>(xs + (pc >> 3) * kLdk + (pc & 7) * 8) = xr[i];
        }
        stage_reference<F32>(wu, img0, img_off);
        const GroupPrep g = prep_group(wu, code);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            uint32_t y[kGroup];
            quantize_slot(wu, g, pw[s], y);
            store_image(img0 + (kRef + s) * kImgElems + img_off, y);
            __builtin_amdgcn_sched_barrier(0);                           // one slot's temporaries at a time: the slots share their registers
        }
        __syncthreads();
        if (k0 + kBK < K) load_step(k0 + kBK);
        bf16x8 a[kBK / 16];
#pragma unroll
        for (int kk = 0; kk < kBK / 16; ++kk) a[kk] = *reinterpret_cast<const bf16x8 *>(xs + aoff + kk * 16);
        MTQ_AWQ_MFMA(ref[0], 0);
        if constexpr (F32) { MTQ_AWQ_MFMA(ref[1], 1); MTQ_AWQ_MFMA(ref[1], 2); }
#pragma unroll
        for (int s = 0; s < S; ++s)
            MTQ_AWQ_MFMA(acc[s], kRef + s);
        __syncthreads();
    }
#undef MTQ_AWQ_MFMA

    // epilogue: lane's outputs are (m0 + 32·wave + (r&3) + 8(r>>2) + 4(lane>>5), n0 + 32·s2 + (lane&31))
    double sum[S];
#pragma unroll
    for (int s = 0; s < S; ++s) sum[s] = 0.0;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const int64_t n = n0 + 32 * s2 + (lane & 31);
        if (n >= N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= M) continue;
            float rf = ref[0][s2][r];
            if constexpr (F32) rf = rf + ref[1][s2][r];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double d = (double)(rf - acc[s][s2][r]);
                sum[s] += d * d;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double v = sum[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][s] = v;
    }
    __syncthreads();
    if (tid < S) partials[(int64_t)blockIdx.x * kS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// loss[i] += the workgroup records of slot i = blockIdx.x in index order: each thread a strided slice, then a fixed tree.
__global__ __launch_bounds__(256) void awq_reduce(const double *__restrict__ partials, int64_t nblocks, double *__restrict__ loss)
{
    __shared__ double buf[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double v = 0.0;
    for (int64_t b = tid; b < nblocks; b += 256) v += partials[b * kS + i];
    buf[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) buf[tid] = buf[tid] + buf[tid + s];
        __syncthreads();
    }
    if (tid == 0) loss[i] += buf[0];
}

// Ŵ of one shift row as float32: a lane per group, rows over gridDim.y.
template <typename T>
__global__ __launch_bounds__(256) void awq_quantize_kernel(const T *__restrict__ w, int64_t N, int64_t K, int64_t ldw, int w_vec,
                                                           const int8_t *__restrict__ codes, int64_t tw, const int8_t *__restrict__ p,
                                                           float *__restrict__ out, int64_t ldo)
{
    const int64_t col0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kGroup;
    if (col0 >= K) return;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
        if (col0 + j < K) b[j >> 2] |= (uint32_t)(uint8_t)p[col0 + j] << (8 * (j & 3));
    const uint4 pw = make_uint4(b[0], b[1], b[2], b[3]);
    for (int64_t row = blockIdx.y; row < N; row += gridDim.y) {
        uint32_t u[kGroup], y[kGroup];
        Loader<T>::group(w, row, col0, N, K, ldw, w_vec != 0, u);
        const GroupPrep g = prep_group(u, (int)codes[(row / kTile) * tw + col0 / kTile]);
        quantize_slot(u, g, pw, y);
#pragma unroll
        for (int i = 0; i < kGroup; ++i)
            if (col0 + i < K) out[row * ldo + col0 + i] = bits_f(y[i]);
    }
}

template <typename T>
int launch_losses(hipStream_t st, int64_t blocks, const uint16_t *x, int64_t m, int64_t k, int64_t ldx, int x_vec, const void *w, int64_t n,
                  int64_t ldw, int w_vec, const int8_t *codes, int64_t tw, const int8_t *p, int p_vec, int g_count, double *loss, double *scratch)
{
    for (int g0 = 0; g0 < g_count; g0 += kS) {
        const int slots = std::min(kS, g_count - g0);
        hipLaunchKernelGGL(awq_losses_kernel<T>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, m, k, ldx, x_vec,
                           static_cast<const T *>(w), n, ldw, w_vec, codes, tw, p + (int64_t)g0 * k, p_vec, slots, scratch);
        if (int rc = check_launch("mtq_awq_losses")) return rc;
        hipLaunchKernelGGL(awq_reduce, dim3((unsigned)slots), dim3(256), 0, st, scratch, blocks, loss + g0);
        if (int rc = check_launch("mtq_awq_losses (reduce)")) return rc;
    }
    return MTQ_OK;
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_awq_losses_scratch_doubles(int64_t m, int64_t n, int g_count)
{
    if (m <= 0 || n <= 0 || g_count <= 0) return 0;
    return (size_t)(((m + kBM - 1) / kBM) * ((n + kBN - 1) / kBN)) * kS;
}

extern "C" int mtq_awq_losses(const void *x, int64_t m, int64_t k, int64_t ldx, const void *w, int w_dtype, int64_t n, int64_t ldw,
                              const int8_t *codes, size_t code_count, const int8_t *p, int g_count, double *loss, double *scratch,
                              size_t scratch_doubles, void *stream)
{
    if (!x || !w || !codes || !p || !loss || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (m <= 0 || n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "m, n and k must be positive (empty operands are handled by the caller)");
    if (g_count <= 0 || g_count > 4096) return fail(MTQ_ERR_INVALID, "g_count must lie in 1 .. 4096");
    if (ldx < k) return fail(MTQ_ERR_INVALID, "ldx < k");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (m > (int64_t)1 << 40 || n > (int64_t)1 << 30 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t th = (n + kTile - 1) / kTile, tw = (k + kTile - 1) / kTile;
    if (code_count != (size_t)(th * tw)) return fail(MTQ_ERR_INVALID, "code_count != ceil(n / 32) * ceil(k / 32)");
    const int64_t blocks = ((m + kBM - 1) / kBM) * ((n + kBN - 1) / kBN);
    if (blocks > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many workgroups for one launch: pass M in chunks");
    if (scratch_doubles < mtq_awq_losses_scratch_doubles(m, n, g_count))
        return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_awq_losses_scratch_doubles(m, n, g_count)");
    if (int rc = require_device()) return rc;

    const bool f32w = w_dtype == MTQ_DTYPE_F32;
    const int x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * (f32w ? 4 : 2)) % 16 == 0;
    const int p_vec = reinterpret_cast<uintptr_t>(p) % 16 == 0 && k % 16 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *xp = static_cast<const uint16_t *>(x);
    if (f32w) return launch_losses<float>(st, blocks, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, codes, tw, p, p_vec, g_count, loss, scratch);
    return launch_losses<uint16_t>(st, blocks, xp, m, k, ldx, x_vec, w, n, ldw, w_vec, codes, tw, p, p_vec, g_count, loss, scratch);
}

extern "C" int mtq_awq_quantize(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const int8_t *codes, size_t code_count,
                                const int8_t *p_row, float *out, int64_t ldo, void *stream)
{
    if (!w || !codes || !p_row || !out) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "n and k must be positive");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (ldo < k) return fail(MTQ_ERR_INVALID, "ldo < k");
    if (n > (int64_t)1 << 30 || k > (int64_t)1 << 30) return fail(MTQ_ERR_INVALID, "matrix too large");
    const int64_t th = (n + kTile - 1) / kTile, tw = (k + kTile - 1) / kTile;
    if (code_count != (size_t)(th * tw)) return fail(MTQ_ERR_INVALID, "code_count != ceil(n / 32) * ceil(k / 32)");
    if (int rc = require_device()) return rc;
    const bool f32w = w_dtype == MTQ_DTYPE_F32;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * (f32w ? 4 : 2)) % 16 == 0;
    const int64_t gw = (k + kGroup - 1) / kGroup;
    const dim3 grid((unsigned)((gw + 255) / 256), (unsigned)std::min<int64_t>(n, 65535));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (f32w)
        hipLaunchKernelGGL(awq_quantize_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(w), n, k, ldw, w_vec, codes, tw, p_row, out, ldo);
    else
        hipLaunchKernelGGL(awq_quantize_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t *>(w), n, k, ldw, w_vec, codes, tw, p_row, out,
                           ldo);
    return check_launch("mtq_awq_quantize");
}
