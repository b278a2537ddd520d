// mtq_gptq_transpose.hip — GPTQ's column sweep in the transposed BFP layout (quantization_analysis_amd/gptq.py holds the contract).
//
// mtq_gptq_sweep_transposed: a shared-exponent group is 16 consecutive ROWS of one column, so the rows of a group meet at every column
//   through E, and all 16 values of a group are final at the step that quantises them: E is the maximum exponent field of the values
//   actually quantised, never a stale one.  A workgroup of 4 waves owns a strip of 32 rows (tile column nb of Wᵀ's grid, two groups)
//   and walks its 32-column blocks left to right; the block's code codes[(b0 / 32) · tn + nb] is uniform over the strip.
//   * The GEMM-shaped part, Σ_{i < b0} e_i · U[i, block], does not depend on the layout: float64 VALU fma from LDS-staged 16-column
//     chunks of Eᵀ and U, the chunks dealt round-robin over the 4 waves and the 4 partials added in wave order (mtq_gptq.hip's scheme
//     and summation order).
//   * The 32 sequential steps run in wave 0 with lane = (half, row): lane l holds row l & 31 and the 16-column half l >> 5 of the block
//     in registers.  A group is then 16 consecutive lanes, one DPP row: E at step j is a 4-step rotate-and-max (row_ror 8, 4, 2, 1) of
//     the exponent fields over that row, which leaves the maximum in all 16 lanes, with no LDS and no readlane on the chain.  The error
//     of the half that owns column j crosses to the other half by v_permlane32_swap (two 32-bit swaps for a double), and both halves
//     apply the rank-1 update with U's diagonal block from LDS.
//   Rows ≥ N load as +0 (exponent field 0: never raises a maximum; q = 0, e = 0) and columns ≥ K are skipped.  e goes to scratch as Eᵀ
//   (k_pad × n_pad doubles), a step's 32 rows in one 256-byte run.  No atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtq_device.hpp"
#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kTChunk = 16;            // earlier columns per LDS-staged chunk of the GEMM-shaped part

__device__ __forceinline__ double2 ld2t(const double *p) { return *reinterpret_cast<const double2 *>(p); }

// max over the 16 lanes of a DPP row, in every lane of it: rotate right by 8, 4, 2, 1 within the row
__device__ __forceinline__ uint32_t row16_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false));
    return v;
}

// v is a value in the lanes of one half of the wave and +0.0 in the other half → that value in lanes l and l ^ 32.  One swap of v with
// itself gives the low half's word in both halves in one result and the high half's in the other; one of the two is the zero word.
__device__ __forceinline__ double across_halves(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    const auto slo = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto shi = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const uint64_t r = (uint64_t)(slo[0] | slo[1]) | ((uint64_t)(shi[0] | shi[1]) << 32);
    return __longlong_as_double((long long)r);
}

template <typename T>
__global__ __launch_bounds__(256) void gptq_sweep_transposed_kernel(const T *__restrict__ w, int64_t N, int64_t K, int64_t ldw, int w_vec,
                                                                    const double *__restrict__ u, int u_vec, const int8_t *__restrict__ codes,
                                                                    int64_t tn, float *__restrict__ out, int64_t ldo, double *__restrict__ loss,
                                                                    double *__restrict__ et, int64_t lde)
{
    // per wave: Eᵀ chunk [16][32] then U chunk [16][32] (8 KB); after the GEMM part the same 8 KB hold the wave's 32 × 32 partial
    __shared__ __attribute__((aligned(16))) double stage[4][2 * kTChunk * kTile];
    __shared__ __attribute__((aligned(16))) double ud[kTile][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int64_t nb = blockIdx.x;
    double *es = stage[wave], *us = stage[wave] + kTChunk * kTile;
    const int rg = lane >> 3, cg = lane & 7;                   // GEMM part: rows 4rg .. +3, columns 4cg .. +3 of the block
    const int row = lane & 31, half = lane >> 5;               // sweep (wave 0): row, 16-column half; a group is one DPP row
    const int64_t grow = r0 + row;
    double lsum = 0.0;

    for (int64_t b0 = 0; b0 < K; b0 += kTile) {
        // ---- Σ_{i < b0} e_i · U[i, b0 + col] for the strip: chunk ch = 4t + wave of the b0 / 16 earlier chunks
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        const int64_t nch = b0 / kTChunk, trips = (nch + 3) / 4;
        double2 er[4], ur[4];
        auto load_chunk = [&](int64_t ch) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int pc = lane + 64 * s, ii = pc >> 4, c2 = (pc & 15) * 2;
                const int64_t gi = ch * kTChunk + ii;            // < b0 <= K − 1: a row of U and of Eᵀ that exists
                er[s] = ld2t(et + gi * lde + r0 + c2);
                const int64_t gc = b0 + c2;
                if (u_vec && gc + 1 < K) {
                    ur[s] = ld2t(u + gi * K + gc);
                } else {
                    ur[s].x = gc < K ? u[gi * K + gc] : 0.0;
                    ur[s].y = gc + 1 < K ? u[gi * K + gc + 1] : 0.0;
                }
            }
        };
        if (wave < nch) load_chunk(wave);
        for (int64_t t = 0; t < trips; ++t) {
            const int64_t ch = 4 * t + wave;
            __syncthreads();
            if (ch < nch) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int pc = lane + 64 * s, ii = pc >> 4, c2 = (pc & 15) * 2;
                    *reinterpret_cast<double2 *>(es + ii * kTile + c2) = er[s];
                    *reinterpret_cast<double2 *>(us + ii * kTile + c2) = ur[s];
                }
            }
            __syncthreads();
            if (ch + 4 < nch) load_chunk(ch + 4);
            if (ch < nch) {
#pragma unroll 4
                for (int ii = 0; ii < kTChunk; ++ii) {
                    const double2 e01 = ld2t(es + ii * kTile + 4 * rg), e23 = ld2t(es + ii * kTile + 4 * rg + 2);
                    const double2 u01 = ld2t(us + ii * kTile + 4 * cg), u23 = ld2t(us + ii * kTile + 4 * cg + 2);
                    const double ev[4] = {e01.x, e01.y, e23.x, e23.y}, uv[4] = {u01.x, u01.y, u23.x, u23.y};
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[r][c] = fma(ev[r], uv[c], acc[r][c]);
                }
            }
        }
        __syncthreads();
        {   // the wave's partial into its own stage region; U's diagonal block (upper triangle only) into ud
            double *red = stage[wave];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) red[(4 * rg + r) * kTile + 4 * cg + c] = acc[r][c];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int idx = tid + 256 * s, i = idx >> 5, c = idx & 31;
                const int64_t gi = b0 + i, gc = b0 + c;
                ud[i][c] = (gi < K && gc < K && c >= i) ? u[gi * K + gc] : 0.0;
            }
        }
        __syncthreads();
        if (wave == 0) {
            // ---- the 32 sequential steps of the block: lane (half, row) holds columns b0 + 16·half .. + 15 of its row
            const int code = (int)codes[(b0 / kTile) * tn + nb];
            const bool is_bf16 = code == 0;
            const uint32_t M = code == 1 ? 7u : (code == 2 ? 3u : 1u);
            uint32_t wu[kGroup];
            Loader<T>::group(w, grow, b0 + 16 * half, N, K, ldw, w_vec != 0, wu);
            double cur[kGroup], eo[kGroup];
            uint32_t qo[kGroup];
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                const int a = row * kTile + 16 * half + c;
                const double v = ((stage[0][a] + stage[1][a]) + stage[2][a]) + stage[3][a];
                cur[c] = (double)__uint_as_float(wu[c]) - v;
                eo[c] = 0.0;
                qo[c] = 0u;
            }
#pragma unroll
            for (int j = 0; j < kTile; ++j) {
                const int gsel = j >> 4, c = j & 15;
                const bool mine = half == gsel && b0 + j < K;
                // the exponent of the column group: the 16 rows of this lane's DPP row (the other half reduces a column of its own
                // that it does not use)
                const uint32_t xu = __float_as_uint((float)cur[c]);
                const uint32_t E = row16_max(xu & 0x7F800000u) >> 23;
                const uint32_t qb = is_bf16 ? bf16_round_bits(xu) : bfp_elem_bits_sat(xu, E, M);
                double e = 0.0;
                if (mine) {
                    e = (cur[c] - (double)__uint_as_float(qb)) / ud[j][j];
                    qo[c] = qb;
                    eo[c] = e;
                }
                e = across_halves(e);
                lsum = lsum + e * e;
#pragma unroll
                for (int cc = 0; cc < kGroup; ++cc) {
                    // columns > j: cc > c of the owning half, and all of half 1 while half 0 owns the step
                    if (cc > c) {
                        if (gsel == 0 || half == 1) cur[cc] = cur[cc] - e * ud[j][16 * half + cc];
                    } else if (gsel == 0 && half == 1) {
                        cur[cc] = cur[cc] - e * ud[j][16 + cc];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                const int64_t col = b0 + 16 * half + c;           // < k_pad: scratch holds it
                et[col * lde + grow] = eo[c];
                if (grow < N && col < K) out[grow * ldo + col] = __uint_as_float(qo[c]);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && half == 0 && grow < N) loss[grow] = lsum;
}

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" int mtq_gptq_sweep_transposed(const void *w, int w_dtype, int64_t n, int64_t k, int64_t ldw, const double *u, size_t u_doubles,
                                         const int8_t *codes, size_t code_count, float *out, int64_t ldo, double *loss, double *scratch,
                                         size_t scratch_doubles, void *stream)
{
    if (!w || !u || !codes || !out || !loss || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (w_dtype != MTQ_DTYPE_BF16 && w_dtype != MTQ_DTYPE_F32) return fail(MTQ_ERR_INVALID, "w_dtype must be MTQ_DTYPE_BF16 or MTQ_DTYPE_F32");
    if (n <= 0 || k <= 0) return fail(MTQ_ERR_INVALID, "n and k must be positive");
    if (ldw < k) return fail(MTQ_ERR_INVALID, "ldw < k");
    if (ldo < k) return fail(MTQ_ERR_INVALID, "ldo < k");
    if (n > (int64_t)1 << 30 || k > (int64_t)1 << 20) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (u_doubles != (size_t)k * (size_t)k) return fail(MTQ_ERR_INVALID, "u_doubles != k * k");
    const int64_t tn = (n + kTile - 1) / kTile, tk = (k + kTile - 1) / kTile;
    if (code_count != (size_t)(tk * tn)) return fail(MTQ_ERR_INVALID, "code_count != ceil(k / 32) * ceil(n / 32)");
    if (scratch_doubles < mtq_gptq_sweep_scratch_doubles(n, k)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_gptq_sweep_scratch_doubles(n, k)");
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(MTQ_ERR_INVALID, "scratch must be 16-byte aligned");
    if (tn > INT32_MAX) return fail(MTQ_ERR_INVALID, "too many row strips for one launch");
    if (int rc = require_device()) return rc;
    const int64_t esz = w_dtype == MTQ_DTYPE_F32 ? 4 : 2;
    const int w_vec = reinterpret_cast<uintptr_t>(w) % 16 == 0 && (ldw * esz) % 16 == 0;
    const int u_vec = reinterpret_cast<uintptr_t>(u) % 16 == 0 && k % 2 == 0;
    const int64_t lde = tn * kTile;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (w_dtype == MTQ_DTYPE_F32)
        hipLaunchKernelGGL(gptq_sweep_transposed_kernel<float>, dim3((unsigned)tn), dim3(256), 0, st, static_cast<const float *>(w), n, k, ldw, w_vec, u,
                           u_vec, codes, tn, out, ldo, loss, scratch, lde);
    else
        hipLaunchKernelGGL(gptq_sweep_transposed_kernel<uint16_t>, dim3((unsigned)tn), dim3(256), 0, st, static_cast<const uint16_t *>(w), n, k, ldw,
                           w_vec, u, u_vec, codes, tn, out, ldo, loss, scratch, lde);
    return check_launch("mtq_gptq_sweep_transposed");
}
