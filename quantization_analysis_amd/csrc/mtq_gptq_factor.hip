// mtq_gptq_factor.hip — GPTQ's factor U on the device: the upper Cholesky factor of H_d⁻¹, from H_d (quantization_analysis_amd/gptq.py
// holds the contract; mtq_gptq.hip has the Gram matrix before this step and the sweep after it).
//
// H_d = R·Rᵀ with R upper triangular ("reverse" Cholesky, from the bottom-right corner upwards); then H_d⁻¹ = R⁻ᵀR⁻¹, so U = R⁻¹ is upper
// triangular with a positive diagonal and UᵀU = H_d⁻¹: the Cholesky factor, by uniqueness.  H_d⁻¹ is never formed.
//
// Blocks of kNB = 64, block J = indices 64J .. 64J + 63; the last block is padded to 64 with an identity diagonal, in a kp × kp work
// matrix W (scratch, kp = 64·ceil(k / 64)), so no kernel below reads or writes outside a whole block and none reads hd or writes u past
// k.  One launch per stage, ordered by the stream alone; no kernel waits for another workgroup.
//   init      W ← the upper triangle of hd, identity padding, zeros below; status ← 0.
//   for J = nb − 1 .. 0:
//     diag(J)   one workgroup: W_JJ in LDS, right-looking reverse Cholesky (correctly rounded sqrt and division), then V_J = R_JJ⁻¹ by
//               right-looking back substitution; R_JJ → W, V_J and V_Jᵀ → scratch (the panel and the inverse both use them).
//     panel(J)  R_IJ = A_IJ·V_Jᵀ for I < J, one workgroup per block, in place (a workgroup stages all it reads before it writes).
//     trail(J)  A_IK −= R_IJ·R_KJᵀ for I ≤ K < J: one workgroup per block of the upper triangle, the grid holds those blocks only.
//   for I = nb − 2 .. 0:
//     inv(I)    U_IJ = −V_I·Σ_{I<K≤J} R_IK·U_KJ for every J > I, one workgroup per J.  It is formed transposed, T_JI = U_IJᵀ, and kept
//               in W's strict lower triangle: block (J, I) there is written once, by this launch, and read only by later launches
//               (inv(I') with I' < I reads T_JK, K > I'); R lives in the upper triangle and the diagonal blocks and is never overwritten
//               after trail, so no block is read after it is overwritten.
//   emit      u ← T transposed (through LDS), V_J on the diagonal blocks, zeros below.
// Every product above has the form C[m][n] = Σ_kk X[m][kk]·Y[n][kk] with X and Y row-major 64 × 64 blocks (kk contiguous): one GEMM
// body, gemm_step.  A workgroup of 4 waves owns a 64 × 64 block of C, wave (wm, wn) its 32 × 32 quadrant as 2 × 2 tiles of
// v_mfma_f64_16x16x4_f64: 4 accumulators of 4 doubles = 32 accumulator VGPRs per lane.  X and Y are staged whole (64 deep) in LDS, row
// pitch 66 doubles: an MFMA operand is 16 rows × 4 kk, lane l reading (row l & 15, kk l >> 4); a half wave's 32 reads fall on double
// banks (2·row + kk) mod 32, all distinct.  2 × 64 × 66 × 8 = 67 584 bytes of LDS per workgroup, two workgroups per CU: one stages while
// the other multiplies; inside inv's K loop the next pair of blocks is fetched to registers during the multiply.
// Deterministic: every entry is written by one thread in a fixed order, no atomics.  A pivot that is not positive and finite is
// replaced by 1 and reported in status; no trip count depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "mtq_error.hpp"

namespace mtq {
namespace {

constexpr int kNB = MTQ_GPTQ_FACTOR_BLOCK;
constexpr int kPitch = kNB + 2;            // LDS row pitch of a staged operand, doubles
constexpr int kDPitch = kNB + 1;           // LDS row pitch of the diagonal kernel's two blocks
constexpr int kBlk = kNB * kNB;
static_assert(kNB == 64, "the thread maps below are written for 64 x 64 blocks and 256 threads");

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Frag { double2 v[8]; };             // a thread's share of one staged 64 × 64 block: 8 pieces of 2 doubles

// piece p = tid + 256·i of a block: row p >> 5, doubles 2·(p & 31) .. + 1 (32 lanes cover one row's 512 bytes)
__device__ __forceinline__ void load_block(const double *__restrict__ src, int64_t ld, int tid, Frag &f)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = tid + 256 * i;
        f.v[i] = *reinterpret_cast<const double2 *>(src + (int64_t)(p >> 5) * ld + 2 * (p & 31));
    }
}

__device__ __forceinline__ void store_block_lds(double *dst, int tid, const Frag &f)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = tid + 256 * i;
        *reinterpret_cast<double2 *>(dst + (p >> 5) * kPitch + 2 * (p & 31)) = f.v[i];
    }
}

// acc[mi][ni] += Σ_kk xs[32wm + 16mi + ·][kk] · ys[32wn + 16ni + ·][kk] over the 64 staged kk
__device__ __forceinline__ void gemm_step(const double *xs, const double *ys, int lane, int wm, int wn, f64x4 (&acc)[2][2])
{
    const int r = lane & 15, q = lane >> 4;
    const double *xa = xs + (32 * wm + r) * kPitch + q, *yb = ys + (32 * wn + r) * kPitch + q;
#pragma unroll
    for (int ks = 0; ks < kNB / 4; ++ks) {
        double a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = xa[16 * t * kPitch + 4 * ks];
            b[t] = yb[16 * t * kPitch + 4 * ks];
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
}

// Register e of accumulator (mi, ni) of wave (wm, wn) holds C[32wm + 16mi + 4e + (lane >> 4)][32wn + 16ni + (lane & 15)].
__device__ __forceinline__ int acc_row(int lane, int wm, int mi, int e) { return 32 * wm + 16 * mi + 4 * e + (lane >> 4); }
__device__ __forceinline__ int acc_col(int lane, int wn, int ni) { return 32 * wn + 16 * ni + (lane & 15); }

__device__ __forceinline__ void zero_acc(f64x4 (&acc)[2][2])
{
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
}

__device__ __forceinline__ void store_acc(double *__restrict__ dst, int64_t ld, int lane, int wm, int wn, const f64x4 (&acc)[2][2])
{
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(int64_t)acc_row(lane, wm, mi, e) * ld + acc_col(lane, wn, ni)] = acc[mi][ni][e];
}

// W ← upper triangle of hd (i ≤ j < k), 1 on the padded diagonal, 0 elsewhere.  Grid (kp / 64, kp / 4), 256 threads = 4 rows × 64 columns.
__global__ __launch_bounds__(256) void factor_init(const double *__restrict__ hd, int64_t K, double *__restrict__ w, int64_t kp,
                                                   int32_t *__restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63), i = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    double v = i == j ? 1.0 : 0.0;
    if (i <= j && j < K) v = hd[i * K + j];
    w[i * kp + j] = v;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *status = 0;
}

// Thread t of the diagonal kernel owns row t >> 2 and the 16 columns (t & 3) + 4m of a 64 × 64 block.
__global__ __launch_bounds__(256) void factor_diag(double *__restrict__ w, int64_t kp, int64_t J, double *__restrict__ vbuf,
                                                   double *__restrict__ vtbuf, int32_t *__restrict__ status)
{
    __shared__ double a[kNB * kDPitch];    // W_JJ, then R_JJ (upper triangle)
    __shared__ double b[kNB * kDPitch];    // the identity, then V_J = R_JJ⁻¹
    const int tid = threadIdx.x, row = tid >> 2, c0 = tid & 3;
    double *blk = w + (J * kNB) * kp + J * kNB;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = tid + 256 * i, r = p >> 6, c = p & 63;
        a[r * kDPitch + c] = blk[(int64_t)r * kp + c];
        b[r * kDPitch + c] = r == c ? 1.0 : 0.0;
    }
    int bad = -1;                          // the largest local index whose pivot failed (the first one met), the same in every thread
    for (int j = kNB - 1; j >= 0; --j) {
        __syncthreads();
        double p = a[j * kDPitch + j];
        if (!(p > 0.0 && p < INFINITY)) {
            if (bad < 0) bad = j;
            p = 1.0;
        }
        const double r = sqrt(p);
        __syncthreads();
        if (tid <= j) a[tid * kDPitch + j] = tid == j ? r : a[tid * kDPitch + j] / r;
        __syncthreads();
        const double rij = a[row * kDPitch + j];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int c = c0 + 4 * m;
            if (row <= c && c < j) a[row * kDPitch + c] = fma(-rij, a[c * kDPitch + j], a[row * kDPitch + c]);
        }
    }
    // R·V = I by rows from the bottom: V[i][·] = B[i][·] / r_ii, then B[t][·] −= r_ti·V[i][·] for t < i (columns ≥ i only: V is upper)
    for (int i = kNB - 1; i >= 0; --i) {
        __syncthreads();
        const double rii = a[i * kDPitch + i];
        if (tid >= i && tid < kNB) b[i * kDPitch + tid] = b[i * kDPitch + tid] / rii;
        __syncthreads();
        const double rti = a[row * kDPitch + i];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int c = c0 + 4 * m;
            if (row < i && c >= i) b[row * kDPitch + c] = fma(-rti, b[i * kDPitch + c], b[row * kDPitch + c]);
        }
    }
    __syncthreads();
    double *v = vbuf + J * kBlk, *vt = vtbuf + J * kBlk;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = tid + 256 * i, r = p >> 6, c = p & 63;
        blk[(int64_t)r * kp + c] = r <= c ? a[r * kDPitch + c] : 0.0;
        v[r * kNB + c] = r <= c ? b[r * kDPitch + c] : 0.0;
        vt[r * kNB + c] = c <= r ? b[c * kDPitch + r] : 0.0;
    }
    if (tid == 0 && bad >= 0 && *status == 0) *status = (int32_t)(J * kNB + bad + 1);
}

// R_IJ = A_IJ·V_Jᵀ, I = blockIdx.x < J, in place.
__global__ __launch_bounds__(256) void factor_panel(double *__restrict__ w, int64_t kp, int64_t J, const double *__restrict__ vbuf)
{
    __shared__ __attribute__((aligned(16))) double xs[kNB * kPitch];
    __shared__ __attribute__((aligned(16))) double ys[kNB * kPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    double *blk = w + ((int64_t)blockIdx.x * kNB) * kp + J * kNB;
    Frag fx, fy;
    load_block(blk, kp, tid, fx);
    load_block(vbuf + J * kBlk, kNB, tid, fy);
    store_block_lds(xs, tid, fx);
    store_block_lds(ys, tid, fy);
    __syncthreads();
    f64x4 acc[2][2];
    zero_acc(acc);
    gemm_step(xs, ys, lane, wm, wn, acc);
    store_acc(blk, kp, lane, wm, wn, acc);
}

// A_IK −= R_IJ·R_KJᵀ for the blocks I ≤ K < J: blockIdx.x = K(K + 1)/2 + I.
__global__ __launch_bounds__(256) void factor_trail(double *__restrict__ w, int64_t kp, int64_t J)
{
    __shared__ __attribute__((aligned(16))) double xs[kNB * kPitch];
    __shared__ __attribute__((aligned(16))) double ys[kNB * kPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t p = blockIdx.x;
    int64_t K = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    if (K * (K + 1) / 2 > p) --K;
    if ((K + 1) * (K + 2) / 2 <= p) ++K;
    const int64_t I = p - K * (K + 1) / 2;
    Frag fx, fy;
    load_block(w + (I * kNB) * kp + J * kNB, kp, tid, fx);
    load_block(w + (K * kNB) * kp + J * kNB, kp, tid, fy);
    double *c = w + (I * kNB) * kp + K * kNB;
    // The product is summed from zero and taken off A_IK once: one rounding at A_IK's magnitude per block step, not one per MFMA
    // (with A_IK as the accumulator's start the residual of U came out 5 times the host route's at k = 520).
    f64x4 old[2][2], acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 4; ++e) old[mi][ni][e] = c[(int64_t)acc_row(lane, wm, mi, e) * kp + acc_col(lane, wn, ni)];
    store_block_lds(xs, tid, fx);
    store_block_lds(ys, tid, fy);
    __syncthreads();
    zero_acc(acc);
    gemm_step(xs, ys, lane, wm, wn, acc);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = old[mi][ni] - acc[mi][ni];
    store_acc(c, kp, lane, wm, wn, acc);
}

// T_JI = U_IJᵀ for J = I + 1 + blockIdx.x: Sᵀ = Σ_{I<K≤J} T_JK·R_IKᵀ (T_JJ = V_Jᵀ), then T_JI = −Sᵀ·V_Iᵀ, into W's block (J, I).
__global__ __launch_bounds__(256) void factor_inverse(double *__restrict__ w, int64_t kp, int64_t I, const double *__restrict__ vbuf,
                                                      const double *__restrict__ vtbuf)
{
    __shared__ __attribute__((aligned(16))) double xs[kNB * kPitch];
    __shared__ __attribute__((aligned(16))) double ys[kNB * kPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t J = I + 1 + blockIdx.x;
    const double *trow = w + (J * kNB) * kp, *rrow = w + (I * kNB) * kp, *vtj = vtbuf + J * kBlk;
    f64x4 acc[2][2];
    zero_acc(acc);
    Frag fx, fy;
    load_block(I + 1 == J ? vtj : trow + (I + 1) * kNB, I + 1 == J ? kNB : kp, tid, fx);
    load_block(rrow + (I + 1) * kNB, kp, tid, fy);
    for (int64_t K = I + 1; K <= J; ++K) {
        __syncthreads();                   // the previous step's reads of xs / ys are done
        store_block_lds(xs, tid, fx);
        store_block_lds(ys, tid, fy);
        __syncthreads();
        if (K < J) {
            load_block(K + 1 == J ? vtj : trow + (K + 1) * kNB, K + 1 == J ? kNB : kp, tid, fx);
            load_block(rrow + (K + 1) * kNB, kp, tid, fy);
        }
        gemm_step(xs, ys, lane, wm, wn, acc);
    }
    load_block(vbuf + I * kBlk, kNB, tid, fy);
    __syncthreads();
    store_block_lds(ys, tid, fy);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 4; ++e) xs[acc_row(lane, wm, mi, e) * kPitch + acc_col(lane, wn, ni)] = acc[mi][ni][e];
    __syncthreads();
    zero_acc(acc);
    gemm_step(xs, ys, lane, wm, wn, acc);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = -acc[mi][ni];
    store_acc(w + (J * kNB) * kp + I * kNB, kp, lane, wm, wn, acc);
}

// u's block (bi, bj) = (blockIdx.y, blockIdx.x): zeros below the diagonal, V on it, T's block (bj, bi) transposed above it.
__global__ __launch_bounds__(256) void factor_emit(const double *__restrict__ w, int64_t kp, const double *__restrict__ vbuf, int64_t K,
                                                   double *__restrict__ u)
{
    __shared__ double t[kNB * kDPitch];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.y, bj = blockIdx.x;
    if (bi < bj) {
        const double *src = w + (bj * kNB) * kp + bi * kNB;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = tid + 256 * i, r = p >> 6, c = p & 63;
            t[c * kDPitch + r] = src[(int64_t)r * kp + c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = tid + 256 * i, r = p >> 6, c = p & 63;
        const int64_t gi = bi * kNB + r, gj = bj * kNB + c;
        if (gi >= K || gj >= K) continue;
        u[gi * K + gj] = bi > bj ? 0.0 : (bi == bj ? vbuf[bi * kBlk + r * kNB + c] : t[r * kDPitch + c]);
    }
}

constexpr int64_t kMaxK = (int64_t)1 << 17;

} // namespace
} // namespace mtq

using namespace mtq;

extern "C" size_t mtq_gptq_factor_scratch_doubles(int64_t k)
{
    if (k <= 0 || k > kMaxK) return 0;
    const size_t nb = (size_t)((k + kNB - 1) / kNB);
    return nb * kNB * nb * kNB + 2 * nb * kBlk;
}

extern "C" int mtq_gptq_factor(const double *hd, int64_t k, double *u, size_t u_doubles, int32_t *status, double *scratch, size_t scratch_doubles,
                               void *stream)
{
    if (!hd || !u || !status || !scratch) return fail(MTQ_ERR_INVALID, "null argument");
    if (k <= 0) return fail(MTQ_ERR_INVALID, "k must be positive");
    if (k > kMaxK) return fail(MTQ_ERR_INVALID, "matrix too large");
    if (u_doubles != (size_t)k * (size_t)k) return fail(MTQ_ERR_INVALID, "u_doubles != k * k");
    if (scratch_doubles < mtq_gptq_factor_scratch_doubles(k)) return fail(MTQ_ERR_INVALID, "scratch smaller than mtq_gptq_factor_scratch_doubles(k)");
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(MTQ_ERR_INVALID, "scratch must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    const int64_t nb = (k + kNB - 1) / kNB, kp = nb * kNB;
    double *w = scratch, *vbuf = scratch + kp * kp, *vtbuf = vbuf + nb * kBlk;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(factor_init, dim3((unsigned)nb, (unsigned)(kp / 4)), dim3(256), 0, st, hd, k, w, kp, status);
    if (int rc = check_launch("mtq_gptq_factor (init)")) return rc;
    for (int64_t J = nb - 1; J >= 0; --J) {
        hipLaunchKernelGGL(factor_diag, dim3(1), dim3(256), 0, st, w, kp, J, vbuf, vtbuf, status);
        if (int rc = check_launch("mtq_gptq_factor (diagonal block)")) return rc;
        if (J == 0) break;
        hipLaunchKernelGGL(factor_panel, dim3((unsigned)J), dim3(256), 0, st, w, kp, J, vbuf);
        if (int rc = check_launch("mtq_gptq_factor (panel)")) return rc;
        hipLaunchKernelGGL(factor_trail, dim3((unsigned)(J * (J + 1) / 2)), dim3(256), 0, st, w, kp, J);
        if (int rc = check_launch("mtq_gptq_factor (trailing update)")) return rc;
    }
    for (int64_t I = nb - 2; I >= 0; --I) {
        hipLaunchKernelGGL(factor_inverse, dim3((unsigned)(nb - 1 - I)), dim3(256), 0, st, w, kp, I, vbuf, vtbuf);
        if (int rc = check_launch("mtq_gptq_factor (inverse)")) return rc;
    }
    hipLaunchKernelGGL(factor_emit, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, st, w, kp, vbuf, k, u);
    return check_launch("mtq_gptq_factor (emit)");
}
