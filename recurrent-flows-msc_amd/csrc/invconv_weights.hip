// InvConv.get_weight for the K steps of a flow level, forward and backward, one launch each way (gfx950).
// Called by rfn_hip.ops (the level nodes of the Glow flow).
#include "common.h"
#include "../../include/rfn_hip.h"

// ------------------------------------------------------------------------------------------------ InvConv.get_weight
// Flow/glow_modules.py:178-207 for the K steps of a flow level in one launch each way (the reference -- and a torch
// restatement -- spends ~17 launches per level forward and ~20 backward on this C x C algebra):
//   Lm = lower o tril(-1) + I,   Um = upper o triu(+1) + diag(sign_s * exp(log_s)),   W = P Lm Um,
//   dlogdet = HW * sum(log_s)  (summed over the K steps, in step order, into ONE scalar that is WRITTEN: no atomics).
// Backward, given gW and the gradient gc of the scalar:  gT = P^T gW;  g_lower = (gT Um^T) o tril(-1);
//   g_upper = (Lm^T gT) o triu(+1);  g_log_s = diag(Lm^T gT) * sign_s * exp(log_s) + gc * HW.
// One workgroup per step, the three matrices in LDS (C <= RFN_INVCONV_MAX_CHANNELS).  Parameters arrive as pointer arrays in the kernel
// arguments (no stacking copies): K <= RFN_INVCONV_MAX_STEPS.
struct InvConvWeightsParams {
    const float* p[RFN_INVCONV_MAX_STEPS];
    const float* lower[RFN_INVCONV_MAX_STEPS];
    const float* upper[RFN_INVCONV_MAX_STEPS];
    const float* log_s[RFN_INVCONV_MAX_STEPS];
    const float* sign_s[RFN_INVCONV_MAX_STEPS];
    float* W;            // [K][C][C]
    float* logdet;       // scalar, written
    const float* gW;     // backward: [K][C][C]
    const float* gc;     // backward: gradient of the scalar (may be null)
    float* g_lower;      // [K][C][C]
    float* g_upper;      // [K][C][C]
    float* g_log_s;      // [K][C]
    int C;
    float hw;
};
// LDS matrices have row stride C + 1: column walks (transposed operands) are bank-conflict free
__device__ __forceinline__ void invconv_load_LU(const InvConvWeightsParams& q, int k, float* Lm, float* Um) {
    const int C = q.C, CP = C + 1;
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
        const int r = i / C, c = i - r * C;
        Lm[r * CP + c] = r > c ? q.lower[k][i] : (r == c ? 1.f : 0.f);
        Um[r * CP + c] = r < c ? q.upper[k][i] : (r == c ? q.sign_s[k][r] * expf(q.log_s[k][r]) : 0.f);
    }
}
__device__ __forceinline__ void invconv_load(const float* __restrict__ src, float* dst, int C) {
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) dst[(i / C) * (C + 1) + i % C] = src[i];
}
// out(r, c) = sum_j A(r, j) * B(j, c) for the C x C matrices in LDS (row stride C + 1), each thread a 4 x 4 block of the
// result (8 LDS reads per 16 multiply-adds); TA / TB: the operand is read transposed.  C % 4 == 0 or the scalar tail runs.
template <bool TA, bool TB, typename Store>
__device__ __forceinline__ void invconv_mm(const float* __restrict__ A, const float* __restrict__ B, int C, Store store) {
    const int CP = C + 1, nb = C >> 2;
    for (int blk = threadIdx.x; blk < nb * nb; blk += blockDim.x) {
        const int r0 = (blk / nb) * 4, c0 = (blk % nb) * 4;
        float acc[4][4] = {};
        for (int j = 0; j < C; ++j) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = TA ? A[j * CP + r0 + i] : A[(r0 + i) * CP + j];
                bv[i] = TB ? B[(c0 + i) * CP + j] : B[j * CP + c0 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[i][k] = fmaf(av[i], bv[k], acc[i][k]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) store(r0 + i, c0 + k, acc[i][k]);
    }
    const int Cm = nb * 4;  // ragged edge (C % 4 != 0): the last rows and columns one element at a time
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
        const int r = i / C, c = i - r * C;
        if (r < Cm && c < Cm) continue;
        float a = 0.f;
        for (int j = 0; j < C; ++j)
            a = fmaf(TA ? A[j * CP + r] : A[r * CP + j], TB ? B[c * CP + j] : B[j * CP + c], a);
        store(r, c, a);
    }
}
__global__ __launch_bounds__(256) void invconv_weights_fwd_kernel(const InvConvWeightsParams q) {
    extern __shared__ float sm_iw[];
    const int C = q.C, CP = C + 1, k = blockIdx.x;
    float* B0 = sm_iw;            // Lm, then P
    float* B1 = B0 + C * CP;      // Um
    float* B2 = B1 + C * CP;      // T = Lm Um
    invconv_load_LU(q, k, B0, B1);
    __syncthreads();
    invconv_mm<false, false>(B0, B1, C, [&](int r, int c, float v) { B2[r * CP + c] = v; });
    __syncthreads();
    invconv_load(q.p[k], B0, C);
    __syncthreads();
    float* W = q.W + (long)k * C * C;
    invconv_mm<false, false>(B0, B2, C, [&](int r, int c, float v) { W[r * C + c] = v; });  // W = P T
    if (k == 0 && threadIdx.x < 64) {  // one wave of ONE block: HW * sum over the steps (in order) of sum(log_s): no atomics
        float tot = 0.f;
        for (int kk = 0; kk < (int)gridDim.x; ++kk) {
            float v = 0.f;
            for (int c = threadIdx.x; c < C; c += 64) v += q.log_s[kk][c];
            tot += wave_sum(v) * q.hw;
        }
        if (threadIdx.x == 0) *q.logdet = tot;
    }
}
__global__ __launch_bounds__(256) void invconv_weights_bwd_kernel(const InvConvWeightsParams q) {
    extern __shared__ float sm_iw[];
    const int C = q.C, CP = C + 1, k = blockIdx.x;
    float* B0 = sm_iw;            // P, then Lm
    float* B1 = B0 + C * CP;      // gW, then Um
    float* B2 = B1 + C * CP;      // gT = P^T gW
    invconv_load(q.p[k], B0, C);
    invconv_load(q.gW + (long)k * C * C, B1, C);
    __syncthreads();
    invconv_mm<true, false>(B0, B1, C, [&](int r, int c, float v) { B2[r * CP + c] = v; });
    __syncthreads();
    invconv_load_LU(q, k, B0, B1);
    __syncthreads();
    const float* Um = B1;
    const float gc = q.gc ? q.gc[0] * q.hw : 0.f;
    float* gl = q.g_lower + (long)k * C * C;
    float* gu = q.g_upper + (long)k * C * C;
    float* gs = q.g_log_s + (long)k * C;
    // g_lower = (gT Um^T) o tril(-1);  g_upper = (Lm^T gT) o triu(+1);  g_log_s from the diagonal of Lm^T gT
    invconv_mm<false, true>(B2, B1, C, [&](int r, int c, float v) { gl[r * C + c] = r > c ? v : 0.f; });
    invconv_mm<true, false>(B0, B2, C, [&](int r, int c, float v) {
        gu[r * C + c] = r < c ? v : 0.f;
        if (r == c) gs[r] = v * Um[r * CP + r] + gc;
    });
}
static int invconv_weights_fill(InvConvWeightsParams& q, const float* const* p, const float* const* lower,
                                const float* const* upper, const float* const* log_s, const float* const* sign_s, int K,
                                int C, int HW) {
    if (!(p && lower && upper && log_s && sign_s && K >= 1 && K <= RFN_INVCONV_MAX_STEPS && C >= 1 &&
          C <= RFN_INVCONV_MAX_CHANNELS && HW > 0))
        return -1;
    memset(&q, 0, sizeof(q));
    for (int k = 0; k < K; ++k) {
        if (!(p[k] && lower[k] && upper[k] && log_s[k] && sign_s[k])) return -2;
        q.p[k] = p[k]; q.lower[k] = lower[k]; q.upper[k] = upper[k]; q.log_s[k] = log_s[k]; q.sign_s[k] = sign_s[k];
    }
    q.C = C;
    q.hw = (float)HW;
    return 0;
}
extern "C" int rfn_invconv_weights_fwd_f32(const float* const* p, const float* const* lower, const float* const* upper,
                                           const float* const* log_s, const float* const* sign_s, float* W, float* logdet,
                                           int K, int C, int HW, rfn_stream_t stream) {
    InvConvWeightsParams q;
    int rc = invconv_weights_fill(q, p, lower, upper, log_s, sign_s, K, C, HW);
    if (rc || !W || !logdet) {
        rfn_set_error("rfn_invconv_weights_fwd_f32: argument check failed (%d)", rc ? rc : -3);
        return rc ? rc : -3;
    }
    q.W = W;
    q.logdet = logdet;
    if (C > 64)  // three padded C x C matrices: 112 KB at C = 96 (the LDS of a CU is 160 KB)
        (void)hipFuncSetAttribute((const void*)invconv_weights_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  3 * C * (C + 1) * (int)sizeof(float));
    hipLaunchKernelGGL(invconv_weights_fwd_kernel, dim3(K), dim3(256), (size_t)3 * C * (C + 1) * sizeof(float),
                       (hipStream_t)stream, q);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_invconv_weights_bwd_f32(const float* const* p, const float* const* lower, const float* const* upper,
                                           const float* const* log_s, const float* const* sign_s, const float* gW,
                                           const float* gc, float* g_lower, float* g_upper, float* g_log_s, int K, int C,
                                           int HW, rfn_stream_t stream) {
    InvConvWeightsParams q;
    int rc = invconv_weights_fill(q, p, lower, upper, log_s, sign_s, K, C, HW);
    if (rc || !gW || !g_lower || !g_upper || !g_log_s) {
        rfn_set_error("rfn_invconv_weights_bwd_f32: argument check failed (%d)", rc ? rc : -3);
        return rc ? rc : -3;
    }
    q.gW = gW; q.gc = gc; q.g_lower = g_lower; q.g_upper = g_upper; q.g_log_s = g_log_s;
    if (C > 64)
        (void)hipFuncSetAttribute((const void*)invconv_weights_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  3 * C * (C + 1) * (int)sizeof(float));
    hipLaunchKernelGGL(invconv_weights_bwd_kernel, dim3(K), dim3(256), (size_t)3 * C * (C + 1) * sizeof(float),
                       (hipStream_t)stream, q);
    RFN_LAUNCH_CHECK();
    return 0;
}
