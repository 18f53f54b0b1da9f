// Row-summed pixel log-likelihoods of the baselines' importance-weighted bound (VRNN/VRNN.py:400-415, SVG/SVG.py:344-385,
// SRNN/SRNN.py:482-579 of the reference): the K*B decoder rows of a time step against its B frames in ONE pass, in place
// of `x.repeat(K, ...)`, a torch.distributions log_prob chain and a reduction; and the two row-summed Normal(mu,
// exp(logvar / 2)) densities of one inner sample of SVG's bound in one launch.  Forward only: evaluation kernels.
//
// Arithmetic: a term's additions, products and squares run in fp64 on the fp32 inputs (exact differences, no cancellation
// error), the logs of "bernoulli" are the accurate fp32 logf / log1pf, and the term is rounded to fp32 ONCE; the terms
// are then added in fp32 in the fixed order written in include/rfn_hip.h.  No fast intrinsics, no atomics, no LDS
// traffic besides the four wave sums of a row.
#include "common.h"
#include "../../include/rfn_hip.h"

// every operation below rounds on its own: the 16-byte and the single-float paths give the same bits
#pragma clang fp contract(off)

constexpr int RFN_PL_THREADS = 256;            // one workgroup per row
constexpr int RFN_PL_MAX_BLOCKS = 1 << 16;     // rows beyond that are taken by the grid-stride loop
constexpr double RFN_PL_HALF_LOG_2PI = 0.91893853320467274178;
constexpr float RFN_PL_EPS = 1.1920928955078125e-07f;   // 2^-23: the clamp of torch.distributions' probs

// One term from the decoder's value p and the target xd (the frame's value, plus the row's noise when there is one, added
// in fp64: exact, the dequantised target is never rounded on its own).  c0 / c1 of "gaussian": -log(sigma) - log(2 pi) / 2
// and 1 / (2 sigma^2), in fp64.
template <int MODE>
__device__ __forceinline__ float pl_term(float p, double xd, double c0, double c1) {
    if (MODE == RFN_PIXEL_LOGLIK_BERNOULLI) {
        const float pc = fminf(fmaxf(p, RFN_PL_EPS), 1.f - RFN_PL_EPS);
        const double a = (double)logf(pc), b = (double)log1pf(-pc);
        return (float)(xd * a + (1.0 - xd) * b);
    } else if (MODE == RFN_PIXEL_LOGLIK_GAUSSIAN) {
        const double d = xd - (double)p;
        return (float)(c0 - d * d * c1);
    } else {
        const double d = (double)p - xd;
        return (float)(-(d * d));
    }
}

template <int MODE, bool NOISE>
__device__ __forceinline__ float pl_term_n(float p, float x, float u, double c0, double c1) {
    return pl_term<MODE>(p, NOISE ? (double)x + (double)u : (double)x, c0, c1);
}

// Row r: lane t takes the groups g = t, t + 256, ... of four consecutive elements and adds their terms in element
// order; VEC reads a group as one 16-byte load per operand when all three row bases allow it (chosen per row,
// workgroup-uniform), else as single floats.  The last group may be short.
template <int MODE, bool NOISE>
__global__ void __launch_bounds__(RFN_PL_THREADS)
pixel_loglik_kernel(const float* __restrict__ pred, const float* __restrict__ target, long target_stride,
                    const float* __restrict__ noise, float* __restrict__ out, long R, int B, long N, double c0,
                    double c1) {
    __shared__ float sm[RFN_PL_THREADS / 64];
    const int tid = threadIdx.x;
    const long full = N >> 2;                  // groups of four whole elements
    const long groups = (N + 3) >> 2;
    for (long r = blockIdx.x; r < R; r += gridDim.x) {
        const float* pr = pred + r * N;
        const float* xr = target + (r % B) * target_stride;
        const float* ur = NOISE ? noise + r * N : nullptr;
        const bool vec = ((((uintptr_t)pr) | ((uintptr_t)xr) | (NOISE ? (uintptr_t)ur : 0)) & 15) == 0;
        float s = 0.f;
        if (vec) {
#pragma unroll 4
            for (long g = tid; g < full; g += RFN_PL_THREADS) {
                const float4 p = reinterpret_cast<const float4*>(pr)[g];
                const float4 x = reinterpret_cast<const float4*>(xr)[g];
                float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
                if (NOISE) u = reinterpret_cast<const float4*>(ur)[g];
                s += pl_term_n<MODE, NOISE>(p.x, x.x, u.x, c0, c1);
                s += pl_term_n<MODE, NOISE>(p.y, x.y, u.y, c0, c1);
                s += pl_term_n<MODE, NOISE>(p.z, x.z, u.z, c0, c1);
                s += pl_term_n<MODE, NOISE>(p.w, x.w, u.w, c0, c1);
            }
        } else {
#pragma unroll 4
            for (long g = tid; g < full; g += RFN_PL_THREADS) {
                const long i = g << 2;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    s += pl_term_n<MODE, NOISE>(pr[i + e], xr[i + e], NOISE ? ur[i + e] : 0.f, c0, c1);
            }
        }
        // the short last group, in its place in the lane's sequence: group `full` belongs to lane full % 256 and comes
        // after all of that lane's whole groups
        if (groups > full && (int)(full % RFN_PL_THREADS) == tid) {
            for (long i = full << 2; i < N; ++i)
                s += pl_term_n<MODE, NOISE>(pr[i], xr[i], NOISE ? ur[i] : 0.f, c0, c1);
        }
        s = wave_sum(s);
        __syncthreads();                        // the previous row's sums have been read
        if ((tid & 63) == 0) sm[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) out[r] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    }
}

template <int MODE>
static void pl_launch(const float* pred, const float* target, long target_stride, const float* noise, float* out, long R,
                      int B, long N, double c0, double c1, hipStream_t s) {
    const dim3 grid((unsigned)(R < RFN_PL_MAX_BLOCKS ? R : RFN_PL_MAX_BLOCKS));
    if (noise)
        hipLaunchKernelGGL((pixel_loglik_kernel<MODE, true>), grid, dim3(RFN_PL_THREADS), 0, s, pred, target,
                           target_stride, noise, out, R, B, N, c0, c1);
    else
        hipLaunchKernelGGL((pixel_loglik_kernel<MODE, false>), grid, dim3(RFN_PL_THREADS), 0, s, pred, target,
                           target_stride, noise, out, R, B, N, c0, c1);
}

extern "C" int rfn_pixel_loglik_f32(const float* pred, const float* target, long target_stride, const float* noise,
                                    float* out, long R, int B, long N, int mode, double scale, rfn_stream_t stream) {
    RFN_CHECK_ARG(R >= 0 && R <= 2147483647L && B >= 1 && N >= 1, -1);
    RFN_CHECK_ARG(R % B == 0, -1);
    RFN_CHECK_ARG(target_stride >= N, -1);
    RFN_CHECK_ARG(mode == RFN_PIXEL_LOGLIK_BERNOULLI || mode == RFN_PIXEL_LOGLIK_GAUSSIAN || mode == RFN_PIXEL_LOGLIK_MSE,
                  -2);
    RFN_CHECK_ARG(mode != RFN_PIXEL_LOGLIK_GAUSSIAN || (scale > 0.0 && scale <= 3.4028234663852886e38), -3);
    if (R == 0) return 0;
    RFN_CHECK_ARG(pred && target && out, -4);
    RFN_CHECK_ARG(((((uintptr_t)pred) | ((uintptr_t)target) | ((uintptr_t)noise) | ((uintptr_t)out)) & 3) == 0, -4);
    hipStream_t s = (hipStream_t)stream;
    if (mode == RFN_PIXEL_LOGLIK_BERNOULLI) {
        pl_launch<RFN_PIXEL_LOGLIK_BERNOULLI>(pred, target, target_stride, noise, out, R, B, N, 0.0, 0.0, s);
    } else if (mode == RFN_PIXEL_LOGLIK_GAUSSIAN) {
        const double c0 = -log(scale) - RFN_PL_HALF_LOG_2PI, c1 = 1.0 / (2.0 * scale * scale);
        pl_launch<RFN_PIXEL_LOGLIK_GAUSSIAN>(pred, target, target_stride, noise, out, R, B, N, c0, c1, s);
    } else {
        pl_launch<RFN_PIXEL_LOGLIK_MSE>(pred, target, target_stride, noise, out, R, B, N, 0.0, 0.0, s);
    }
    RFN_LAUNCH_CHECK();
    return 0;
}

// ---- two row-summed densities of N(mu, exp(logvar / 2)) at z: one wavefront per row and distribution
constexpr int RFN_NLP_ROWS = 4;   // waves per workgroup

__device__ __forceinline__ float nlp_term(float mu, float logvar, float z) {
    const double d = (double)z - (double)mu, lv = (double)logvar;
    return (float)(-0.5 * lv - d * d * exp(-lv) * 0.5 - RFN_PL_HALF_LOG_2PI);
}

__global__ void __launch_bounds__(64 * RFN_NLP_ROWS)
normal_logvar_pair_kernel(const float* __restrict__ mu_a, const float* __restrict__ logvar_a, const float* __restrict__ z_a,
                          const float* __restrict__ mu_b, const float* __restrict__ logvar_b, const float* __restrict__ z_b,
                          float* __restrict__ out_a, float* __restrict__ out_b, int B, int Z) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * RFN_NLP_ROWS + (threadIdx.x >> 6);   // wave w: row w % B of pair member w / B
    if (w >= 2L * B) return;                                                  // whole waves leave
    const bool second = w >= B;
    const long b = second ? w - B : w;
    const float* mu = (second ? mu_b : mu_a) + b * Z;
    const float* lv = (second ? logvar_b : logvar_a) + b * Z;
    const float* z = (second ? z_b : z_a) + b * Z;
    float s = 0.f;
    for (int j = lane; j < Z; j += 64) s += nlp_term(mu[j], lv[j], z[j]);
    s = wave_sum(s);
    if (lane == 0) (second ? out_b : out_a)[b] = s;
}

extern "C" int rfn_normal_logvar_pair_f32(const float* mu_a, const float* logvar_a, const float* z_a, const float* mu_b,
                                          const float* logvar_b, const float* z_b, float* out_a, float* out_b, int B,
                                          int Z, rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 1 && Z >= 1 && B <= (1 << 30), -1);
    RFN_CHECK_ARG(mu_a && logvar_a && z_a && mu_b && logvar_b && z_b && out_a && out_b, -2);
    hipLaunchKernelGGL(normal_logvar_pair_kernel, dim3((unsigned)ceil_div(2L * B, RFN_NLP_ROWS)), dim3(64 * RFN_NLP_ROWS),
                       0, (hipStream_t)stream, mu_a, logvar_a, z_a, mu_b, logvar_b, z_b, out_a, out_b, B, Z);
    RFN_LAUNCH_CHECK();
    return 0;
}
