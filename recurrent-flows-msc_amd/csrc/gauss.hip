// Diagonal Gaussian log-prob, its backward, and sampling with a scalar or a per-row temperature (gfx950): HBM-bound
// streaming kernels.  Called by rfn_hip.ops (the flow priors and the temperature sweep of the evaluation driver).
#include "common.h"
#include "../../include/rfn_hip.h"

// ------------------------------------------------------------------------------------------------ gaussian log-prob
#define RFN_HALF_LOG_2PI 0.91893853320467274178f

__device__ __forceinline__ void gauss_params(const float* on, int layout, int c, int Cz, int HW, int p, float& mean,
                                             float& raw) {
    if (layout == 0) {
        mean = on[(long)(2 * c) * HW + p];
        raw = on[(long)(2 * c + 1) * HW + p];
    } else {
        mean = on[(long)c * HW + p];
        raw = on[(long)(Cz + c) * HW + p];
    }
}

__global__ __launch_bounds__(256) void gauss_logp_kernel(const float* __restrict__ z, long z_ns,
                                                         const float* __restrict__ o, long o_ns,
                                                         float* __restrict__ logp, int layout, int std_mode, int Cz,
                                                         int HW) {
    __shared__ float sm[4];
    const int n = blockIdx.x;
    const float* zn = z + n * z_ns;
    const float* on = o + n * o_ns;
    float acc = 0.f;
    for (int e = threadIdx.x; e < Cz * HW; e += 256) {
        int c = e / HW, p = e - c * HW;
        float mean, raw;
        gauss_params(on, layout, c, Cz, HW, p, mean, raw);
        float logstd, std;
        if (std_mode == 0) {
            std = softplusf_(raw) + 1e-8f;
            logstd = logf(std);
        } else {
            std = expf(raw);
            logstd = raw;
        }
        float d = zn[e] - mean;
        acc += -(d * d) / (2.f * std * std) - logstd - RFN_HALF_LOG_2PI;
    }
    float tot = block_sum_256(acc, sm);
    if (threadIdx.x == 0) logp[n] += tot;
}
extern "C" int rfn_gauss_logp_f32(const float* z, long z_ns, const float* o, long o_ns, float* logp, int layout,
                                  int std_mode, int N, int Cz, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(z && o && logp && N >= 0 && Cz > 0 && HW > 0, -1);
    if (N == 0) return 0;
    hipLaunchKernelGGL(gauss_logp_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, z, z_ns, o, o_ns, logp, layout,
                       std_mode, Cz, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void gauss_logp_bwd_kernel(const float* __restrict__ z, long z_ns,
                                                             const float* __restrict__ o, long o_ns,
                                                             const float* __restrict__ glogp, float* __restrict__ gz,
                                                             long gz_ns, float* __restrict__ go, long go_ns, int layout,
                                                             int std_mode, int Cz, int HW) {
    const int n = blockIdx.x;
    const float* zn = z + n * z_ns;
    const float* on = o + n * o_ns;
    float* gzn = gz + n * gz_ns;
    float* gon = go + n * go_ns;
    const float g = glogp[n];
    for (int e = threadIdx.x; e < Cz * HW; e += 256) {
        int c = e / HW, p = e - c * HW;
        float mean, raw;
        gauss_params(on, layout, c, Cz, HW, p, mean, raw);
        float std, dstd_draw;
        if (std_mode == 0) {
            std = softplusf_(raw) + 1e-8f;
            dstd_draw = raw > 20.f ? 1.f : 1.f / (1.f + expf(-raw));
        } else {
            std = expf(raw);
            dstd_draw = std;
        }
        float d = zn[e] - mean;
        float inv = 1.f / (std * std);
        float gzv = -d * inv * g;                        // d logp / d z
        float gstd = (d * d * inv / std - 1.f / std) * g;  // d logp / d std
        gzn[e] = gzv;
        if (layout == 0) {
            gon[(long)(2 * c) * HW + p] = -gzv;
            gon[(long)(2 * c + 1) * HW + p] = gstd * dstd_draw;
        } else {
            gon[(long)c * HW + p] = -gzv;
            gon[(long)(Cz + c) * HW + p] = gstd * dstd_draw;
        }
    }
}
extern "C" int rfn_gauss_logp_bwd_f32(const float* z, long z_ns, const float* o, long o_ns, const float* glogp,
                                      float* gz, long gz_ns, float* go, long go_ns, int layout, int std_mode, int N,
                                      int Cz, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(z && o && glogp && gz && go && N >= 0 && Cz > 0 && HW > 0, -1);
    if (N == 0) return 0;
    hipLaunchKernelGGL(gauss_logp_bwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, z, z_ns, o, o_ns, glogp, gz,
                       gz_ns, go, go_ns, layout, std_mode, Cz, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}

// temperature_rows (may be null): one temperature per frame, uniform per block; null: the scalar for every frame.  One
// kernel for both, so a vector filled with the scalar's value gives the scalar call's bits.
__global__ __launch_bounds__(256) void gauss_sample_kernel(const float* __restrict__ o, long o_ns,
                                                           const float* __restrict__ eps, float* __restrict__ z,
                                                           long z_ns, float temperature,
                                                           const float* __restrict__ temperature_rows, int layout,
                                                           int std_mode, int Cz, int HW) {
    const int n = blockIdx.x;
    const float* on = o + n * o_ns;
    const float t = temperature_rows ? temperature_rows[n] : temperature;
    for (int e = threadIdx.x; e < Cz * HW; e += 256) {
        int c = e / HW, p = e - c * HW;
        float mean, raw;
        gauss_params(on, layout, c, Cz, HW, p, mean, raw);
        float std = std_mode == 0 ? softplusf_(raw) + 1e-8f : expf(raw);
        z[n * z_ns + e] = mean + std * t * eps[(long)n * Cz * HW + e];
    }
}
extern "C" int rfn_gauss_sample_f32(const float* o, long o_ns, const float* eps, float* z, long z_ns, float temperature,
                                    int layout, int std_mode, int N, int Cz, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(o && eps && z && N >= 0 && Cz > 0 && HW > 0, -1);
    if (N == 0) return 0;
    hipLaunchKernelGGL(gauss_sample_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, o, o_ns, eps, z, z_ns,
                       temperature, (const float*)nullptr, layout, std_mode, Cz, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_gauss_sample_rows_f32(const float* o, long o_ns, const float* eps, float* z, long z_ns,
                                         const float* temperature_rows, int layout, int std_mode, int N, int Cz,
                                         int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(o && eps && z && temperature_rows && N >= 0 && Cz > 0 && HW > 0, -1);
    if (N == 0) return 0;
    hipLaunchKernelGGL(gauss_sample_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, o, o_ns, eps, z, z_ns, 0.0f,
                       temperature_rows, layout, std_mode, Cz, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}
