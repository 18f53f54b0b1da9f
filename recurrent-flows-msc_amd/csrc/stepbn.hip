// Per-step BatchNorm + activation, plain and with the 2x2 max-pool folded in, forward and backward (gfx950): the
// BatchNorm layers of the VGG extractor and the upscaler, time-batched.  Called by rfn_hip.ops (StepBatchNormActFn,
// StepBatchNormActPoolFn).
#include "common.h"
#include "../../include/rfn_hip.h"

// ------------------------------------------------------------------------------------------------ per-step BatchNorm
// The reference runs its VGG extractor / upscaler once per timestep (RFN_new.py:126-128,191-194), so every BatchNorm
// sees the B samples of ONE step.  Time-batched here: x is [S*B, C, HW] step-major and the statistics are per (step,
// channel) over (B, HW).  Four kernels replace the permute-copy / batch_norm / permute-copy / activation chain (and its
// backward): statistics (two-pass, second pass from L2), apply + activation, backward reduction, backward apply.
// act: 0 none, 1 relu, 2 leaky_relu(slope), 3 tanh.
__device__ __forceinline__ float stepbn_act(float u, int act, float slope) {
    if (act == 1) return u > 0.f ? u : 0.f;
    if (act == 2) return u > 0.f ? u : slope * u;
    if (act == 3) return tanhf(u);
    return u;
}
__device__ __forceinline__ float stepbn_dact(float u, int act, float slope) {  // from the activation's INPUT u = xhat*g + b
    if (act == 1) return u > 0.f ? 1.f : 0.f;                                  // (recomputed: saves a pass over y)
    if (act == 2) return u > 0.f ? 1.f : slope;
    if (act == 3) {
        const float t = tanhf(u);
        return 1.f - t * t;
    }
    return 1.f;
}
// block (sc, j) = frames j, j+gridDim.y, ... of one (step, channel): shifted sums s1 = sum(x-K), s2 = sum((x-K)^2) with
// K = the pair's first element (keeps the one-pass variance well conditioned).  Every block stores ITS partial pair at
// acc[j][sc][2] (no atomics, nothing to zero, deterministic); the consumers add the gridDim.y <= STEPBN_MAX_SPLIT partials.
constexpr int STEPBN_MAX_SPLIT = 16;
static int stepbn_split(int S, int B, int C) {  // workgroups per (step, channel): enough blocks for the chip, <= B
    int ny = 2048 / (S * C);
    if (ny > STEPBN_MAX_SPLIT) ny = STEPBN_MAX_SPLIT;
    if (ny > B) ny = B;
    return ny < 1 ? 1 : ny;
}
__global__ __launch_bounds__(256) void stepbn_stats_kernel(const float* __restrict__ x, float* __restrict__ acc, int B,
                                                           int C, int HW) {
    __shared__ float sm[4];
    const int s = blockIdx.x / C, c = blockIdx.x - s * C;
    const float* base = x + ((long)s * B * C + c) * HW;
    const long fs = (long)C * HW;
    const float K = base[0];
    float a = 0.f, v = 0.f;
    if ((HW & 3) == 0 && (((uintptr_t)x) & 15) == 0) {  // 16-byte loads (frames and channel planes stay aligned)
        // (frame, pixel quad) pairs of this block flattened over the threads: small maps keep all 256 lanes busy
        const int HW4 = HW >> 2, nb = (B - (int)blockIdx.y + (int)gridDim.y - 1) / (int)gridDim.y;
        for (int idx = threadIdx.x; idx < nb * HW4; idx += 256) {
            const int bi = idx / HW4, p = idx - bi * HW4;
            const float4 q = reinterpret_cast<const float4*>(base + (blockIdx.y + (long)bi * gridDim.y) * fs)[p];
            const float d0 = q.x - K, d1 = q.y - K, d2 = q.z - K, d3 = q.w - K;
            a += (d0 + d1) + (d2 + d3);
            v = fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, fmaf(d3, d3, v))));
        }
    } else {
        for (int b = blockIdx.y; b < B; b += gridDim.y) {
            const float* row = base + b * fs;
            for (int p = threadIdx.x; p < HW; p += 256) {
                const float d = row[p] - K;
                a += d;
                v = fmaf(d, d, v);
            }
        }
    }
    const float ta = block_sum_256(a, sm);
    const float tv = block_sum_256(v, sm);
    if (threadIdx.x == 0) {
        float* dst = acc + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        dst[0] = ta;
        dst[1] = tv;
    }
}
// elementwise kernels: VEC = 4 consecutive pixels per thread when HW % 4 == 0 (16-byte accesses); 32-bit index math
// (the host checks total < 2^31).  The statistics come straight from the stats kernel's partial sums (no finalize launch);
// ONE extra workgroup (the first: dispatched first, so no streaming block is delayed by it) writes mean / var for the
// backward and applies the S running-statistics updates of the step-wise calls in closed form.
struct StepBnFused {
    const float* acc;      // [ny][S*C][2] partial shifted sums of stepbn_stats_kernel
    float* mean_out;
    float* var_out;
    float* run_mean;       // optional [C]: r <- decay r + sum_s coef[s] mean[s]   (and var with coef_u)
    float* run_var;
    const float* coef;
    const float* coef_u;
    float decay;
    long long* nbt;        // optional: += S
    int S, ny;
};
__device__ __forceinline__ void stepbn_moments(const float* __restrict__ x, const float* __restrict__ acc, int sc, int s,
                                               int c, int B, int C, int HW, int ny, int SC, float& m, float& v) {
    if (!acc) return;   // statistics given by the caller (m, v preloaded): synchronised BatchNorm
    const float K = x[((long)s * B * C + c) * HW];
    const float n = (float)B * HW;
    float s1 = 0.f, s2 = 0.f;
    for (int y = 0; y < ny; ++y) {
        s1 += acc[((long)y * SC + sc) * 2];
        s2 += acc[((long)y * SC + sc) * 2 + 1];
    }
    const float m1 = s1 / n;
    m = K + m1;
    const float vv = s2 / n - m1 * m1;
    v = vv > 0.f ? vv : 0.f;
}
// the extra first workgroup of a forward apply kernel (pooled or not)
__device__ __forceinline__ void stepbn_finalise(const float* __restrict__ x, int B, int C, int HW, const StepBnFused& f) {
    const int SC = f.S * C;
    if (!f.acc) return;   // given statistics: nothing to finalise
    for (int sc = threadIdx.x; sc < SC; sc += blockDim.x) {
        float m, v;
        stepbn_moments(x, f.acc, sc, sc / C, sc % C, B, C, HW, f.ny, SC, m, v);
        f.mean_out[sc] = m;
        f.var_out[sc] = v;
    }
    if (f.run_mean) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {  // loads only inside the loop: they pipeline
            float em = 0.f, ev = 0.f;
#pragma unroll 4
            for (int s = 0; s < f.S; ++s) {
                float m, v;
                stepbn_moments(x, f.acc, s * C + c, s, c, B, C, HW, f.ny, SC, m, v);
                em = fmaf(f.coef[s], m, em);
                ev = fmaf(f.coef_u[s], v, ev);
            }
            f.run_mean[c] = fmaf(f.decay, f.run_mean[c], em);
            f.run_var[c] = fmaf(f.decay, f.run_var[c], ev);
        }
    }
    if (f.nbt && threadIdx.x == 0) *f.nbt += f.S;
}
template <int VEC>
__global__ void stepbn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float* __restrict__ y, unsigned total, int B, int C,
                                    int HW, float eps, int act, float slope, StepBnFused f) {
    const int SC = f.S * C;
    const unsigned nblk = gridDim.x - 1, bid = blockIdx.x - 1;
    if (blockIdx.x == 0) {
        stepbn_finalise(x, B, C, HW, f);
        return;
    }
    const unsigned nvec = total / VEC;
    for (unsigned iv = bid * blockDim.x + threadIdx.x; iv < nvec; iv += nblk * blockDim.x) {
        const unsigned idx = iv * VEC;
        const unsigned r = idx / (unsigned)HW;  // frame * C + c
        const int c = (int)(r % (unsigned)C);
        const int s = (int)(r / (unsigned)C / (unsigned)B);
        float m = f.acc ? 0.f : f.mean_out[s * C + c], vr = f.acc ? 0.f : f.var_out[s * C + c];
        stepbn_moments(x, f.acc, s * C + c, s, c, B, C, HW, f.ny, SC, m, vr);
        const float rstd = rsqrtf(vr + eps);
        const float ga = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
        float v[VEC];
        if (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(x + idx);
            v[0] = t.x; v[1 % VEC] = t.y; v[2 % VEC] = t.z; v[3 % VEC] = t.w;
        } else {
            v[0] = x[idx];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = stepbn_act((v[j] - m) * rstd * ga + be, act, slope);
        if (VEC == 4)
            *reinterpret_cast<float4*>(y + idx) = float4{v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]};
        else
            y[idx] = v[0];
    }
}
// block (sc, j): partial sums of g' and g' * xhat over frames j, j+gridDim.y, ...  with g' = g * act'(y), stored at
// sg[j][sc] / sgx[j][sc] (no atomics, nothing to zero)
__global__ __launch_bounds__(256) void stepbn_bwd_reduce_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ var, float* __restrict__ sg,
                                                                float* __restrict__ sgx, int B, int C, int HW, float eps,
                                                                int act, float slope) {
    __shared__ float sm[4];
    const int s = blockIdx.x / C, c = blockIdx.x - s * C;
    const long off = ((long)s * B * C + c) * HW, fs = (long)C * HW;
    const float m = mean[blockIdx.x], rstd = rsqrtf(var[blockIdx.x] + eps);
    const float ga = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
    float a = 0.f, ax = 0.f;
    if ((HW & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)g)) & 15) == 0) {  // 16-byte loads
        const int HW4 = HW >> 2, nb = (B - (int)blockIdx.y + (int)gridDim.y - 1) / (int)gridDim.y;
        for (int idx = threadIdx.x; idx < nb * HW4; idx += 256) {
            const int bi = idx / HW4, p = idx - bi * HW4;
            const long e0 = off + (blockIdx.y + (long)bi * gridDim.y) * fs;
            const float4 xq = reinterpret_cast<const float4*>(x + e0)[p], gq = reinterpret_cast<const float4*>(g + e0)[p];
            const float xv[4] = {xq.x, xq.y, xq.z, xq.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float xh = (xv[i] - m) * rstd;
                const float gp = gv[i] * stepbn_dact(xh * ga + be, act, slope);
                a += gp;
                ax = fmaf(gp, xh, ax);
            }
        }
    } else {
        for (int b = blockIdx.y; b < B; b += gridDim.y) {
            const long e0 = off + b * fs;
            for (int p = threadIdx.x; p < HW; p += 256) {
                const float xh = (x[e0 + p] - m) * rstd;
                const float gp = g[e0 + p] * stepbn_dact(xh * ga + be, act, slope);
                a += gp;
                ax = fmaf(gp, xh, ax);
            }
        }
    }
    const float ta = block_sum_256(a, sm);
    const float tx = block_sum_256(ax, sm);
    if (threadIdx.x == 0) {
        sg[(long)blockIdx.y * gridDim.x + blockIdx.x] = ta;
        sgx[(long)blockIdx.y * gridDim.x + blockIdx.x] = tx;
    }
}
// the extra first workgroup of a backward apply kernel (pooled or not): the parameter gradients
__device__ __forceinline__ void stepbn_param_grads(const float* __restrict__ sg, const float* __restrict__ sgx,
                                                   float* __restrict__ ggamma, float* __restrict__ gbeta, int C, int S,
                                                   int ny, int world) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < ny * S; ++i) {  // [ny][S][C]: all partials of channel c
            a += sgx[(long)i * C + c];
            b += sg[(long)i * C + c];
        }
        // (world > 1: the partial sums were added over the ranks for gx; a parameter gradient is this rank's
        // share of a rank average, so the sum over ranks is divided by their number)
        ggamma[c] = a / (float)world;
        gbeta[c] = b / (float)world;
    }
}
template <int VEC>
__global__ void stepbn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ beta,
                                        const float* __restrict__ g, const float* __restrict__ mean,
                                        const float* __restrict__ var, const float* __restrict__ gamma,
                                        const float* __restrict__ sg, const float* __restrict__ sgx,
                                        float* __restrict__ gx, unsigned total, int B, int C, int HW, float eps, int act,
                                        float slope, float* __restrict__ ggamma, float* __restrict__ gbeta, int S, int ny,
                                        int world) {
    // (one extra workgroup, the first, for the parameter gradients = the per-step sums added over the steps)
    const int SC = S * C;
    const unsigned nblk = ggamma ? gridDim.x - 1 : gridDim.x, bid = ggamma ? blockIdx.x - 1 : blockIdx.x;
    if (ggamma && blockIdx.x == 0) {
        stepbn_param_grads(sg, sgx, ggamma, gbeta, C, S, ny, world);
        return;
    }
    const float inv_n = 1.f / ((float)(B * HW) * (float)world);
    const unsigned nvec = total / VEC;
    for (unsigned iv = bid * blockDim.x + threadIdx.x; iv < nvec; iv += nblk * blockDim.x) {
        const unsigned idx = iv * VEC;
        const unsigned r = idx / (unsigned)HW;
        const int c = (int)(r % (unsigned)C);
        const int s = (int)(r / (unsigned)C / (unsigned)B);
        const int sc = s * C + c;
        const float rstd = rsqrtf(var[sc] + eps), m = mean[sc];
        const float w = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
        float k1 = 0.f, k2 = 0.f;
        for (int yy = 0; yy < ny; ++yy) {
            k1 += sg[(long)yy * SC + sc];
            k2 += sgx[(long)yy * SC + sc];
        }
        k1 *= inv_n;
        k2 *= inv_n;
        float xv[VEC], gv[VEC];
        if (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(x + idx);
            const float4 u = *reinterpret_cast<const float4*>(g + idx);
            xv[0] = t.x; xv[1 % VEC] = t.y; xv[2 % VEC] = t.z; xv[3 % VEC] = t.w;
            gv[0] = u.x; gv[1 % VEC] = u.y; gv[2 % VEC] = u.z; gv[3 % VEC] = u.w;
        } else {
            xv[0] = x[idx];
            gv[0] = g[idx];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float xh = (xv[j] - m) * rstd;
            const float gp = gv[j] * stepbn_dact(xh * w + be, act, slope);
            xv[j] = w * rstd * (gp - k1 - xh * k2);
        }
        if (VEC == 4)
            *reinterpret_cast<float4*>(gx + idx) = float4{xv[0], xv[1 % VEC], xv[2 % VEC], xv[3 % VEC]};
        else
            gx[idx] = xv[0];
    }
}

// ---------------------------------------------------------------------------- per-step BatchNorm + 2x2 max-pool
// conv -> BatchNorm -> activation -> MaxPool2d(2, 2) of the extractor: the apply kernel writes only the pooled map
// p [S*B, C, H/2, W/2], and the backward recomputes each window's winner from x, so neither the full-resolution
// activation, nor an index map, nor a full-resolution gradient exists.  The statistics kernel, the moments, the finalising
// workgroup and the parameter-gradient workgroup are those of the unpooled kernels above.
// A window's winner by max_pool2d's rule: the ACTIVATED values in the order (0,0), (0,1), (1,0), (1,1); a candidate
// replaces the best when it is larger or NaN.  xv = the four inputs in that order -> the winner's position (0..3), its
// activated value, its xhat and its activation input u.
__device__ __forceinline__ int stepbn_pool_winner(const float xv[4], float m, float rstd, float ga, float be, int act,
                                                  float slope, float& best, float& xh_w, float& u_w) {
    int k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xh = (xv[j] - m) * rstd;
        const float u = xh * ga + be;
        const float a = stepbn_act(u, act, slope);
        if (j == 0 || a > best || isnan(a)) {
            best = a;
            xh_w = xh;
            u_w = u;
            k = j;
        }
    }
    return k;
}
// A thread's unit: VEC == 4: rows 2i, 2i+1 x columns 4j..4j+3 of one plane (two 16-byte loads) = two windows; VEC == 1:
// one window, scalar accesses.  Unit u of either kind: q = u / (units per pooled row) = plane * H/2 + i, its first input
// element is q * 2W + (VEC == 4 ? 4 : 2) * (u - q * units per row) and its first pooled element is u * (VEC == 4 ? 2 : 1).
template <int VEC>
__device__ __forceinline__ void stepbn_pool_load(const float* __restrict__ x, unsigned in0, int W, float xv[2][4]) {
    if (VEC == 4) {
        const float4 r0 = *reinterpret_cast<const float4*>(x + in0);
        const float4 r1 = *reinterpret_cast<const float4*>(x + in0 + W);
        xv[0][0] = r0.x; xv[0][1] = r0.y; xv[0][2] = r1.x; xv[0][3] = r1.y;
        xv[1][0] = r0.z; xv[1][1] = r0.w; xv[1][2] = r1.z; xv[1][3] = r1.w;
    } else {
        xv[0][0] = x[in0]; xv[0][1] = x[in0 + 1]; xv[0][2] = x[in0 + W]; xv[0][3] = x[in0 + W + 1];
    }
}
template <int VEC>
__global__ void stepbn_pool_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, float* __restrict__ p, unsigned nunits, int B,
                                         int C, int H, int W, float eps, int act, float slope, StepBnFused f) {
    constexpr int NW = VEC == 4 ? 2 : 1;  // windows per unit
    const int SC = f.S * C, HW = H * W;
    const unsigned nblk = gridDim.x - 1, bid = blockIdx.x - 1;
    if (blockIdx.x == 0) {
        stepbn_finalise(x, B, C, HW, f);
        return;
    }
    const unsigned upr = (unsigned)W / (2 * NW), Ho = (unsigned)H / 2;
    for (unsigned u = bid * blockDim.x + threadIdx.x; u < nunits; u += nblk * blockDim.x) {
        const unsigned q = u / upr;
        const unsigned r = q / Ho;  // frame * C + c
        const int c = (int)(r % (unsigned)C);
        const int s = (int)(r / (unsigned)C / (unsigned)B);
        float m = f.acc ? 0.f : f.mean_out[s * C + c], vr = f.acc ? 0.f : f.var_out[s * C + c];
        stepbn_moments(x, f.acc, s * C + c, s, c, B, C, HW, f.ny, SC, m, vr);
        const float rstd = rsqrtf(vr + eps);
        const float ga = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
        float xv[2][4], o[NW];
        stepbn_pool_load<VEC>(x, q * 2u * (unsigned)W + 2u * NW * (u - q * upr), W, xv);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            float xh, uu;
            stepbn_pool_winner(xv[w], m, rstd, ga, be, act, slope, o[w], xh, uu);
        }
        if (VEC == 4)
            *reinterpret_cast<float2*>(p + 2u * u) = float2{o[0], o[NW - 1]};
        else
            p[u] = o[0];
    }
}
// block (sc, j): partial sums of g' and g' * xhat_winner over the windows of frames j, j+gridDim.y, ... with
// g' = gp * act'(u_winner), stored like stepbn_bwd_reduce_kernel's (the same terms: a lost position's gradient is zero).
// A block adds its terms in fp64 and rounds its pair once (a quarter of the unpooled kernel's loads feed the sums, so the
// adds are hidden behind them): the fp32 partial rows and their consumers are unchanged.
__device__ __forceinline__ double block_sum_256_f64(double v, double* sm /* >= 4 doubles */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
template <int VEC>
__global__ __launch_bounds__(256) void stepbn_pool_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ gp, const float* __restrict__ mean, const float* __restrict__ var, float* __restrict__ sg,
    float* __restrict__ sgx, int B, int C, int H, int W, float eps, int act, float slope) {
    constexpr int NW = VEC == 4 ? 2 : 1;
    __shared__ double sm[4];
    const int s = blockIdx.x / C, c = blockIdx.x - s * C;
    const int HW = H * W, upr = W / (2 * NW), upf = (H / 2) * upr;  // units per pooled row / per plane
    const unsigned pl0 = (unsigned)(s * B) * C + c;                 // plane of frame 0 of this step
    const float m = mean[blockIdx.x], rstd = rsqrtf(var[blockIdx.x] + eps);
    const float ga = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
    double a = 0., ax = 0.;
    const int nb = (B - (int)blockIdx.y + (int)gridDim.y - 1) / (int)gridDim.y;
    for (int idx = threadIdx.x; idx < nb * upf; idx += 256) {
        const int bi = idx / upf, t = idx - bi * upf;
        const unsigned pl = pl0 + (blockIdx.y + (unsigned)bi * gridDim.y) * (unsigned)C;
        const int i = t / upr, j = t - i * upr;
        float xv[2][4], gv[NW];
        stepbn_pool_load<VEC>(x, pl * (unsigned)HW + 2u * i * W + 2u * NW * j, W, xv);
        const unsigned o0 = pl * (unsigned)(HW / 4) + (unsigned)t * NW;
        if (VEC == 4) {
            const float2 g2 = *reinterpret_cast<const float2*>(gp + o0);
            gv[0] = g2.x; gv[NW - 1] = g2.y;
        } else {
            gv[0] = gp[o0];
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            float best, xh, u;
            stepbn_pool_winner(xv[w], m, rstd, ga, be, act, slope, best, xh, u);
            const float g1 = gv[w] * stepbn_dact(u, act, slope);
            a += (double)g1;
            ax = fma((double)g1, (double)xh, ax);
        }
    }
    const float ta = (float)block_sum_256_f64(a, sm);
    const float tx = (float)block_sum_256_f64(ax, sm);
    if (threadIdx.x == 0) {
        sg[(long)blockIdx.y * gridDim.x + blockIdx.x] = ta;
        sgx[(long)blockIdx.y * gridDim.x + blockIdx.x] = tx;
    }
}
// gx = gamma rstd (g' [winner] - k1 - xhat k2) at the four positions of every window
template <int VEC>
__global__ void stepbn_pool_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ beta,
                                             const float* __restrict__ gp, const float* __restrict__ mean,
                                             const float* __restrict__ var, const float* __restrict__ gamma,
                                             const float* __restrict__ sg, const float* __restrict__ sgx,
                                             float* __restrict__ gx, unsigned nunits, int B, int C, int H, int W,
                                             float eps, int act, float slope, float* __restrict__ ggamma,
                                             float* __restrict__ gbeta, int S, int ny, int world) {
    constexpr int NW = VEC == 4 ? 2 : 1;
    const int SC = S * C, HW = H * W;
    const unsigned nblk = ggamma ? gridDim.x - 1 : gridDim.x, bid = ggamma ? blockIdx.x - 1 : blockIdx.x;
    if (ggamma && blockIdx.x == 0) {
        stepbn_param_grads(sg, sgx, ggamma, gbeta, C, S, ny, world);
        return;
    }
    const float inv_n = 1.f / ((float)(B * HW) * (float)world);
    const unsigned upr = (unsigned)W / (2 * NW), Ho = (unsigned)H / 2;
    for (unsigned u = bid * blockDim.x + threadIdx.x; u < nunits; u += nblk * blockDim.x) {
        const unsigned q = u / upr;
        const unsigned r = q / Ho;
        const int c = (int)(r % (unsigned)C);
        const int s = (int)(r / (unsigned)C / (unsigned)B);
        const int sc = s * C + c;
        const float rstd = rsqrtf(var[sc] + eps), m = mean[sc];
        const float w = gamma ? gamma[c] : 1.f, be = gamma ? beta[c] : 0.f;
        float k1 = 0.f, k2 = 0.f;
        for (int yy = 0; yy < ny; ++yy) {
            k1 += sg[(long)yy * SC + sc];
            k2 += sgx[(long)yy * SC + sc];
        }
        k1 *= inv_n;
        k2 *= inv_n;
        const unsigned in0 = q * 2u * (unsigned)W + 2u * NW * (u - q * upr);
        float xv[2][4], gv[NW];
        stepbn_pool_load<VEC>(x, in0, W, xv);
        if (VEC == 4) {
            const float2 g2 = *reinterpret_cast<const float2*>(gp + 2u * u);
            gv[0] = g2.x; gv[NW - 1] = g2.y;
        } else {
            gv[0] = gp[u];
        }
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            float best, xhw, uw;
            const int k = stepbn_pool_winner(xv[ww], m, rstd, w, be, act, slope, best, xhw, uw);
            const float g1 = gv[ww] * stepbn_dact(uw, act, slope);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (xv[ww][j] - m) * rstd;
                const float gpos = j == k ? g1 : 0.f;
                xv[ww][j] = w * rstd * (gpos - k1 - xh * k2);
            }
        }
        if (VEC == 4) {
            *reinterpret_cast<float4*>(gx + in0) = float4{xv[0][0], xv[0][1], xv[NW - 1][0], xv[NW - 1][1]};
            *reinterpret_cast<float4*>(gx + in0 + W) = float4{xv[0][2], xv[0][3], xv[NW - 1][2], xv[NW - 1][3]};
        } else {
            gx[in0] = xv[0][0]; gx[in0 + 1] = xv[0][1]; gx[in0 + W] = xv[0][2]; gx[in0 + W + 1] = xv[0][3];
        }
    }
}

// ---------------------------------------------------------------------------- the host side of both forms
// The launch decisions of the entry points, plain and pooled, made once: the launchers below launch what this says and
// rfn_stepbn_kernel_label / rfn_stepbn_pool_kernel_label print it.  The plain form passes its HW as (H, W) = (HW, 1).
// `aligned` bit 0: every pointer the stats (x) / reduce (x, g) kernel tests is 16-byte aligned; bit 1: the same for the
// apply kernel (forward x, y; backward x, g, gx).  The plain stats / reduce kernels decide their load width on the
// device, by the test restated in stats_vec.  The pooled forward runs the plain stats kernel, whose H*W % 4 is always 0
// there; the pooled reduce and apply kernels read two 16-byte row pieces per unit and need W % 4 == 0.
constexpr int STEPBN_GRID_CAP = 16384, STEPBN_POOL_GRID_CAP = 8192;
struct StepBnRoute {
    int ny;          // workgroups per (step, channel) of the stats / reduce kernel (stepbn_split)
    bool stats_vec;  // stats / reduce kernel: 16-byte loads; else the scalar loops (pooled reduce: <4>; else <1>)
    bool v4;         // apply kernel <4> (plain: 4 pixels per thread, pooled: units of two windows); else <1>
    long total;      // elements of x
    long nunits;     // threads' units of the apply kernel
    int grid;        // streaming workgroups of the apply kernel (the launch adds the one that finalises, if any)
    int sweeps;      // most grid-stride iterations of an apply workgroup
};
static StepBnRoute choose_stepbn(int S, int B, int C, int H, int W, bool pool, int aligned, int bwd) {
    StepBnRoute r;
    r.total = (long)S * B * C * H * W;
    r.ny = stepbn_split(S, B, C);
    if (pool) {
        r.stats_vec = (aligned & 1) && (bwd ? W % 4 == 0 : true);
        r.v4 = W % 4 == 0 && (aligned & 2);
        r.nunits = r.v4 ? r.total / 8 : r.total / 4;
    } else {
        r.stats_vec = H * W % 4 == 0 && (aligned & 1);
        r.v4 = H * W % 4 == 0 && (aligned & 2);
        r.nunits = r.v4 ? r.total / 4 : r.total;
    }
    const long nb = (r.nunits + 255) / 256, cap = pool ? STEPBN_POOL_GRID_CAP : STEPBN_GRID_CAP;
    r.grid = (int)(nb < cap ? nb : cap);
    r.sweeps = (int)((nb + r.grid - 1) / r.grid);
    return r;
}
static int stepbn_aligned(const void* s0, const void* s1, const void* a0, const void* a1, const void* a2) {
    const uintptr_t st = (uintptr_t)s0 | (uintptr_t)s1, ap = (uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2;
    return ((st & 15) == 0 ? 1 : 0) | ((ap & 15) == 0 ? 2 : 0);
}
static const char* stepbn_label(char (&buf)[160], const char* name, int S, int B, int C, int H, int W, bool pool, int aligned,
                                int bwd) {
    if (S <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (pool && (H % 2 || W % 2)) || (long)S * B * C * H * W >= (1L << 31))
        return "unsupported";
    const StepBnRoute r = choose_stepbn(S, B, C, H, W, pool, aligned, bwd);
    snprintf(buf, sizeof(buf), "%s ny=%d stats=%s apply=%s grid=%d sweeps=%d", name, r.ny, r.stats_vec ? "vec" : "scalar",
             r.v4 ? "vec4" : "vec1", r.grid, r.sweeps);
    return buf;
}
// bwd says which pair of kernels `aligned` was derived for (forward: stats + apply, backward: reduce + apply); the
// plain route arithmetic is the same either way, so it changes nothing printed there
extern "C" const char* rfn_stepbn_kernel_label(int S, int B, int C, int HW, int aligned, int bwd) {
    static thread_local char buf[160];
    return stepbn_label(buf, "stepbn", S, B, C, HW, 1, false, aligned, bwd);
}
extern "C" const char* rfn_stepbn_pool_kernel_label(int S, int B, int C, int H, int W, int aligned, int bwd) {
    static thread_local char buf[160];
    return stepbn_label(buf, "stepbn_pool", S, B, C, H, W, true, aligned, bwd);
}
// floats of scratch the forward (acc) / backward (sums) entry points need for these sizes
extern "C" long rfn_stepbn_scratch_floats(int S, int B, int C) {
    if (S <= 0 || B <= 0 || C <= 0) return 0;
    return 2L * S * C * stepbn_split(S, B, C);
}

// The argument checks of the five entry points, in one order.  A macro, because RFN_CHECK_ARG names the function it
// stands in and the condition as written: `ptrs` = the pointers that must be set, `pairs` = the both-or-neither rules;
// S, B, C are the entry point's own, the plain form passes (HW, 1) for (H, W) and the forward (0, 1) for (stage, world).
#define STEPBN_CHECK_ARGS(ptrs, pairs, H, W, pool, stage, world)                              \
    RFN_CHECK_ARG(ptrs && S > 0 && B > 0 && C > 0 && H > 0 && W > 0, -1);                     \
    RFN_CHECK_ARG(stage >= 0 && stage <= 2 && world >= 1, -4);                                \
    RFN_CHECK_ARG(pairs, -2);                                                                 \
    RFN_CHECK_ARG(!pool || (H % 2 == 0 && W % 2 == 0), -5);                                   \
    RFN_CHECK_ARG((long)S * B * C * H * W < (1L << 31), -3)
#define STEPBN_BOTH_OR_NEITHER(a, b) ((a && b) || (!a && !b))
#define STEPBN_RUNNING_OK ((run_mean && run_var && coef && coef_u) || (!run_mean && !run_var))

// acc set: the statistics launch, then apply + finalise (mean / var are outputs, the running statistics optional);
// acc null: one apply launch with GIVEN statistics mean / var and no running arguments.
static void stepbn_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* var,
                           float* acc, float* run_mean, float* run_var, const float* coef, const float* coef_u,
                           float decay, long long* nbt, int S, int B, int C, int H, int W, bool pool, float eps, int act,
                           float slope, hipStream_t st) {
    const StepBnRoute r = choose_stepbn(S, B, C, H, W, pool, stepbn_aligned(x, nullptr, x, y, nullptr), 0);
    if (acc) hipLaunchKernelGGL(stepbn_stats_kernel, dim3(S * C, r.ny), dim3(256), 0, st, x, acc, B, C, H * W);
    const StepBnFused f = {acc, mean, var, run_mean, run_var, coef, coef_u, decay, nbt, S, acc ? r.ny : 0};
    if (pool)
        launch_vec(r.v4, stepbn_pool_apply_kernel<4>, stepbn_pool_apply_kernel<1>, dim3(r.grid + 1), st, x, gamma, beta, y,
                   (unsigned)r.nunits, B, C, H, W, eps, act, slope, f);
    else
        launch_vec(r.v4, stepbn_apply_kernel<4>, stepbn_apply_kernel<1>, dim3(r.grid + 1), st, x, gamma, beta, y,
                   (unsigned)r.total, B, C, H * W, eps, act, slope, f);
}
// stage 0: both launches; 1: the partial sums only; 2: the apply only (the caller has added `sums` over `world`
// data-parallel ranks in between: synchronised BatchNorm; mean / var are the global statistics).  g is the gradient of
// the entry point's output: full resolution (plain) or pooled.
static void stepbn_backward(const float* x, const float* gamma, const float* beta, const float* g, const float* mean,
                            const float* var, float* sums, float* gx, float* ggamma, float* gbeta, int S, int B, int C,
                            int H, int W, bool pool, float eps, int act, float slope, int stage, int world, hipStream_t st) {
    const StepBnRoute r = choose_stepbn(S, B, C, H, W, pool, stepbn_aligned(x, g, x, g, gx), 1);
    const int ny = r.ny;
    float* sg = sums;
    float* sgx = sums + (long)ny * S * C;
    if (stage != 2) {
        if (pool)
            launch_vec(r.stats_vec, stepbn_pool_bwd_reduce_kernel<4>, stepbn_pool_bwd_reduce_kernel<1>, dim3(S * C, ny), st, x,
                       gamma, beta, g, mean, var, sg, sgx, B, C, H, W, eps, act, slope);
        else
            hipLaunchKernelGGL(stepbn_bwd_reduce_kernel, dim3(S * C, ny), dim3(256), 0, st, x, gamma, beta, g, mean, var, sg,
                               sgx, B, C, H * W, eps, act, slope);
    }
    if (stage == 1) return;
    const dim3 grid(r.grid + (ggamma ? 1 : 0));  // one more workgroup, the first, for the parameter gradients
    if (pool)
        launch_vec(r.v4, stepbn_pool_bwd_apply_kernel<4>, stepbn_pool_bwd_apply_kernel<1>, grid, st, x, beta, g, mean, var,
                   gamma, sg, sgx, gx, (unsigned)r.nunits, B, C, H, W, eps, act, slope, ggamma, gbeta, S, ny, world);
    else
        launch_vec(r.v4, stepbn_bwd_apply_kernel<4>, stepbn_bwd_apply_kernel<1>, grid, st, x, beta, g, mean, var, gamma, sg,
                   sgx, gx, (unsigned)r.total, B, C, H * W, eps, act, slope, ggamma, gbeta, S, ny, world);
}

// stats + normalise + activate + running statistics in TWO launches (partial sums, apply): what per_step_batchnorm_act
// needs of one BatchNorm layer.  mean / var [S*C] are outputs (kept for the backward); run_mean / run_var [C] (both or
// neither) receive r <- decay r + sum_s coef[s] stat[s] with coef / coef_u [S] on the device; nbt (optional) += S.
extern "C" int rfn_stepbn_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* var,
                                  float* acc, float* run_mean, float* run_var, const float* coef, const float* coef_u,
                                  float decay, long long* nbt, int S, int B, int C, int HW, float eps, int act, float slope,
                                  rfn_stream_t stream) {
    STEPBN_CHECK_ARGS(x && y && mean && var && acc,
                      STEPBN_BOTH_OR_NEITHER(gamma, beta) && STEPBN_RUNNING_OK, HW, 1, false, 0, 1);
    stepbn_forward(x, gamma, beta, y, mean, var, acc, run_mean, run_var, coef, coef_u, decay, nbt, S, B, C, HW, 1, false, eps,
                   act, slope, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
/* normalise + activate with GIVEN per-step statistics mean / var [S*C] (synchronised BatchNorm across data-parallel
 * ranks: the caller combined the ranks' moments); one launch */
extern "C" int rfn_stepbn_apply_f32(const float* x, const float* gamma, const float* beta, float* y, const float* mean,
                                    const float* var, int S, int B, int C, int HW, float eps, int act, float slope,
                                    rfn_stream_t stream) {
    STEPBN_CHECK_ARGS(x && y && mean && var, STEPBN_BOTH_OR_NEITHER(gamma, beta), HW, 1, false, 0, 1);
    stepbn_forward(x, gamma, beta, y, const_cast<float*>(mean), const_cast<float*>(var), nullptr, nullptr, nullptr, nullptr,
                   nullptr, 0.f, nullptr, S, B, C, HW, 1, false, eps, act, slope, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
// the whole backward of one layer in TWO launches (per-step partial sums, apply): sums = scratch
// [rfn_stepbn_scratch_floats] (sg | sgx); ggamma / gbeta [C] (both or neither) = the parameter gradients, written by the
// apply kernel
extern "C" int rfn_stepbn_bwd_f32(const float* x, const float* gamma, const float* beta, const float* g, const float* mean,
                                  const float* var, float* sums, float* gx, float* ggamma, float* gbeta, int S, int B,
                                  int C, int HW, float eps, int act, float slope, int stage, int world,
                                  rfn_stream_t stream) {
    STEPBN_CHECK_ARGS(x && g && mean && var && sums && gx,
                      STEPBN_BOTH_OR_NEITHER(gamma, beta) && STEPBN_BOTH_OR_NEITHER(ggamma, gbeta), HW, 1, false, stage, world);
    stepbn_backward(x, gamma, beta, g, mean, var, sums, gx, ggamma, gbeta, S, B, C, HW, 1, false, eps, act, slope, stage,
                    world, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
// rfn_stepbn_fwd_f32 with the 2x2 max-pool folded into the apply launch: p [S*B, C, H/2, W/2] is the only map written
extern "C" int rfn_stepbn_pool_fwd_f32(const float* x, const float* gamma, const float* beta, float* p, float* mean,
                                       float* var, float* acc, float* run_mean, float* run_var, const float* coef,
                                       const float* coef_u, float decay, long long* nbt, int S, int B, int C, int H, int W,
                                       float eps, int act, float slope, rfn_stream_t stream) {
    STEPBN_CHECK_ARGS(x && p && mean && var && acc,
                      STEPBN_BOTH_OR_NEITHER(gamma, beta) && STEPBN_RUNNING_OK, H, W, true, 0, 1);
    stepbn_forward(x, gamma, beta, p, mean, var, acc, run_mean, run_var, coef, coef_u, decay, nbt, S, B, C, H, W, true, eps,
                   act, slope, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
// the backward of that layer from the POOLED gradient gp [S*B, C, H/2, W/2]: stage / world as rfn_stepbn_bwd_f32
extern "C" int rfn_stepbn_pool_bwd_f32(const float* x, const float* gamma, const float* beta, const float* gp,
                                       const float* mean, const float* var, float* sums, float* gx, float* ggamma,
                                       float* gbeta, int S, int B, int C, int H, int W, float eps, int act, float slope,
                                       int stage, int world, rfn_stream_t stream) {
    STEPBN_CHECK_ARGS(x && gp && mean && var && sums && gx,
                      STEPBN_BOTH_OR_NEITHER(gamma, beta) && STEPBN_BOTH_OR_NEITHER(ggamma, gbeta), H, W, true, stage, world);
    stepbn_backward(x, gamma, beta, gp, mean, var, sums, gx, ggamma, gbeta, S, B, C, H, W, true, eps, act, slope, stage,
                    world, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
