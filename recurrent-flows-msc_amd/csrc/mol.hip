// Mixture-of-discretized-logistics likelihood of the SRNN baseline (Utils/discretize_logits.py of the reference, the
// PixelCNN++ likelihood; DESIGN.md section 19 is the definition) on fp32 NCHW tensors, gfx950.
//   x [N,C,H,W] in [-1,1], C in {1,3};  l [N,Cl,H,W], Cl = M (1 + P C), P = 3 (RGB: mean, log-scale, coefficient) or 2.
//   channel m                      mixture logit of component m
//   channel M + (c P + j) M + m    parameter j of colour channel c, component m
// One thread per pixel, the channel loop inside the thread: the lanes of a wave hold adjacent pixels of one frame, so
// every channel load and every gradient store is one dense 256-byte row per wave.  Nothing M-wide lives in registers or
// memory: the two log-sum-exps run online over the component loop, and the backward recomputes the items from x and l
// (it reads the forward's log-sum-exp, one float per pixel, for the responsibilities).  A workgroup belongs to ONE frame
// and the frame's sum is its workgroups' partials added in index order by a second small launch: no atomics, and the
// bits of a frame's sum depend on nothing but that frame.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr float kBin = 1.0f / 255.0f;
constexpr float kLog1275 = 4.8481163645f;  // log(127.5)
constexpr float kMinLogScale = -7.0f;

// log-probability of one (pixel, colour channel, component) item and, with GRAD, its derivatives with respect to the
// (adjusted) mean and the UNCLAMPED log-scale.  With p = (x - mu + 1/255)/s, q = (x - mu - 1/255)/s, mid = (x - mu)/s:
//   x < -0.999:  log sigmoid(p)        x > 0.999:  log(1 - sigmoid(q))
//   otherwise    delta = sigmoid(p) - sigmoid(q);  delta > 1e-5 ? log(delta) : log pdf(mid) - log s - log 127.5
// delta is taken from ONE exponential on the side where it cannot overflow: with h = (1/255)/s, k = exp(-2h),
// E1 = exp(mid <= 0 ? p : -q), E2 = k E1:  delta = E1 (1 - k) / ((1 + E1)(1 + E2)), 1 - k from expm1 -- no difference
// of two sigmoids, which is where the op chain loses its digits.  The same quantities give d log(delta)/dp and /dq in
// closed form, and their sum (the mean's gradient) as (1 - E1 E2) / ((1 + E1)(1 + E2)), again without a difference.
template <bool GRAD>
__device__ __forceinline__ float mol_item(float x, float mu, float ls_raw, float& gmu, float& gls) {
    const float ls = fmaxf(ls_raw, kMinLogScale);
    const float inv = expf(-ls);
    const float cx = x - mu;
    float L;
    if (x < -0.999f) {
        const float p = inv * (cx + kBin);
        const float ea = expf(-fabsf(p));
        L = fminf(p, 0.f) - log1pf(ea);
        if (GRAD) {
            const float g = (p >= 0.f ? ea : 1.0f) / (1.0f + ea);  // sigmoid(-p)
            gmu = -inv * g;
            gls = -p * g;
        }
    } else if (x > 0.999f) {
        const float q = inv * (cx - kBin);
        const float ea = expf(-fabsf(q));
        L = -(fmaxf(q, 0.f) + log1pf(ea));
        if (GRAD) {
            const float g = -(q >= 0.f ? 1.0f : ea) / (1.0f + ea);  // -sigmoid(q)
            gmu = -inv * g;
            gls = -q * g;
        }
    } else {
        const float mid = inv * cx, h = inv * kBin;
        const bool low = mid <= 0.f;
        const float omk = -expm1f(-2.0f * h);                  // 1 - k
        const float E1 = expf(low ? mid + h : h - mid), E2 = E1 * (1.0f - omk);
        const float a1 = 1.0f + E1, a2 = 1.0f + E2;
        const float delta = E1 * omk / (a1 * a2);
        if (delta > 1e-5f) {
            L = logf(delta);  // (the reference's clamp at 1e-12 cannot bind here)
            if (GRAD) {
                const float s1 = a2 / (a1 * omk), s2 = (1.0f - omk) * a1 / (a2 * omk);  // sigmoid'(.)/delta of E1's, E2's side
                float gsum = (1.0f - E1 * E2) / (a1 * a2);                                // d/dp + d/dq
                if (!low) gsum = -gsum;
                gmu = -inv * gsum;
                gls = -(mid * gsum + h * (s1 + s2));
            }
        } else {
            const float ea = expf(-fabsf(mid));
            L = -fabsf(mid) - 2.0f * log1pf(ea) - ls - kLog1275;
            if (GRAD) {
                const float t = (1.0f - ea) / (1.0f + ea);         // tanh(|mid|/2)
                const float g = mid >= 0.f ? -t : t;               // 1 - 2 sigmoid(mid)
                gmu = -inv * g;
                gls = -mid * g - 1.0f;
            }
        }
    }
    if (GRAD && ls_raw < kMinLogScale) gls = 0.f;  // the clamp binds
    return L;
}

__device__ __forceinline__ void lse_push(float v, float& mx, float& s) {
    if (v > mx) {
        s = s * expf(mx - v) + 1.0f;
        mx = v;
    } else {
        s += expf(v - mx);
    }
}

// sum over colour channels of the item log-probabilities of component m; with GRAD the per-channel derivatives too
template <int C, bool GRAD>
__device__ __forceinline__ float mol_component(const float* __restrict__ lp, long HW, int M, int m, const float (&xv)[C],
                                               float (&gmu)[C], float (&gls)[C], float (&th)[C]) {
    constexpr int P = C == 3 ? 3 : 2;
    float S = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = lp + ((long)M + ((long)c * P) * M + m) * HW;
        float mu = q[0];
        const float ls = q[(long)M * HW];
        if (C == 3) th[c] = tanhf(q[2L * M * HW]);
        if (C == 3 && c == 1) mu += th[0] * xv[0];
        if (C == 3 && c == 2) mu += th[1] * xv[0] + th[2] * xv[1];
        S += mol_item<GRAD>(xv[c], mu, ls, gmu[c], gls[c]);
    }
    return S;
}

// grid N * nbx workgroups of 256 pixels of one frame; part [N][nbx]
template <int C>
__global__ __launch_bounds__(256) void mol_nll_fwd_kernel(const float* __restrict__ x, const float* __restrict__ l,
                                                          float* __restrict__ nll_pix, float* __restrict__ lse,
                                                          float* __restrict__ part, int M, int HW, int nbx) {
    __shared__ float sm[4];
    constexpr int P = C == 3 ? 3 : 2;
    const int n = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int p = bx * 256 + threadIdx.x;
    float v = 0.f;
    if (p < HW) {
        const long Cl = (long)M * (1 + P * C);
        const float* lp = l + (long)n * Cl * HW + p;
        float xv[C], gmu[C], gls[C], th[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c] = x[((long)n * C + c) * HW + p];
        float lg = lp[0];
        float mxl = lg, sl = 1.0f;
        float mx = mol_component<C, false>(lp, HW, M, 0, xv, gmu, gls, th) + lg, s = 1.0f;
        for (int m = 1; m < M; ++m) {
            lg = lp[(long)m * HW];
            lse_push(lg, mxl, sl);
            lse_push(mol_component<C, false>(lp, HW, M, m, xv, gmu, gls, th) + lg, mx, s);
        }
        const float ls = mx + logf(s);
        v = (mxl + logf(sl)) - ls;
        nll_pix[(long)n * HW + p] = v;
        lse[(long)n * HW + p] = ls;
    }
    v = block_sum_256(v, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void mol_frame_sum_kernel(const float* __restrict__ part, float* __restrict__ nll, int N,
                                                            int nbx) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float t = 0.f;
    for (int i = 0; i < nbx; ++i) t += part[(long)n * nbx + i];
    nll[n] = t;
}

// same grid.  up: [N] (per_pixel = 0) or [N,HW].  lse: the forward's log-sum-exp over components of v_m = S_m + logit_m;
// the responsibility of component m is exp(v_m - lse) with v_m recomputed by the forward's own operations, bit for bit:
// for M = 1 it is exp(0) = 1 and the logit's gradient exactly 0, as autograd gives them.
template <int C>
__global__ __launch_bounds__(256) void mol_nll_bwd_kernel(const float* __restrict__ x, const float* __restrict__ l,
                                                          const float* __restrict__ lse, const float* __restrict__ up,
                                                          int per_pixel, float* __restrict__ dl, int M, int HW, int nbx) {
    constexpr int P = C == 3 ? 3 : 2;
    const int n = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int p = bx * 256 + threadIdx.x;
    if (p >= HW) return;
    const long Cl = (long)M * (1 + P * C);
    const float* lp = l + (long)n * Cl * HW + p;
    float* gp = dl + (long)n * Cl * HW + p;
    float xv[C], gmu[C], gls[C], th[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = x[((long)n * C + c) * HW + p];
    const float g = per_pixel ? up[(long)n * HW + p] : up[n];
    const float lv = lse[(long)n * HW + p];
    float mxl = lp[0], sl = 1.0f;
    for (int m = 1; m < M; ++m) lse_push(lp[(long)m * HW], mxl, sl);
    const float lse_mix = mxl + logf(sl);
    for (int m = 0; m < M; ++m) {
        const float lg = lp[(long)m * HW];
        const float S = mol_component<C, true>(lp, HW, M, m, xv, gmu, gls, th);
        const float r = expf((S + lg) - lv);  // responsibility of component m
        gp[(long)m * HW] = g * (expf(lg - lse_mix) - r);
        const float w = -g * r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* q = gp + ((long)M + ((long)c * P) * M + m) * HW;
            q[0] = w * gmu[c];
            q[(long)M * HW] = w * gls[c];
        }
        if (C == 3) {
            const float k0 = w * gmu[1] * xv[0] * (1.0f - th[0] * th[0]);
            const float k1 = w * gmu[2] * xv[0] * (1.0f - th[1] * th[1]);
            const float k2 = w * gmu[2] * xv[1] * (1.0f - th[2] * th[2]);
            gp[((long)M + 2L * M + m) * HW] = k0;
            gp[((long)M + 5L * M + m) * HW] = k1;
            gp[((long)M + 8L * M + m) * HW] = k2;
        }
    }
}

// u_mix [N,HW,M], u_x [N,HW,C] (the reference's draw shapes), out [N,C,HW]
template <int C>
__global__ __launch_bounds__(256) void mol_sample_kernel(const float* __restrict__ l, const float* __restrict__ u_mix,
                                                         const float* __restrict__ u_x, float* __restrict__ out, int M,
                                                         int HW, int nbx) {
    constexpr int P = C == 3 ? 3 : 2;
    const int n = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int p = bx * 256 + threadIdx.x;
    if (p >= HW) return;
    const long Cl = (long)M * (1 + P * C);
    const float* lp = l + (long)n * Cl * HW + p;
    const float* um = u_mix + ((long)n * HW + p) * M;
    int best = 0;
    float sc = lp[0] - logf(-logf(um[0]));
    for (int m = 1; m < M; ++m) {
        const float t = lp[(long)m * HW] - logf(-logf(um[m]));
        if (t > sc) {  // strict: the lowest index wins a tie
            sc = t;
            best = m;
        }
    }
    float xs[C], th[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = lp + ((long)M + ((long)c * P) * M + best) * HW;
        const float u = u_x[((long)n * HW + p) * C + c];
        float v = q[0] + expf(fmaxf(q[(long)M * HW], kMinLogScale)) * (logf(u) - logf(1.0f - u));
        if (C == 3) th[c] = tanhf(q[2L * M * HW]);
        if (C == 3 && c == 1) v += th[0] * xs[0];
        if (C == 3 && c == 2) v += th[1] * xs[0] + th[2] * xs[1];
        xs[c] = fminf(fmaxf(v, -1.0f), 1.0f);
        out[((long)n * C + c) * HW + p] = xs[c];
    }
}

bool mol_grid(int N, int HW, int* nbx, long* blocks) {
    *nbx = ceil_div(HW, 256);
    *blocks = (long)N * *nbx;
    return *blocks <= 0x7fffffffL;
}

}  // namespace

extern "C" long rfn_mol_part_floats(int N, int HW) {
    if (N <= 0 || HW <= 0) return 0;
    return (long)N * ceil_div(HW, 256);
}

extern "C" int rfn_mol_nll_fwd(const float* x, const float* l, float* nll_pix, float* lse, float* nll, float* part, int N,
                               int C, int M, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(x && l && nll_pix && lse && nll && part, -1);
    RFN_CHECK_ARG(N > 0 && (C == 1 || C == 3) && M > 0 && HW > 0, -2);
    int nbx;
    long blocks;
    RFN_CHECK_ARG(mol_grid(N, HW, &nbx, &blocks), -3);
    hipStream_t st = (hipStream_t)stream;
    if (C == 3)
        hipLaunchKernelGGL(mol_nll_fwd_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, x, l, nll_pix, lse, part, M,
                           HW, nbx);
    else
        hipLaunchKernelGGL(mol_nll_fwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, x, l, nll_pix, lse, part, M,
                           HW, nbx);
    hipLaunchKernelGGL(mol_frame_sum_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, part, nll, N, nbx);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_mol_nll_bwd(const float* x, const float* l, const float* lse, const float* up, int up_per_pixel,
                               float* dl, int N, int C, int M, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(x && l && lse && up && dl, -1);
    RFN_CHECK_ARG(N > 0 && (C == 1 || C == 3) && M > 0 && HW > 0, -2);
    int nbx;
    long blocks;
    RFN_CHECK_ARG(mol_grid(N, HW, &nbx, &blocks), -3);
    hipStream_t st = (hipStream_t)stream;
    if (C == 3)
        hipLaunchKernelGGL(mol_nll_bwd_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, x, l, lse, up, up_per_pixel,
                           dl, M, HW, nbx);
    else
        hipLaunchKernelGGL(mol_nll_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, x, l, lse, up, up_per_pixel,
                           dl, M, HW, nbx);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_mol_sample(const float* l, const float* u_mix, const float* u_x, float* out, int N, int C, int M,
                                  int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(l && u_mix && u_x && out, -1);
    RFN_CHECK_ARG(N > 0 && (C == 1 || C == 3) && M > 0 && HW > 0, -2);
    int nbx;
    long blocks;
    RFN_CHECK_ARG(mol_grid(N, HW, &nbx, &blocks), -3);
    hipStream_t st = (hipStream_t)stream;
    if (C == 3)
        hipLaunchKernelGGL(mol_sample_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, l, u_mix, u_x, out, M, HW, nbx);
    else
        hipLaunchKernelGGL(mol_sample_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, l, u_mix, u_x, out, M, HW, nbx);
    RFN_LAUNCH_CHECK();
    return 0;
}
