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
#include "philox.h"
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

// ---- the sampler.  The arithmetic after the uniforms is ONE device function, mol_sample_pixel; its uniforms come from a
// source object, eight mixture uniforms (one "block") at a time and the C colour uniforms at once, always through
// compile-time register indices (a run-time index into u[] would put it in scratch memory):
//   MolGivenUniforms  reads them from u_mix [N,HW,M] and u_x [N,HW,C] (the reference's draw shapes)   rfn_mol_sample
//   MolKeyedUniforms  makes them from their address (below)                                            rfn_mol_sample_keyed
// so the keyed sampler and the sampler fed the emitted uniforms run the same operations on the same numbers.
struct MolGivenUniforms {
    const float* um;  // this pixel's M mixture uniforms
    const float* ux;  // this pixel's C colour uniforms
    __device__ __forceinline__ void mix_block(int j, int M, float (&u)[8]) const {
        const int left = M - 8 * j;
#pragma unroll
        for (int e = 0; e < 8; ++e) u[e] = e < left ? um[8 * j + e] : 0.5f;
    }
    template <int C>
    __device__ __forceinline__ void colour(float (&u)[C]) const {
#pragma unroll
        for (int c = 0; c < C; ++c) u[c] = ux[c];
    }
};

// Addressed uniforms (DESIGN.md section 20 is the contract).  Row n of a launch is draw first_draw + n / B of sequence
// first_seq + n % B (draw-major, as csrc/keyed_normal.hip).  Block j of pixel p:
//   Philox4x64-10(key = (seed, (step << 32) | slot), counter = (j, p, seq, draw)),  slot 16 mixture, 17 colour
//   (keyed_normal owns slots 0..7: another key, so no address is shared with it).
// Uniform e (e = m for the mixture, e = c for the colour) is the 32-bit half e % 8 of block e / 8, the halves in
// keyed_normal's order (high half of w0, low half of w0, high half of w1, ...):
//   u = min(max((2 (half >> 9) + 1) 2^-24, 1e-5f), 1 - 1e-5f)
// The numerator is an odd integer below 2^24: u is exact, never 0 or 1, and no rounded multiply enters.
constexpr uint32_t kMolSlotMix = 16, kMolSlotColour = 17;
constexpr float kMolULo = 1e-5f, kMolUHi = 1.0f - 1e-5f;

__device__ __forceinline__ float mol_uniform(uint32_t half) {
    const float u = (float)(2u * (half >> 9) + 1u) * 0x1p-24f;
    return fminf(fmaxf(u, kMolULo), kMolUHi);
}

struct MolKeyedUniforms {
    uint64_t seed, step_hi, seq, draw, p;
    __device__ __forceinline__ void block(uint32_t slot, int j, float (&u)[8]) const {
        const Philox4x64 w = philox4x64_10((uint64_t)j, p, seq, draw, seed, step_hi | (uint64_t)slot);
        u[0] = mol_uniform((uint32_t)(w.w0 >> 32));
        u[1] = mol_uniform((uint32_t)w.w0);
        u[2] = mol_uniform((uint32_t)(w.w1 >> 32));
        u[3] = mol_uniform((uint32_t)w.w1);
        u[4] = mol_uniform((uint32_t)(w.w2 >> 32));
        u[5] = mol_uniform((uint32_t)w.w2);
        u[6] = mol_uniform((uint32_t)(w.w3 >> 32));
        u[7] = mol_uniform((uint32_t)w.w3);
    }
    __device__ __forceinline__ void mix_block(int j, int M, float (&u)[8]) const { block(kMolSlotMix, j, u); }
    template <int C>
    __device__ __forceinline__ void colour(float (&u)[C]) const {
        float v[8];
        block(kMolSlotColour, 0, v);
#pragma unroll
        for (int c = 0; c < C; ++c) u[c] = v[c];
    }
};

// lp: the pixel's first logit (channel stride HW); op: the pixel's first output (channel stride HW)
template <int C, class Uniforms>
__device__ __forceinline__ void mol_sample_pixel(const float* __restrict__ lp, float* __restrict__ op, int M, int HW,
                                                 const Uniforms& src) {
    constexpr int P = C == 3 ? 3 : 2;
    float um[8];
    src.mix_block(0, M, um);
    int best = 0;
    float sc = lp[0] - logf(-logf(um[0]));
    for (int j = 0; 8 * j < M; ++j) {
        if (j) src.mix_block(j, M, um);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int m = 8 * j + e;
            if (m >= 1 && m < M) {
                const float t = lp[(long)m * HW] - logf(-logf(um[e]));
                if (t > sc) {  // strict: the lowest index wins a tie
                    sc = t;
                    best = m;
                }
            }
        }
    }
    float ux[C];
    src.template colour<C>(ux);
    float xs[C], th[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = lp + ((long)M + ((long)c * P) * M + best) * HW;
        const float u = ux[c];
        float v = q[0] + expf(fmaxf(q[(long)M * HW], kMinLogScale)) * (logf(u) - logf(1.0f - u));
        if (C == 3) th[c] = tanhf(q[2L * M * HW]);
        if (C == 3 && c == 1) v += th[0] * xs[0];
        if (C == 3 && c == 2) v += th[1] * xs[0] + th[2] * xs[1];
        xs[c] = fminf(fmaxf(v, -1.0f), 1.0f);
        op[(long)c * HW] = xs[c];
    }
}

// u_mix [N,HW,M], u_x [N,HW,C], out [N,C,HW]
template <int C>
__global__ __launch_bounds__(256) void mol_sample_kernel(const float* __restrict__ l, const float* __restrict__ u_mix,
                                                         const float* __restrict__ u_x, float* __restrict__ out, int M,
                                                         int HW, int nbx) {
    constexpr int P = C == 3 ? 3 : 2;
    const int n = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int p = bx * 256 + threadIdx.x;
    if (p >= HW) return;
    const long Cl = (long)M * (1 + P * C);
    const MolGivenUniforms src{u_mix + ((long)n * HW + p) * M, u_x + ((long)n * HW + p) * C};
    mol_sample_pixel<C>(l + (long)n * Cl * HW + p, out + (long)n * C * HW + p, M, HW, src);
}

struct MolKeyedParams {
    int rows, B, M, HW, nbx;
    uint64_t seed, step_hi, first_seq, first_draw;
};

__device__ __forceinline__ MolKeyedUniforms mol_keyed_source(const MolKeyedParams& k, int n, int p) {
    return MolKeyedUniforms{k.seed, k.step_hi, k.first_seq + (uint64_t)(n % k.B), k.first_draw + (uint64_t)(n / k.B),
                            (uint64_t)p};
}

// the grid and thread layout of mol_sample_kernel; l [rows,Cl,HW], out [rows,C,HW]
template <int C>
__global__ __launch_bounds__(256) void mol_sample_keyed_kernel(const float* __restrict__ l, float* __restrict__ out,
                                                               const MolKeyedParams k) {
    constexpr int P = C == 3 ? 3 : 2;
    const int n = blockIdx.x / k.nbx, bx = blockIdx.x % k.nbx;
    const int p = bx * 256 + threadIdx.x;
    if (p >= k.HW) return;
    const long Cl = (long)k.M * (1 + P * C);
    const MolKeyedUniforms src = mol_keyed_source(k, n, p);
    mol_sample_pixel<C>(l + (long)n * Cl * k.HW + p, out + (long)n * C * k.HW + p, k.M, k.HW, src);
}

// the uniforms mol_sample_keyed_kernel uses, as tensors: u_mix [rows,HW,M], u_x [rows,HW,C]
template <int C>
__global__ __launch_bounds__(256) void mol_keyed_uniforms_kernel(float* __restrict__ u_mix, float* __restrict__ u_x,
                                                                 const MolKeyedParams k) {
    const int n = blockIdx.x / k.nbx, bx = blockIdx.x % k.nbx;
    const int p = bx * 256 + threadIdx.x;
    if (p >= k.HW) return;
    const MolKeyedUniforms src = mol_keyed_source(k, n, p);
    float* um = u_mix + ((long)n * k.HW + p) * k.M;
    float u[8];
    for (int j = 0; 8 * j < k.M; ++j) {
        src.mix_block(j, k.M, u);
        const int left = k.M - 8 * j;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < left) um[8 * j + e] = u[e];
    }
    float ux[C];
    src.template colour<C>(ux);
#pragma unroll
    for (int c = 0; c < C; ++c) u_x[((long)n * k.HW + p) * C + c] = ux[c];
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

static int mol_keyed_params(int rows, int B, int C, int M, int HW, long seed, int step, long first_seq, long first_draw,
                            MolKeyedParams* k, long* blocks) {
    RFN_CHECK_ARG(rows > 0 && B >= 1 && rows % B == 0, -2);
    RFN_CHECK_ARG((C == 1 || C == 3) && M > 0 && HW > 0, -2);
    RFN_CHECK_ARG(seed >= 0 && first_seq >= 0 && first_draw >= 0 && step >= 0, -4);
    int nbx;
    RFN_CHECK_ARG(mol_grid(rows, HW, &nbx, blocks), -3);
    *k = MolKeyedParams{rows, B, M, HW, nbx, (uint64_t)seed, (uint64_t)(uint32_t)step << 32, (uint64_t)first_seq,
                        (uint64_t)first_draw};
    return 0;
}

extern "C" int rfn_mol_sample_keyed(const float* l, float* out, int rows, int B, int C, int M, int HW, long seed, int step,
                                    long first_seq, long first_draw, rfn_stream_t stream) {
    RFN_CHECK_ARG(l && out, -1);
    MolKeyedParams k;
    long blocks;
    if (int rc = mol_keyed_params(rows, B, C, M, HW, seed, step, first_seq, first_draw, &k, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (C == 3)
        hipLaunchKernelGGL(mol_sample_keyed_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, l, out, k);
    else
        hipLaunchKernelGGL(mol_sample_keyed_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, l, out, k);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_mol_keyed_uniforms(float* u_mix, float* u_x, int rows, int B, int C, int M, int HW, long seed, int step,
                                      long first_seq, long first_draw, rfn_stream_t stream) {
    RFN_CHECK_ARG(u_mix && u_x, -1);
    MolKeyedParams k;
    long blocks;
    if (int rc = mol_keyed_params(rows, B, C, M, HW, seed, step, first_seq, first_draw, &k, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (C == 3)
        hipLaunchKernelGGL(mol_keyed_uniforms_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, u_mix, u_x, k);
    else
        hipLaunchKernelGGL(mol_keyed_uniforms_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, u_mix, u_x, k);
    RFN_LAUNCH_CHECK();
    return 0;
}
