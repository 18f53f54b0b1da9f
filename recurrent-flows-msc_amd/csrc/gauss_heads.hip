// The diagonal Gaussians of one VRNN time step (VRNN/VRNN.py:203-213,223 of the reference in `loss`, :383-394,419-420 in
// `elbo_importance_weighting`, :290-294 in generation): from the four MLP outputs [B, Z] (loc and raw scale of the encoder
// q and of the prior p) and the standard normals to both samples, the scales, the row-summed KL(q || p) and the row-summed
// log-densities of each distribution at its OWN sample -- about twenty torch launches on B*Z numbers as one kernel each
// way.  sigma = softplus(raw) as torch.nn.Softplus() computes it (raw itself above 20); nothing is added to it.
//
// One wavefront per row, RFN_GH_ROWS rows per workgroup.  Lane l takes the elements l, l + 64, ... of its row and adds its
// terms in index order; the 64 lane sums are combined by the xor butterfly of wave_sum (offsets 32, 16, ..., 1: register
// shuffles, every lane ends with the same bits).  No atomics, no LDS memory: a row's bits depend on that row alone.
#include "common.h"
#include "../../include/rfn_hip.h"

constexpr int RFN_GH_ROWS = 4;  // waves (= rows) per workgroup of 256 threads

__device__ __forceinline__ float gh_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }  // torch threshold = 20
__device__ __forceinline__ float gh_logistic(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
constexpr float RFN_GH_HALF_LOG_2PI = 0.91893853320467274178f;

// Every pointer but p_loc / p_raw may be null (wave-uniform branches).  The launcher has checked that an output's inputs
// are there.
__global__ void __launch_bounds__(64 * RFN_GH_ROWS)
gauss_heads_fwd_kernel(const float* __restrict__ q_loc, const float* __restrict__ q_raw, const float* __restrict__ p_loc,
                       const float* __restrict__ p_raw, const float* __restrict__ eps_q, const float* __restrict__ eps_p,
                       float* __restrict__ z_q, float* __restrict__ z_p, float* __restrict__ q_scale,
                       float* __restrict__ p_scale, float* __restrict__ kl, float* __restrict__ logq,
                       float* __restrict__ logp, int B, int Z) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * RFN_GH_ROWS + (threadIdx.x >> 6);
    if (b >= B) return;  // whole waves leave: no shuffle below is divergent
    const long row = b * Z;
    float s_kl = 0.f, s_lq = 0.f, s_lp = 0.f;
    for (int j = lane; j < Z; j += 64) {
        const long i = row + j;
        const float pm = p_loc[i], ps = gh_softplus(p_raw[i]);
        const float lps = logf(ps);
        if (p_scale) p_scale[i] = ps;
        if (eps_p) {
            const float e = eps_p[i];
            if (z_p) z_p[i] = pm + ps * e;
            s_lp += -0.5f * e * e - lps - RFN_GH_HALF_LOG_2PI;
        }
        if (q_loc) {
            const float qm = q_loc[i], qs = gh_softplus(q_raw[i]);
            const float lqs = logf(qs);
            if (q_scale) q_scale[i] = qs;
            if (eps_q) {
                const float e = eps_q[i];
                if (z_q) z_q[i] = qm + qs * e;
                s_lq += -0.5f * e * e - lqs - RFN_GH_HALF_LOG_2PI;
            }
            const float a = qs / ps, d = (qm - pm) / ps;
            s_kl += 0.5f * (a * a + d * d - 1.f) - (lqs - lps);
        }
    }
    if (kl) {
        s_kl = wave_sum(s_kl);
        if (lane == 0) kl[b] = s_kl;
    }
    if (logq) {
        s_lq = wave_sum(s_lq);
        if (lane == 0) logq[b] = s_lq;
    }
    if (logp) {
        s_lp = wave_sum(s_lp);
        if (lane == 0) logp[b] = s_lp;
    }
}

// gradient of the formulas above; sigma is recomputed from the raw inputs.  g_zq / g_zp: row stride in floats.
__global__ void __launch_bounds__(64 * RFN_GH_ROWS)
gauss_heads_bwd_kernel(const float* __restrict__ q_loc, const float* __restrict__ q_raw, const float* __restrict__ p_loc,
                       const float* __restrict__ p_raw, const float* __restrict__ eps_q, const float* __restrict__ eps_p,
                       const float* __restrict__ g_zq, long g_zq_ns, const float* __restrict__ g_zp, long g_zp_ns,
                       const float* __restrict__ g_kl, const float* __restrict__ g_logq,
                       const float* __restrict__ g_logp, float* __restrict__ g_q_loc, float* __restrict__ g_q_raw,
                       float* __restrict__ g_p_loc, float* __restrict__ g_p_raw, int B, int Z) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * RFN_GH_ROWS + (threadIdx.x >> 6);
    if (b >= B) return;
    const long row = b * Z;
    const float gk = g_kl ? g_kl[b] : 0.f, glq = g_logq ? g_logq[b] : 0.f, glp = g_logp ? g_logp[b] : 0.f;
    for (int j = lane; j < Z; j += 64) {
        const long i = row + j;
        const float praw = p_raw[i];
        const float pm = p_loc[i], ps = gh_softplus(praw), ips = 1.f / ps;
        const float gzp = g_zp ? g_zp[b * g_zp_ns + j] : 0.f;
        float d_pm = gzp, d_ps = -glp * ips;
        if (eps_p) d_ps += gzp * eps_p[i];
        if (q_loc) {
            const float qraw = q_raw[i];
            const float qm = q_loc[i], qs = gh_softplus(qraw), iqs = 1.f / qs;
            const float gzq = g_zq ? g_zq[b * g_zq_ns + j] : 0.f;
            const float a = qs * ips, d = (qm - pm) * ips;
            const float d_qm = gzq + gk * d * ips;
            float d_qs = gk * (a * ips - iqs) - glq * iqs;
            if (eps_q) d_qs += gzq * eps_q[i];
            d_pm -= gk * d * ips;
            d_ps += gk * (1.f - a * a - d * d) * ips;
            g_q_loc[i] = d_qm;
            g_q_raw[i] = d_qs * gh_logistic(qraw);
        }
        g_p_loc[i] = d_pm;
        g_p_raw[i] = d_ps * gh_logistic(praw);
    }
}

extern "C" int rfn_gauss_heads_fwd_f32(const float* q_loc, const float* q_raw, const float* p_loc, const float* p_raw,
                                       const float* eps_q, const float* eps_p, float* z_q, float* z_p, float* q_scale,
                                       float* p_scale, float* kl, float* logq, float* logp, int B, int Z,
                                       rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 1 && Z >= 1, -1);
    RFN_CHECK_ARG(p_loc && p_raw, -1);
    RFN_CHECK_ARG((q_loc != nullptr) == (q_raw != nullptr), -1);
    // an output whose inputs are missing
    RFN_CHECK_ARG(q_loc || !(z_q || q_scale || kl || logq || eps_q), -2);
    RFN_CHECK_ARG(eps_q || !(z_q || logq), -2);
    RFN_CHECK_ARG(eps_p || !(z_p || logp), -2);
    hipLaunchKernelGGL(gauss_heads_fwd_kernel, dim3((unsigned)ceil_div(B, RFN_GH_ROWS)), dim3(64 * RFN_GH_ROWS), 0,
                       (hipStream_t)stream, q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, z_q, z_p, q_scale, p_scale, kl, logq,
                       logp, B, Z);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_gauss_heads_bwd_f32(const float* q_loc, const float* q_raw, const float* p_loc, const float* p_raw,
                                       const float* eps_q, const float* eps_p, const float* g_zq, long g_zq_ns,
                                       const float* g_zp, long g_zp_ns, const float* g_kl, const float* g_logq,
                                       const float* g_logp, float* g_q_loc, float* g_q_raw, float* g_p_loc,
                                       float* g_p_raw, int B, int Z, rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 1 && Z >= 1, -1);
    RFN_CHECK_ARG(p_loc && p_raw && g_p_loc && g_p_raw, -1);
    RFN_CHECK_ARG((q_loc != nullptr) == (q_raw != nullptr), -1);
    RFN_CHECK_ARG((q_loc != nullptr) == (g_q_loc != nullptr) && (q_loc != nullptr) == (g_q_raw != nullptr), -1);
    // an upstream gradient of an output the forward could not have given
    RFN_CHECK_ARG(q_loc || !(g_zq || g_kl || g_logq || eps_q), -2);
    RFN_CHECK_ARG(eps_q || !(g_zq || g_logq), -2);
    RFN_CHECK_ARG(eps_p || !(g_zp || g_logp), -2);
    RFN_CHECK_ARG((!g_zq || g_zq_ns >= Z) && (!g_zp || g_zp_ns >= Z), -3);
    hipLaunchKernelGGL(gauss_heads_bwd_kernel, dim3((unsigned)ceil_div(B, RFN_GH_ROWS)), dim3(64 * RFN_GH_ROWS), 0,
                       (hipStream_t)stream, q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, g_zq, g_zq_ns, g_zp, g_zp_ns, g_kl,
                       g_logq, g_logp, g_q_loc, g_q_raw, g_p_loc, g_p_raw, B, Z);
    RFN_LAUNCH_CHECK();
    return 0;
}
