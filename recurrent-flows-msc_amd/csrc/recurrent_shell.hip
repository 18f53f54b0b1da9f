// The elementwise shell of the recurrent part (gfx950): the SRNN latent step (softplus, both rsamples, KL) and the
// ConvLSTM gate update, forward and backward, with their launch-label queries.  Called by rfn_hip.ops (RFN and SRNN).
#include "common.h"
#include "../../include/rfn_hip.h"

// ------------------------------------------------------------------------------------------------ SRNN latent step
// RFN.loss per timestep (RFN_new.py:167-184,206-207): enc / pri are the outputs [B, 2*Z, HW] of the encoder / prior
// parameter convs (loc | raw scale, "chunk(2,1)" halves, SimpleParamNet.forward Utils/modules.py:240-244):
//   ps = softplus(pri_raw), es = softplus(enc_raw), pm = pri_loc, em = enc_loc (+ pm with res_q)
//   zt = pm + ps*eps_p ;  zxt = em + es*eps_q ;  kl = KL(N(em,es) || N(pm,ps)) element-wise
// One launch instead of ~25 tiny elementwise kernels per timestep (and ~50 in backward).
// grid of an elementwise grid-stride kernel of 256 threads: one thread per element up to `cap` workgroups (the latent
// step and ConvLSTM gate launchers launch this; their label queries print it)
struct StrideRoute {
    int grid;    // workgroups
    int sweeps;  // most grid-stride iterations of a thread
};
static StrideRoute choose_stride_grid(long tot, int cap) {
    StrideRoute r;
    const long blocks = (tot + 255) / 256;
    r.grid = (int)(blocks < cap ? blocks : cap);
    r.sweeps = (int)((blocks + r.grid - 1) / r.grid);
    return r;
}
constexpr int LATENT_STEP_MAX_GRID = 1024, CONVLSTM_GATES_MAX_GRID = 2048;
extern "C" const char* rfn_latent_step_kernel_label(int B, int ZHW) {
    static thread_local char buf[96];
    if (B <= 0 || ZHW <= 0) return "unsupported";
    const StrideRoute r = choose_stride_grid((long)B * ZHW, LATENT_STEP_MAX_GRID);
    snprintf(buf, sizeof(buf), "latent_step grid=%d sweeps=%d", r.grid, r.sweeps);
    return buf;
}
extern "C" const char* rfn_convlstm_gates_kernel_label(int N, int Hc, int HW) {
    static thread_local char buf[96];
    if (N <= 0 || Hc <= 0 || HW <= 0) return "unsupported";
    const StrideRoute r = choose_stride_grid((long)N * Hc * HW, CONVLSTM_GATES_MAX_GRID);
    snprintf(buf, sizeof(buf), "convlstm_gates grid=%d sweeps=%d", r.grid, r.sweeps);
    return buf;
}

__device__ __forceinline__ float sigmoid_sp(float raw) { return raw > 20.f ? 1.f : 1.f / (1.f + expf(-raw)); }

__global__ void latent_step_fwd_kernel(const float* __restrict__ enc, const float* __restrict__ pri,
                                       const float* __restrict__ eps_p, const float* __restrict__ eps_q,
                                       float* __restrict__ zt, float* __restrict__ zxt, float* __restrict__ kl,
                                       float* __restrict__ em_o, float* __restrict__ es_o, int B, int ZHW, int res_q) {
    const long total = (long)B * ZHW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / ZHW, e = idx - b * ZHW;
        const float pm = pri[b * 2 * ZHW + e], ps = softplusf_(pri[b * 2 * ZHW + ZHW + e]);
        const float es = softplusf_(enc[b * 2 * ZHW + ZHW + e]);
        const float em = enc[b * 2 * ZHW + e] + (res_q ? pm : 0.f);
        zt[idx] = pm + ps * eps_p[idx];
        zxt[idx] = em + es * eps_q[idx];
        const float r = es / ps, d = (em - pm) / ps;
        kl[idx] = 0.5f * (r * r + d * d - 1.f - logf(r * r));
        em_o[idx] = em;
        es_o[idx] = es;
    }
}
__global__ void latent_step_bwd_kernel(const float* __restrict__ enc, const float* __restrict__ pri,
                                       const float* __restrict__ eps_p, const float* __restrict__ eps_q,
                                       const float* __restrict__ g_zt, long g_zt_ns,
                                       const float* __restrict__ g_zxt, long g_zxt_ns,
                                       const float* __restrict__ g_kl, const float* __restrict__ g_em,
                                       const float* __restrict__ g_es, float* __restrict__ g_enc,
                                       float* __restrict__ g_pri, int B, int ZHW, int res_q) {
    const long total = (long)B * ZHW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / ZHW, e = idx - b * ZHW;
        const float praw = pri[b * 2 * ZHW + ZHW + e], eraw = enc[b * 2 * ZHW + ZHW + e];
        const float pm = pri[b * 2 * ZHW + e], ps = softplusf_(praw), es = softplusf_(eraw);
        const float em = enc[b * 2 * ZHW + e] + (res_q ? pm : 0.f);
        const float gzt = g_zt ? g_zt[b * g_zt_ns + e] : 0.f, gzx = g_zxt ? g_zxt[b * g_zxt_ns + e] : 0.f;
        const float gk = g_kl ? g_kl[idx] : 0.f;
        const float ips = 1.f / ps, d = (em - pm) * ips * ips;  // (em-pm)/ps^2
        const float d_em = gzx + gk * d + (g_em ? g_em[idx] : 0.f);
        const float d_es = gzx * eps_q[idx] + gk * (es * ips * ips - 1.f / es) + (g_es ? g_es[idx] : 0.f);
        float d_pm = gzt - gk * d;
        const float d_ps = gzt * eps_p[idx] + gk * (ips - (es * es + (em - pm) * (em - pm)) * ips * ips * ips);
        if (res_q) d_pm += d_em;
        g_enc[b * 2 * ZHW + e] = d_em;
        g_enc[b * 2 * ZHW + ZHW + e] = d_es * sigmoid_sp(eraw);
        g_pri[b * 2 * ZHW + e] = d_pm;
        g_pri[b * 2 * ZHW + ZHW + e] = d_ps * sigmoid_sp(praw);
    }
}
extern "C" int rfn_latent_step_fwd_f32(const float* enc, const float* pri, const float* eps_p, const float* eps_q,
                                       float* zt, float* zxt, float* kl, float* em, float* es, int B, int ZHW,
                                       int res_q, rfn_stream_t stream) {
    RFN_CHECK_ARG(enc && pri && eps_p && eps_q && zt && zxt && kl && em && es && B >= 0 && ZHW > 0, -1);
    if (B == 0) return 0;
    const int grid = choose_stride_grid((long)B * ZHW, LATENT_STEP_MAX_GRID).grid;
    hipLaunchKernelGGL(latent_step_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, enc, pri, eps_p, eps_q, zt,
                       zxt, kl, em, es, B, ZHW, res_q);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_latent_step_bwd_f32(const float* enc, const float* pri, const float* eps_p, const float* eps_q,
                                       const float* g_zt, long g_zt_ns, const float* g_zxt, long g_zxt_ns,
                                       const float* g_kl, const float* g_em, const float* g_es, float* g_enc,
                                       float* g_pri, int B, int ZHW, int res_q, rfn_stream_t stream) {
    RFN_CHECK_ARG(enc && pri && eps_p && eps_q && g_enc && g_pri && B >= 0 && ZHW > 0, -1);
    RFN_CHECK_ARG((!g_zt || g_zt_ns >= ZHW) && (!g_zxt || g_zxt_ns >= ZHW), -1);
    if (B == 0) return 0;
    const int grid = choose_stride_grid((long)B * ZHW, LATENT_STEP_MAX_GRID).grid;
    hipLaunchKernelGGL(latent_step_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, enc, pri, eps_p, eps_q,
                       g_zt, g_zt_ns, g_zxt, g_zxt_ns, g_kl, g_em, g_es, g_enc, g_pri, B, ZHW, res_q);
    RFN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ ConvLSTM gates
__global__ void convlstm_gates_fwd_kernel(const float* __restrict__ cc, const float* __restrict__ c_prev, long c_ns,
                                          const float* __restrict__ Wci, const float* __restrict__ Wcf,
                                          const float* __restrict__ Wco, float* __restrict__ h_out, long h_ns,
                                          float* __restrict__ c_out, long co_ns, float* __restrict__ gates, int N,
                                          int Hc, int HW) {
    const long per = (long)Hc * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)N * per;
         idx += (long)gridDim.x * blockDim.x) {
        int n = (int)(idx / per);
        long e = idx - n * per;  // channel*HW + p
        const float* ccn = cc + (long)n * 4 * per;
        float cp = c_prev[n * c_ns + e];
        float wi = Wci ? Wci[e] : 0.f, wf = Wcf ? Wcf[e] : 0.f, wo = Wco ? Wco[e] : 0.f;
        float i = 1.f / (1.f + expf(-(ccn[e] + wi * cp)));
        float f = 1.f / (1.f + expf(-(ccn[per + e] + wf * cp)));
        float g = tanhf(ccn[3 * per + e]);
        float cn = f * cp + i * g;
        float o = 1.f / (1.f + expf(-(ccn[2 * per + e] + wo * cn)));
        h_out[n * h_ns + e] = o * tanhf(cn);
        c_out[n * co_ns + e] = cn;
        if (gates) {
            float* gn = gates + (long)n * 4 * per;
            gn[e] = i;
            gn[per + e] = f;
            gn[2 * per + e] = o;
            gn[3 * per + e] = g;
        }
    }
}
extern "C" int rfn_convlstm_gates_fwd_f32(const float* cc, const float* c_prev, long c_ns, const float* Wci,
                                          const float* Wcf, const float* Wco, float* h_out, long h_ns, float* c_out,
                                          long co_ns, float* gates, int N, int Hc, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(cc && c_prev && h_out && c_out && N >= 0 && Hc > 0 && HW > 0, -1);
    if (N == 0) return 0;
    const int grid = choose_stride_grid((long)N * Hc * HW, CONVLSTM_GATES_MAX_GRID).grid;
    hipLaunchKernelGGL(convlstm_gates_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, cc, c_prev, c_ns, Wci,
                       Wcf, Wco, h_out, h_ns, c_out, co_ns, gates, N, Hc, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}

__global__ void convlstm_gates_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ c_prev, long c_ns,
                                          const float* __restrict__ c_out, long co_ns, const float* __restrict__ gh,
                                          long gh_ns, const float* __restrict__ gc_next, long gcn_ns,
                                          const float* __restrict__ Wci, const float* __restrict__ Wcf,
                                          const float* __restrict__ Wco, float* __restrict__ gcc,
                                          float* __restrict__ gc_prev, long gcp_ns, int N, int Hc, int HW) {
    const long per = (long)Hc * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)N * per;
         idx += (long)gridDim.x * blockDim.x) {
        int n = (int)(idx / per);
        long e = idx - n * per;
        const float* gn = gates + (long)n * 4 * per;
        float i = gn[e], f = gn[per + e], o = gn[2 * per + e], g = gn[3 * per + e];
        float cp = c_prev[n * c_ns + e];
        float cn = c_out[n * co_ns + e];
        float wi = Wci ? Wci[e] : 0.f, wf = Wcf ? Wcf[e] : 0.f, wo = Wco ? Wco[e] : 0.f;
        float ghv = gh ? gh[n * gh_ns + e] : 0.f;
        float gcn = gc_next ? gc_next[n * gcn_ns + e] : 0.f;
        float tc = tanhf(cn);
        float go_pre = ghv * tc * o * (1.f - o);  // grad wrt (cc_o + Wco*cn)
        float gc = gcn + ghv * o * (1.f - tc * tc) + go_pre * wo;
        float gi_pre = gc * g * i * (1.f - i);
        float gf_pre = gc * cp * f * (1.f - f);
        float gg_pre = gc * i * (1.f - g * g);
        float* gccn = gcc + (long)n * 4 * per;
        gccn[e] = gi_pre;
        gccn[per + e] = gf_pre;
        gccn[2 * per + e] = go_pre;
        gccn[3 * per + e] = gg_pre;
        gc_prev[n * gcp_ns + e] = gc * f + gi_pre * wi + gf_pre * wf;
    }
}
extern "C" int rfn_convlstm_gates_bwd_f32(const float* gates, const float* c_prev, long c_ns, const float* c_out,
                                          long co_ns, const float* gh, long gh_ns, const float* gc_next, long gcn_ns,
                                          const float* Wci, const float* Wcf, const float* Wco, float* gcc,
                                          float* gc_prev, long gcp_ns, int N, int Hc, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(gates && c_prev && c_out && gcc && gc_prev && N >= 0 && Hc > 0 && HW > 0, -1);
    if (N == 0) return 0;
    const int grid = choose_stride_grid((long)N * Hc * HW, CONVLSTM_GATES_MAX_GRID).grid;
    hipLaunchKernelGGL(convlstm_gates_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, gates, c_prev, c_ns,
                       c_out, co_ns, gh, gh_ns, gc_next, gcn_ns, Wci, Wcf, Wco, gcc, gc_prev, gcp_ns, N, Hc, HW);
    RFN_LAUNCH_CHECK();
    return 0;
}
