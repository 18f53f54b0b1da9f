// Batch-norm flow step (Flow/glow_modules.py:56-104 of the reference) on a step-major time-batched tensor
// x [S*B, E], E = C*H*W: statistics over the B rows of each (step, element), as the reference's per-timestep calls
// compute them.  Streaming passes (gfx950): a thread owns VEC consecutive elements of one step, so the B strided row
// reads of a wave are 64*VEC consecutive floats each; the four waves of a workgroup take the rows b = wave (mod 4) and
// meet in LDS in a fixed order.  A workgroup's slab of x (B rows x 64*VEC floats) is read three times forward (mean,
// variance about the mean, normalise) and twice backward: once from HBM, then from the caches.  No atomics anywhere:
// the sums over elements (log-det) and over steps (parameter gradients, running statistics) go through partials that a
// second small launch adds in index order, so every output repeats bit for bit.
#include "common.h"
#include "../../include/rfn_hip.h"
#include <initializer_list>

namespace {

template <int VEC> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef float4 type; };

template <int VEC> __device__ __forceinline__ void ldv(const float* __restrict__ p, float (&v)[VEC]) {
    const typename Vec<VEC>::type t = *reinterpret_cast<const typename Vec<VEC>::type*>(p);
    __builtin_memcpy(v, &t, sizeof(t));
}
template <int VEC> __device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[VEC]) {
    typename Vec<VEC>::type t;
    __builtin_memcpy(&t, v, sizeof(t));
    *reinterpret_cast<typename Vec<VEC>::type*>(p) = t;
}

// sum over the four row groups (waves) of a workgroup, in wave order; every thread gets the sums of its lane's elements
template <int VEC> __device__ __forceinline__ void rows_sum(float (&a)[VEC], float (*sm)[64 * VEC], int lane, int rg) {
    __syncthreads();  // (the previous round's reads are done)
#pragma unroll
    for (int j = 0; j < VEC; ++j) sm[rg][lane * VEC + j] = a[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        a[j] = ((sm[0][lane * VEC + j] + sm[1][lane * VEC + j]) + sm[2][lane * VEC + j]) + sm[3][lane * VEC + j];
}

// grid (ceil(E / (64*VEC)), S), 256 threads.  part [S][gridDim.x]: this workgroup's share of dl[s].
template <int VEC>
__global__ __launch_bounds__(256) void bnflow_fwd_kernel(const float* __restrict__ x, const float* __restrict__ lg,
                                                         const float* __restrict__ beta, float* __restrict__ z,
                                                         float* __restrict__ mean, float* __restrict__ var,
                                                         float* __restrict__ part, int B, int E, float eps) {
    __shared__ float sm[4][64 * VEC];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6, s = blockIdx.y;
    const long e0 = ((long)blockIdx.x * 64 + lane) * VEC;
    const bool ok = e0 < E;  // E % VEC == 0: a thread's elements are all inside or all outside
    const long base = (long)s * B * E + e0;
    const float invB = 1.0f / (float)B;
    float m[VEC], q[VEC], v[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = q[j] = 0.f;
    if (ok)
        for (int b = rg; b < B; b += 4) {
            ldv<VEC>(x + base + (long)b * E, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) m[j] += v[j];
        }
    rows_sum<VEC>(m, sm, lane, rg);
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] *= invB;
    if (ok)
        for (int b = rg; b < B; b += 4) {
            ldv<VEC>(x + base + (long)b * E, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) q[j] += (v[j] - m[j]) * (v[j] - m[j]);
        }
    rows_sum<VEC>(q, sm, lane, rg);
    float sc[VEC], be[VEC], lgv[VEC];
    if (ok) {
        ldv<VEC>(lg + e0, lgv);
        ldv<VEC>(beta + e0, be);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            q[j] = q[j] * invB + eps;  // eps is INSIDE var (glow_modules.py:78-79), also where the log-det reads it
            sc[j] = expf(lgv[j]) / sqrtf(q[j]);
        }
        for (int b = rg; b < B; b += 4) {
            ldv<VEC>(x + base + (long)b * E, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = (v[j] - m[j]) * sc[j] + be[j];
            stv<VEC>(z + base + (long)b * E, v);
        }
    }
    if (rg == 0) {  // wave-uniform
        float t = 0.f;
        if (ok) {
            stv<VEC>(mean + (long)s * E + e0, m);
            stv<VEC>(var + (long)s * E + e0, q);
#pragma unroll
            for (int j = 0; j < VEC; ++j) t += lgv[j] - 0.5f * logf(q[j]);
        }
        t = wave_sum(t);
        if (lane == 0) part[(long)s * gridDim.x + blockIdx.x] = t;
    }
}

// workgroups 0 .. nrun-1: the S running-statistics updates of the step-wise calls in closed form, one thread per element,
// steps in order; the last workgroup: dl[s] = the partials of step s added in index order.
__global__ __launch_bounds__(256) void bnflow_fwd_finish_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                                const float* __restrict__ part, float* __restrict__ dl,
                                                                float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                const float* __restrict__ coef_m,
                                                                const float* __restrict__ coef_v, float decay, int S, int E,
                                                                int nbx, int nrun) {
    if ((int)blockIdx.x < nrun) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= E) return;
        float rm = decay * run_mean[e], rv = decay * run_var[e];
        for (int s = 0; s < S; ++s) {
            rm = fmaf(coef_m[s], mean[(long)s * E + e], rm);
            rv = fmaf(coef_v[s], var[(long)s * E + e], rv);
        }
        run_mean[e] = rm;
        run_var[e] = rv;
        return;
    }
    for (int s = threadIdx.x; s < S; s += 256) {
        float t = 0.f;
        for (int i = 0; i < nbx; ++i) t += part[(long)s * nbx + i];
        dl[s] = t;
    }
}

// same grid as the forward.  sums [S][2][E]: per-step partials of (g_log_gamma, g_beta).
template <int VEC>
__global__ __launch_bounds__(256) void bnflow_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lg,
                                                         const float* __restrict__ gz, const float* __restrict__ gdl,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         float* __restrict__ gx, float* __restrict__ sums, int B, int E) {
    __shared__ float sm[4][64 * VEC];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6, s = blockIdx.y;
    const long e0 = ((long)blockIdx.x * 64 + lane) * VEC;
    const bool ok = e0 < E;
    const long base = (long)s * B * E + e0;
    const float invB = 1.0f / (float)B, gd = gdl ? gdl[s] : 0.f;
    float m[VEC], rstd[VEC], eg[VEC], sg[VEC], sgx[VEC], v[VEC], g[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) sg[j] = sgx[j] = m[j] = rstd[j] = eg[j] = 0.f;
    if (ok) {
        ldv<VEC>(mean + (long)s * E + e0, m);
        ldv<VEC>(var + (long)s * E + e0, rstd);
        ldv<VEC>(lg + e0, eg);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            rstd[j] = 1.0f / sqrtf(rstd[j]);
            eg[j] = expf(eg[j]);
        }
        for (int b = rg; b < B; b += 4) {
            ldv<VEC>(x + base + (long)b * E, v);
            ldv<VEC>(gz + base + (long)b * E, g);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                sg[j] += g[j];
                sgx[j] += g[j] * ((v[j] - m[j]) * rstd[j]);
            }
        }
    }
    rows_sum<VEC>(sg, sm, lane, rg);
    rows_sum<VEC>(sgx, sm, lane, rg);
    if (!ok) return;  // (after the last barrier)
    if (rg == 0) {
        float t[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = eg[j] * sgx[j] + gd;  // sum_b g' xhat + gdl[s]
        stv<VEC>(sums + ((long)s * 2 + 0) * E + e0, t);
        stv<VEC>(sums + ((long)s * 2 + 1) * E + e0, sg);            // sum_b gz
    }
    for (int b = rg; b < B; b += 4) {
        ldv<VEC>(x + base + (long)b * E, v);
        ldv<VEC>(gz + base + (long)b * E, g);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float xh = (v[j] - m[j]) * rstd[j];
            // the second term: the log-det depends on the data through var
            v[j] = rstd[j] * (eg[j] * (g[j] - sg[j] * invB - xh * (sgx[j] * invB))) - gd * xh * rstd[j] * invB;
        }
        stv<VEC>(gx + base + (long)b * E, v);
    }
}

__global__ __launch_bounds__(256) void bnflow_bwd_reduce_kernel(const float* __restrict__ sums, float* __restrict__ g_lg,
                                                                float* __restrict__ g_beta, int S, int E) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float a = 0.f, b = 0.f;
    for (int s = 0; s < S; ++s) {  // steps in order
        a += sums[((long)s * 2 + 0) * E + e];
        b += sums[((long)s * 2 + 1) * E + e];
    }
    g_lg[e] = a;
    g_beta[e] = b;
}

// workgroups 0 .. nbx*ny-1: column block bx = id % nbx of the rows by = id / nbx, by + ny, ...; the last workgroup: dl.
template <int VEC>
__global__ __launch_bounds__(256) void bnflow_apply_kernel(const float* __restrict__ x, const float* __restrict__ lg,
                                                           const float* __restrict__ beta, const float* __restrict__ rm,
                                                           const float* __restrict__ rv, float* __restrict__ y,
                                                           float* __restrict__ dl, int N, int E, int reverse, int nbx,
                                                           int ny) {
    __shared__ float sm[4];
    if ((int)blockIdx.x == nbx * ny) {
        float t = 0.f;
        for (int e = threadIdx.x; e < E; e += 256) t += lg[e] - 0.5f * logf(rv[e]);
        t = block_sum_256(t, sm);
        if (threadIdx.x == 0) dl[0] = reverse ? -t : t;
        return;
    }
    const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
    const long e0 = ((long)bx * 256 + threadIdx.x) * VEC;
    if (e0 >= E) return;
    float a[VEC], sub[VEC], add[VEC], t0[VEC], t1[VEC], v[VEC];
    ldv<VEC>(lg + e0, a);
    ldv<VEC>(rv + e0, v);
    ldv<VEC>(beta + e0, t0);
    ldv<VEC>(rm + e0, t1);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const float eg = expf(a[j]), sd = sqrtf(v[j]);
        a[j] = reverse ? sd / eg : eg / sd;
        sub[j] = reverse ? t0[j] : t1[j];
        add[j] = reverse ? t1[j] : t0[j];
    }
    for (int n = by; n < N; n += ny) {
        ldv<VEC>(x + (long)n * E + e0, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (v[j] - sub[j]) * a[j] + add[j];
        stv<VEC>(y + (long)n * E + e0, v);
    }
}

bool all16(std::initializer_list<const void*> ps) {
    uintptr_t m = 0;
    for (const void* p : ps) m |= (uintptr_t)p;
    return (m & 15) == 0;
}

}  // namespace

// floats of scratch rfn_bnflow_fwd_f32 (bwd = 0: log-det partials, one per workgroup, S * ceil(E/64) on the 4-byte
// route and fewer on the 16-byte one) / rfn_bnflow_bwd_f32 (bwd = 1: per-step parameter-gradient partials, 2*S*E) needs
extern "C" long rfn_bnflow_scratch_floats(int S, int B, int E, int bwd) {
    if (S <= 0 || B <= 0 || E <= 0) return 0;
    return bwd ? 2L * S * E : (long)S * ceil_div(E, 64);
}

extern "C" int rfn_bnflow_fwd_f32(const float* x, const float* log_gamma, const float* beta, float* z, float* mean,
                                  float* var, float* dl, float* scratch, float* run_mean, float* run_var,
                                  const float* coef_mean, const float* coef_var, float decay, int S, int B, int E, float eps,
                                  rfn_stream_t stream) {
    RFN_CHECK_ARG(x && log_gamma && beta && z && mean && var && dl && scratch && S > 0 && B > 0 && E > 0, -1);
    RFN_CHECK_ARG((run_mean && run_var && coef_mean && coef_var) || (!run_mean && !run_var), -2);
    RFN_CHECK_ARG(S <= 65535, -3);
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = E % 4 == 0 && all16({x, log_gamma, beta, z, mean, var});
    const int nbx = ceil_div(E, v4 ? 256 : 64);
    if (v4)
        hipLaunchKernelGGL(bnflow_fwd_kernel<4>, dim3(nbx, S), dim3(256), 0, st, x, log_gamma, beta, z, mean, var, scratch,
                           B, E, eps);
    else
        hipLaunchKernelGGL(bnflow_fwd_kernel<1>, dim3(nbx, S), dim3(256), 0, st, x, log_gamma, beta, z, mean, var, scratch,
                           B, E, eps);
    const int nrun = run_mean ? ceil_div(E, 256) : 0;
    hipLaunchKernelGGL(bnflow_fwd_finish_kernel, dim3(nrun + 1), dim3(256), 0, st, mean, var, scratch, dl, run_mean,
                       run_var, coef_mean, coef_var, decay, S, E, nbx, nrun);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_bnflow_bwd_f32(const float* x, const float* log_gamma, const float* gz, const float* gdl,
                                  const float* mean, const float* var, float* gx, float* g_log_gamma, float* g_beta,
                                  float* scratch, int S, int B, int E, rfn_stream_t stream) {
    RFN_CHECK_ARG(x && log_gamma && gz && mean && var && gx && g_log_gamma && g_beta && scratch, -1);
    RFN_CHECK_ARG(S > 0 && S <= 65535 && B > 0 && E > 0, -3);
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = E % 4 == 0 && all16({x, log_gamma, gz, mean, var, gx, scratch});
    const int nbx = ceil_div(E, v4 ? 256 : 64);
    if (v4)
        hipLaunchKernelGGL(bnflow_bwd_kernel<4>, dim3(nbx, S), dim3(256), 0, st, x, log_gamma, gz, gdl, mean, var, gx,
                           scratch, B, E);
    else
        hipLaunchKernelGGL(bnflow_bwd_kernel<1>, dim3(nbx, S), dim3(256), 0, st, x, log_gamma, gz, gdl, mean, var, gx,
                           scratch, B, E);
    hipLaunchKernelGGL(bnflow_bwd_reduce_kernel, dim3(ceil_div(E, 256)), dim3(256), 0, st, scratch, g_log_gamma, g_beta, S,
                       E);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_bnflow_apply_f32(const float* x, const float* log_gamma, const float* beta, const float* run_mean,
                                    const float* run_var, float* y, float* dl, int N, int E, int reverse,
                                    rfn_stream_t stream) {
    RFN_CHECK_ARG(x && log_gamma && beta && run_mean && run_var && y && dl && N > 0 && E > 0, -1);
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = E % 4 == 0 && all16({x, log_gamma, beta, run_mean, run_var, y});
    const int nbx = ceil_div(E, v4 ? 1024 : 256);
    int ny = ceil_div(2048, nbx);  // about 2048 streaming workgroups at most; the rows beyond them by stride
    if (ny > N) ny = N;
    if (v4)
        hipLaunchKernelGGL(bnflow_apply_kernel<4>, dim3(nbx * ny + 1), dim3(256), 0, st, x, log_gamma, beta, run_mean,
                           run_var, y, dl, N, E, reverse, nbx, ny);
    else
        hipLaunchKernelGGL(bnflow_apply_kernel<1>, dim3(nbx * ny + 1), dim3(256), 0, st, x, log_gamma, beta, run_mean,
                           run_var, y, dl, N, E, reverse, nbx, ny);
    RFN_LAUNCH_CHECK();
    return 0;
}
