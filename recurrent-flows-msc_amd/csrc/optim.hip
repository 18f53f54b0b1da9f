// Adam (Kingma & Ba; torch.optim.Adam's arithmetic, RFN/trainer.py:96 of the reference builds it with defaults) over ALL
// parameter tensors of the model in one launch.  The step is memory bound: 28 bytes per parameter (p, g, m, v read; p, m,
// v written), 1.0 GB for the canonical RFN; at::native's fused multi-tensor kernel needs 35 launches of <= 4 KB argument
// tables for the 1269 tensors and reaches ~0.85 TB/s.  Here the table lives in device memory (built once while the
// gradient tensors are static, i.e. in hipGraph mode) and a flat chunk list maps workgroups to (tensor, offset).
#include "common.h"
#include "../../include/rfn_hip.h"

static_assert(sizeof(rfn_adam_entry) == 48, "rfn_adam_entry layout is part of the ABI");

constexpr int ADAM_THREADS = 256;

// One body for the plain and the guarded step: GUARDED multiplies every gradient by `scale` before weight decay (torch
// clips before the optimizer sees the gradient) and counts `skipped` steps out of the bias corrections.  The plain
// instantiation is the kernel as it was; with scale == 1.0f the product is exact, so whatever the compiler contracts it
// into rounds as the plain kernel does.
//
// EMA folds the Polyak average of the weights into the same pass: after the update of the tensor's n-th applied step,
// ema <- ema + w (p_new - ema) with w = 1 - min(decay, (1 + n) / (10 + n)), formed in double and rounded once like w1 and
// w2.  p_new is still in registers, so the average costs one more read and one more write per element (36 bytes against
// 28).  The update of p, m, v is the same expression in all four instantiations: their bits do not depend on EMA.
template <bool GUARDED, bool EMA>
__device__ __forceinline__ void adam_chunk(const rfn_adam_entry* __restrict__ tab, const int2* __restrict__ chunks,
                                           int chunk_elems, double lr, double beta1d, double beta2d, float eps,
                                           float weight_decay, int t, float scale, int skipped, double ema_decay,
                                           float* const* __restrict__ ema_tab) {
    __shared__ float s_step_size, s_bc2_sqrt, s_ema_w;
    const int2 ck = chunks[blockIdx.x];
    const rfn_adam_entry e = tab[ck.x];
    if (threadIdx.x == 0) {
        const double step = (double)(t - e.step_offset - skipped);
        s_step_size = (float)(lr / (1.0 - pow(beta1d, step)));
        s_bc2_sqrt = (float)sqrt(1.0 - pow(beta2d, step));
        if constexpr (EMA) {
            const double warm = (1.0 + step) / (10.0 + step);
            s_ema_w = (float)(1.0 - (ema_decay < warm ? ema_decay : warm));
        }
    }
    __syncthreads();
    // 1 - beta in double, then rounded: 1.f - (float)0.999 is off by 1.3e-5 relative
    const float step_size = s_step_size, bc2_sqrt = s_bc2_sqrt, w1 = (float)(1.0 - beta1d), w2 = (float)(1.0 - beta2d);
    const float beta2 = (float)beta2d;
    const long base = (long)ck.y * chunk_elems;
    const long rem = e.n - base;
    const int n = (int)(rem < chunk_elems ? rem : chunk_elems);
    float* __restrict__ p = e.p + base;
    const float* __restrict__ g = e.g + base;
    float* __restrict__ m = e.m + base;
    float* __restrict__ v = e.v + base;
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        if constexpr (GUARDED) gg = scale * gg;
        if (weight_decay != 0.f) gg = fmaf(weight_decay, pp, gg);
        mm = fmaf(w1, gg - mm, mm);
        vv = fmaf(w2 * gg, gg, beta2 * vv);
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        pp -= step_size * (mm / denom);
    };
    float* __restrict__ a = nullptr;   // the average (EMA only)
    float ema_w = 0.f;
    if constexpr (EMA) {
        a = ema_tab[ck.x] + base;
        ema_w = s_ema_w;
    }
    auto avg = [&](float& aa, float pp) { aa = fmaf(ema_w, pp - aa, aa); };
    const bool v4 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)a) & 15) == 0);
    int i0 = 0;
    if (v4) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
            float4 pp = reinterpret_cast<float4*>(p)[i];
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            float4 mm = reinterpret_cast<float4*>(m)[i];
            float4 vv = reinterpret_cast<float4*>(v)[i];
            upd(pp.x, gg.x, mm.x, vv.x);
            upd(pp.y, gg.y, mm.y, vv.y);
            upd(pp.z, gg.z, mm.z, vv.z);
            upd(pp.w, gg.w, mm.w, vv.w);
            reinterpret_cast<float4*>(p)[i] = pp;
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
            if constexpr (EMA) {
                float4 aa = reinterpret_cast<float4*>(a)[i];
                avg(aa.x, pp.x);
                avg(aa.y, pp.y);
                avg(aa.z, pp.z);
                avg(aa.w, pp.w);
                reinterpret_cast<float4*>(a)[i] = aa;
            }
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < n; i += ADAM_THREADS) {
        float pp = p[i], mm = m[i], vv = v[i];
        upd(pp, g[i], mm, vv);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if constexpr (EMA) {
            float aa = a[i];
            avg(aa, pp);
            a[i] = aa;
        }
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_multi_kernel(const rfn_adam_entry* __restrict__ tab,
                                                                   const int2* __restrict__ chunks, int chunk_elems,
                                                                   double lr, double beta1d, double beta2d, float eps,
                                                                   float weight_decay, int t) {
    adam_chunk<false, false>(tab, chunks, chunk_elems, lr, beta1d, beta2d, eps, weight_decay, t, 1.f, 0, 0., nullptr);
}

// stats = (norm, scale, skip) as rfn_grad_guard_f32 left them; a skipped step writes nothing at all
__global__ __launch_bounds__(ADAM_THREADS) void adam_multi_guarded_kernel(
    const rfn_adam_entry* __restrict__ tab, const int2* __restrict__ chunks, int chunk_elems, double lr, double beta1d,
    double beta2d, float eps, float weight_decay, int t, const float* __restrict__ stats,
    const long long* __restrict__ skipped) {
    if (stats[2] != 0.f) return;
    adam_chunk<true, false>(tab, chunks, chunk_elems, lr, beta1d, beta2d, eps, weight_decay, t, stats[1], (int)*skipped,
                            0., nullptr);
}

// ema[i] is the average of table entry i: a device array of device pointers, indexed like tab[ck.x]
__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_multi_kernel(const rfn_adam_entry* __restrict__ tab,
                                                                       const int2* __restrict__ chunks, int chunk_elems,
                                                                       double lr, double beta1d, double beta2d, float eps,
                                                                       float weight_decay, int t, double ema_decay,
                                                                       float* const* __restrict__ ema) {
    adam_chunk<false, true>(tab, chunks, chunk_elems, lr, beta1d, beta2d, eps, weight_decay, t, 1.f, 0, ema_decay, ema);
}

// a skipped step leaves the average alone as well, and the count that sets its decay does not advance
__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_multi_guarded_kernel(
    const rfn_adam_entry* __restrict__ tab, const int2* __restrict__ chunks, int chunk_elems, double lr, double beta1d,
    double beta2d, float eps, float weight_decay, int t, const float* __restrict__ stats,
    const long long* __restrict__ skipped, double ema_decay, float* const* __restrict__ ema) {
    if (stats[2] != 0.f) return;
    adam_chunk<true, true>(tab, chunks, chunk_elems, lr, beta1d, beta2d, eps, weight_decay, t, stats[1], (int)*skipped,
                           ema_decay, ema);
}

// p <-> ema over the same table and chunk list: bit-exact moves, so two launches are the identity
__global__ __launch_bounds__(ADAM_THREADS) void param_swap_kernel(const rfn_adam_entry* __restrict__ tab,
                                                                   const int2* __restrict__ chunks, int chunk_elems,
                                                                   float* const* __restrict__ ema) {
    const int2 ck = chunks[blockIdx.x];
    const rfn_adam_entry e = tab[ck.x];
    const long base = (long)ck.y * chunk_elems;
    const long rem = e.n - base;
    const int n = (int)(rem < chunk_elems ? rem : chunk_elems);
    float* __restrict__ p = e.p + base;
    float* __restrict__ a = ema[ck.x] + base;
    int i0 = 0;
    if ((((uintptr_t)p | (uintptr_t)a) & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
            const float4 pp = reinterpret_cast<float4*>(p)[i];
            const float4 aa = reinterpret_cast<float4*>(a)[i];
            reinterpret_cast<float4*>(p)[i] = aa;
            reinterpret_cast<float4*>(a)[i] = pp;
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < n; i += ADAM_THREADS) {
        const float pp = p[i], aa = a[i];
        p[i] = aa;
        a[i] = pp;
    }
}

// ---- the guard: global gradient norm over the same table and chunk list -------------------------------------------
// Stage 1, one workgroup per chunk: every lane sums the squares of at most chunk/256 = 32 elements serially, the wave
// adds its 64 lanes in a shuffle tree, the four waves meet in LDS, and the chunk's partial is one plain store.  Stage 2,
// one workgroup: the partials are added in a fixed order in double, apart for tensors with flag bit 0 (rank-local
// gradients) and without.  No float atomics: equal inputs give equal bits, on every run and every rank.
__global__ __launch_bounds__(ADAM_THREADS) void grad_sumsq_chunks_kernel(const rfn_adam_entry* __restrict__ tab,
                                                                          const int2* __restrict__ chunks,
                                                                          int chunk_elems,
                                                                          float* __restrict__ partials) {
    __shared__ float sm[ADAM_THREADS / RFN_WAVE];
    const int2 ck = chunks[blockIdx.x];
    const rfn_adam_entry e = tab[ck.x];
    const long base = (long)ck.y * chunk_elems;
    const long rem = e.n - base;
    const int n = (int)(rem < chunk_elems ? rem : chunk_elems);
    const float* __restrict__ g = e.g + base;
    // the same test as the Adam kernel: both take the 16-byte path for the same chunks
    const bool v4 = ((((uintptr_t)(e.p + base) | (uintptr_t)g | (uintptr_t)(e.m + base) | (uintptr_t)(e.v + base)) & 15) == 0);
    float acc = 0.f;
    int i0 = 0;
    if (v4) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            acc = fmaf(gg.x, gg.x, acc);
            acc = fmaf(gg.y, gg.y, acc);
            acc = fmaf(gg.z, gg.z, acc);
            acc = fmaf(gg.w, gg.w, acc);
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < n; i += ADAM_THREADS) acc = fmaf(g[i], g[i], acc);
    acc = wave_sum(acc);
    if ((threadIdx.x & (RFN_WAVE - 1)) == 0) sm[threadIdx.x / RFN_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(ADAM_THREADS) void grad_sumsq_finish_kernel(const rfn_adam_entry* __restrict__ tab,
                                                                          const int2* __restrict__ chunks, int n_chunks,
                                                                          const float* __restrict__ partials,
                                                                          float* __restrict__ sumsq) {
    __shared__ double sm[2][ADAM_THREADS / RFN_WAVE];
    double a0 = 0., a1 = 0.;
    for (int c = threadIdx.x; c < n_chunks; c += ADAM_THREADS) {
        const double v = (double)partials[c];
        if (tab[chunks[c].x].flags & 1) a1 += v; else a0 += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_xor(a0, off, 64);
        a1 += __shfl_xor(a1, off, 64);
    }
    if ((threadIdx.x & (RFN_WAVE - 1)) == 0) {
        sm[0][threadIdx.x / RFN_WAVE] = a0;
        sm[1][threadIdx.x / RFN_WAVE] = a1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sumsq[0] = (float)((sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]));
        sumsq[1] = (float)((sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]));
    }
}

// One lane decides for the whole step.  NaN compares false everywhere below, so a NaN norm gives a NaN scale, as
// torch.clamp does in clip_grad_norm_.
__global__ void grad_guard_kernel(const float* __restrict__ sumsq, double max_norm, int skip_nonfinite,
                                  float* __restrict__ stats, long long* __restrict__ skipped) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double s = (double)sumsq[0] + (double)sumsq[1];
    const double norm = sqrt(s);
    double scale = 1.0;
    if (max_norm > 0.) {
        const double c = max_norm / (norm + 1e-6);
        scale = c > 1.0 ? 1.0 : c;
    }
    // the sum of squares is held to fp32's range: a sum that rounds to +inf there is non-finite, whatever its root is
    const bool skip = skip_nonfinite && !isfinite((float)s);
    stats[0] = (float)norm;
    stats[1] = (float)scale;
    stats[2] = skip ? 1.f : 0.f;
    if (skip) *skipped = *skipped + 1;
}

extern "C" int rfn_adam_chunk_elems(void) { return 8192; }

extern "C" int rfn_adam_step_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, int t, rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0, -1);
    RFN_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., -2);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), lr, beta1, beta2, (float)eps,
                       (float)weight_decay, t);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_grad_sumsq_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, float* partials,
                                  float* sumsq, rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0 && sumsq, -1);
    RFN_CHECK_ARG(partials || n_chunks == 0, -2);
    if (n_chunks > 0) {
        hipLaunchKernelGGL(grad_sumsq_chunks_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                           reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), partials);
        RFN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), n_chunks, partials, sumsq);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_grad_guard_f32(const float* sumsq, double max_norm, int skip_nonfinite, float* stats,
                                  long long* skipped, rfn_stream_t stream) {
    RFN_CHECK_ARG(sumsq && stats && skipped, -1);
    RFN_CHECK_ARG(max_norm == max_norm, -2);
    hipLaunchKernelGGL(grad_guard_kernel, dim3(1), dim3(RFN_WAVE), 0, (hipStream_t)stream, sumsq, max_norm,
                       skip_nonfinite, stats, skipped);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_adam_step_guarded_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr,
                                         double beta1, double beta2, double eps, double weight_decay, int t,
                                         const float* stats, long long* skipped, rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0 && stats && skipped, -1);
    RFN_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., -2);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_guarded_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), lr, beta1, beta2, (float)eps,
                       (float)weight_decay, t, stats, skipped);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_adam_ema_step_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, int t, double ema_decay,
                                     float* const* ema, rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0 && ema, -1);
    RFN_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., -2);
    RFN_CHECK_ARG(ema_decay >= 0. && ema_decay < 1., -3);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(adam_ema_multi_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), lr, beta1, beta2, (float)eps,
                       (float)weight_decay, t, ema_decay, ema);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_adam_ema_step_guarded_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr,
                                             double beta1, double beta2, double eps, double weight_decay, int t,
                                             const float* stats, long long* skipped, double ema_decay, float* const* ema,
                                             rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0 && stats && skipped && ema, -1);
    RFN_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., -2);
    RFN_CHECK_ARG(ema_decay >= 0. && ema_decay < 1., -3);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(adam_ema_multi_guarded_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), lr, beta1, beta2, (float)eps,
                       (float)weight_decay, t, stats, skipped, ema_decay, ema);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_param_swap_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, float* const* ema,
                                  rfn_stream_t stream) {
    RFN_CHECK_ARG(table && chunks && n_chunks >= 0 && ema, -1);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(param_swap_kernel, dim3(n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const int2*>(chunks), rfn_adam_chunk_elems(), ema);
    RFN_LAUNCH_CHECK();
    return 0;
}
