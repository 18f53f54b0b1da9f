// The linear-extrapolation baseline (averagemodel/averagemodel.py of the reference, its "simple linear model"): a
// per-pixel linear map of the last n frames and of all their lagged differences, and the Gaussian-window SSIM its
// evaluation reports.  DESIGN.md section 26 is the contract; include/rfn_hip.h states the entry points.
//
// Features of a window x_0 .. x_{n-1} (one pixel), in the order of SimpleLinearModel.get_prediction (:65-81):
//   f = 0 .. n-1:                                   x_f
//   then k = 0 .. n-2, inside that j = 0 .. n-k-2:  x_j - x_{j+k+1}
// F = n (n + 1) / 2;  pred = bias + sum_f W[f] feat_f, one fma chain in feature order.
//
// All three kernels stream from HBM: the train and rollout kernels read every conditioning frame once (16-byte loads
// when the pixel count and the strides allow, single floats otherwise) and keep the window in registers; the quality
// kernel reads X and Y once and forms the five window sums in LDS.  No atomics anywhere: reductions run in a fixed
// order, so results are bit-identical run to run on one device.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int LX_THREADS = 256;
constexpr int LX_MAX_BLOCKS = 4096;   // rows of the partials buffer the train kernel may use, at the most

// ---- the per-pixel prediction: features formed in registers, never collapsed into per-frame weights (the gradient
// needs each feature, and differences of large sums would cancel)
template <int N>
__device__ __forceinline__ float linext_predict(const float (&win)[N], const float* __restrict__ w, float bias,
                                                float (&feat)[N * (N + 1) / 2]) {
    float acc = bias;
#pragma unroll
    for (int f = 0; f < N; ++f) {
        feat[f] = win[f];
        acc = fmaf(w[f], feat[f], acc);
    }
    int idx = N;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
#pragma unroll
        for (int j = 0; j < N - k - 1; ++j) {
            feat[idx] = win[j] - win[j + k + 1];
            acc = fmaf(w[idx], feat[idx], acc);
            ++idx;
        }
    }
    return acc;
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
    __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// frames s .. s+N-1 of sequence b at pixel q (V consecutive pixels) into win[v][f]
template <int N, int V>
__device__ __forceinline__ void load_window(const float* __restrict__ base, long xf, float (&win)[V][N]) {
#pragma unroll
    for (int f = 0; f < N; ++f) {
        Vec<V> t;
        t.load(base + (long)f * xf);
#pragma unroll
        for (int v = 0; v < V; ++v) win[v][f] = t.v[v];
    }
}

// ---- loss and gradients, stage 1: grid (gx, gy); block (bx, by) walks the pixels bx*256+tid, += gx*256 of the sequences
// by, by+gy, ...; its row of `partials` holds [sum r^2, sum r feat_0 .. sum r feat_{F-1}, sum r]
template <int N, int V>
__global__ __launch_bounds__(LX_THREADS) void linext_train_kernel(const float* __restrict__ x, long xs, long xf, int s,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias,
                                                                  float* __restrict__ partials, int B, long items) {
    constexpr int F = N * (N + 1) / 2;
    __shared__ float sm[LX_THREADS / 64][F + 2];
    float acc[F + 2];
#pragma unroll
    for (int o = 0; o < F + 2; ++o) acc[o] = 0.f;
    const float b0 = bias[0];
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ seq = x + (long)b * xs + (long)s * xf;
        for (long i = (long)blockIdx.x * LX_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * LX_THREADS) {
            float win[V][N];
            load_window<N, V>(seq + i * V, xf, win);
            Vec<V> tgt;
            tgt.load(seq + (long)N * xf + i * V);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float feat[F];
                const float r = linext_predict<N>(win[v], w, b0, feat) - tgt.v[v];
                acc[0] = fmaf(r, r, acc[0]);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[1 + f] = fmaf(r, feat[f], acc[1 + f]);
                acc[F + 1] += r;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 0; o < F + 2; ++o) {
        const float t = wave_sum(acc[o]);
        if (lane == 0) sm[wave][o] = t;
    }
    __syncthreads();
    float* __restrict__ row = partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (F + 2);
    for (int o = threadIdx.x; o < F + 2; o += LX_THREADS) row[o] = ((sm[0][o] + sm[1][o]) + sm[2][o]) + sm[3][o];
}

// stage 2: one workgroup; wave w owns outputs w, w+4, ...; lane l adds rows l, l+64, ... in row order in double, then
// the xor butterfly.  out[0] = loss, out[1 .. F] = dL/dW, out[F+1] = dL/dbias of the MEAN squared error over `count`.
__global__ __launch_bounds__(LX_THREADS) void linext_finish_kernel(const float* __restrict__ partials, int rows, int F,
                                                                   double count, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = wave; o < F + 2; o += LX_THREADS / 64) {
        double t = 0.0;
        for (int r = lane; r < rows; r += 64) t += (double)partials[(long)r * (F + 2) + o];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) out[o] = (float)((o == 0 ? t : 2.0 * t) / count);
    }
}

// ---- the autoregressive rollout: a thread owns V pixels of one sequence, keeps their window in registers and writes
// all P frames
template <int N, int V>
__global__ __launch_bounds__(LX_THREADS) void linext_rollout_kernel(const float* __restrict__ x, long xs, long xf, int s,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ out, int B, int P, long CHW,
                                                                    long items) {
    constexpr int F = N * (N + 1) / 2;
    const float b0 = bias[0];
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ seq = x + (long)b * xs + (long)s * xf;
        float* __restrict__ dst = out + (long)b * P * CHW;
        for (long i = (long)blockIdx.x * LX_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * LX_THREADS) {
            float win[V][N];
            load_window<N, V>(seq + i * V, xf, win);
            for (int t = 0; t < P; ++t) {
                Vec<V> pred;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float feat[F];
                    pred.v[v] = linext_predict<N>(win[v], w, b0, feat);
#pragma unroll
                    for (int f = 0; f + 1 < N; ++f) win[v][f] = win[v][f + 1];
                    win[v][N - 1] = pred.v[v];
                }
                pred.store(dst + (long)t * CHW + i * V);
            }
        }
    }
}

// compute units of the current device (cached; a query, nothing is enqueued)
int device_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// grid (gx, gy) of at most `limit` blocks over B sequences of `items` work items each
dim3 linext_grid(int B, long items, long limit) {
    if (limit < 1) limit = 1;
    long gx = (items + LX_THREADS - 1) / LX_THREADS;
    const long per_seq = limit / B > 1 ? limit / B : 1;
    if (gx > per_seq) gx = per_seq;
    long gy = limit / gx;
    if (gy > B) gy = B;
    if (gy > 65535) gy = 65535;
    if (gy < 1) gy = 1;
    return dim3((unsigned)gx, (unsigned)gy);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int V, typename... Args>
int linext_launch_train(int n, dim3 grid, hipStream_t st, Args... a) {
    switch (n) {
#define LX_CASE(NN) case NN: hipLaunchKernelGGL((linext_train_kernel<NN, V>), grid, dim3(LX_THREADS), 0, st, a...); return 0;
        LX_CASE(1) LX_CASE(2) LX_CASE(3) LX_CASE(4) LX_CASE(5) LX_CASE(6) LX_CASE(7) LX_CASE(8) LX_CASE(9) LX_CASE(10)
#undef LX_CASE
    }
    return -1;
}

template <int V, typename... Args>
int linext_launch_rollout(int n, dim3 grid, hipStream_t st, Args... a) {
    switch (n) {
#define LX_CASE(NN) case NN: hipLaunchKernelGGL((linext_rollout_kernel<NN, V>), grid, dim3(LX_THREADS), 0, st, a...); return 0;
        LX_CASE(1) LX_CASE(2) LX_CASE(3) LX_CASE(4) LX_CASE(5) LX_CASE(6) LX_CASE(7) LX_CASE(8) LX_CASE(9) LX_CASE(10)
#undef LX_CASE
    }
    return -1;
}

// ---- Gaussian-window SSIM and MSE of scaled, clamped float frames
constexpr int GQ_WIN = RFN_GAUSS_QUALITY_MIN_SIDE;   // the window's length
constexpr int GQ_MAX = RFN_GAUSS_QUALITY_MAX_SIDE;   // largest H and W
constexpr int GQ_TR = 6;                    // input rows per chunk
constexpr int GQ_RB = 16;                   // ring of row sums: >= GQ_TR + GQ_WIN - 1, a power of two
constexpr int GQ_WO = GQ_MAX - GQ_WIN + 1;  // most output columns

struct GaussWindow {
    float g[GQ_WIN];
    double gd[GQ_WIN];
};

__device__ __forceinline__ double block_sum_d(double v, double* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// One workgroup per image.  A channel is walked in chunks of GQ_TR input rows: the chunk of X and Y is loaded once
// (scaled and clamped) into LDS, its five row sums g*x, g*y, g*xx, g*yy, g*xy go into a ring of GQ_RB rows, and the
// output rows whose eleven row sums are now complete are finished from the ring.  Row sums are fp32 fma chains in tap
// order; the column pass and the SSIM formula run in fp64 on them (sigma^2 = g*(xx) - mu^2 cancels).
__global__ __launch_bounds__(LX_THREADS) void gauss_quality_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                   float* __restrict__ ssim, float* __restrict__ mse,
                                                                   int C, int H, int W, float scale, float lo, float hi,
                                                                   GaussWindow win) {
    __shared__ float sx[GQ_TR][GQ_MAX], sy[GQ_TR][GQ_MAX];
    __shared__ float hs[5][GQ_RB][GQ_WO];
    __shared__ double sm_d[LX_THREADS / 64];
    const int n = blockIdx.x;
    const int Ho = H - (GQ_WIN - 1), Wo = W - (GQ_WIN - 1);
    const long HW = (long)H * W;
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double sse = 0.0, ssim_sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ x = X + ((long)n * C + c) * HW;
        const float* __restrict__ y = Y + ((long)n * C + c) * HW;
        double s_acc = 0.0;
        for (int a = 0; a < H; a += GQ_TR) {
            const int rows = min(GQ_TR, H - a);
            __syncthreads();  // the previous chunk's readers are done with sx, sy and the ring rows about to be replaced
            for (int k = threadIdx.x; k < rows * W; k += LX_THREADS) {
                const int i = k / W, j = k - i * W;
                const float u = fminf(fmaxf(x[(long)(a + i) * W + j] * scale, lo), hi);
                const float v = fminf(fmaxf(y[(long)(a + i) * W + j] * scale, lo), hi);
                sx[i][j] = u;
                sy[i][j] = v;
                const double d = (double)u - (double)v;
                sse += d * d;
            }
            __syncthreads();
            for (int k = threadIdx.x; k < rows * Wo; k += LX_THREADS) {
                const int i = k / Wo, j = k - i * Wo;
                float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
                for (int t = 0; t < GQ_WIN; ++t) {
                    const float u = sx[i][j + t], v = sy[i][j + t], g = win.g[t];
                    mx = fmaf(g, u, mx);
                    my = fmaf(g, v, my);
                    mxx = fmaf(g, u * u, mxx);
                    myy = fmaf(g, v * v, myy);
                    mxy = fmaf(g, u * v, mxy);
                }
                const int r = (a + i) & (GQ_RB - 1);
                hs[0][r][j] = mx;
                hs[1][r][j] = my;
                hs[2][r][j] = mxx;
                hs[3][r][j] = myy;
                hs[4][r][j] = mxy;
            }
            __syncthreads();
            // output rows o with o + 10 inside this chunk
            const int o0 = max(a - (GQ_WIN - 1), 0), o1 = a + rows - (GQ_WIN - 1);  // [o0, o1)
            for (int k = threadIdx.x; k < (o1 - o0) * Wo; k += LX_THREADS) {
                const int i = k / Wo, j = k - i * Wo;
                const int o = o0 + i;
                double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
                for (int t = 0; t < GQ_WIN; ++t) {
                    const int r = (o + t) & (GQ_RB - 1);
                    const double g = win.gd[t];
                    mx += g * (double)hs[0][r][j];
                    my += g * (double)hs[1][r][j];
                    mxx += g * (double)hs[2][r][j];
                    myy += g * (double)hs[3][r][j];
                    mxy += g * (double)hs[4][r][j];
                }
                const double vx = mxx - mx * mx, vy = myy - my * my, cxy = mxy - mx * my;
                s_acc += ((2.0 * mx * my + C1) / (mx * mx + my * my + C1)) * ((2.0 * cxy + C2) / (vx + vy + C2));
            }
        }
        s_acc = block_sum_d(s_acc, sm_d);
        ssim_sum += s_acc / ((double)Ho * (double)Wo);
    }
    sse = block_sum_d(sse, sm_d);
    if (threadIdx.x == 0) {
        ssim[n] = (float)(ssim_sum / C);
        mse[n] = (float)(sse / ((double)C * (double)HW));
    }
}

}  // namespace

extern "C" int rfn_linext_max_blocks(void) { return LX_MAX_BLOCKS; }
extern "C" int rfn_linext_max_frames(void) { return RFN_LINEXT_MAX_FRAMES; }
extern "C" int rfn_gauss_quality_min_side(void) { return RFN_GAUSS_QUALITY_MIN_SIDE; }
extern "C" int rfn_gauss_quality_max_side(void) { return RFN_GAUSS_QUALITY_MAX_SIDE; }

extern "C" int rfn_linext_train_f32(const float* x, long seq_stride, long frame_stride, int start, const float* w,
                                    const float* bias, float* partials, long partial_floats, float* out, int B, int T,
                                    int n, long CHW, rfn_stream_t stream) {
    RFN_CHECK_ARG(n >= 1 && n <= RFN_LINEXT_MAX_FRAMES, -1);
    RFN_CHECK_ARG(B >= 1 && CHW >= 1 && start >= 0 && T >= 1 && (long)start + n + 1 <= T, -1);
    RFN_CHECK_ARG(frame_stride >= CHW && seq_stride >= (long)(T - 1) * frame_stride + CHW, -1);
    const int F = n * (n + 1) / 2;
    RFN_CHECK_ARG(partial_floats >= F + 2, -1);
    RFN_CHECK_ARG(x && w && bias && partials && out, -2);
    const bool vec = CHW % 4 == 0 && seq_stride % 4 == 0 && frame_stride % 4 == 0 && aligned16(x);
    const long items = vec ? CHW / 4 : CHW;
    long limit = (long)device_cus() * 8;
    if (limit > LX_MAX_BLOCKS) limit = LX_MAX_BLOCKS;
    if (limit > partial_floats / (F + 2)) limit = partial_floats / (F + 2);
    const dim3 grid = linext_grid(B, items, limit);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        linext_launch_train<4>(n, grid, st, x, seq_stride, frame_stride, start, w, bias, partials, B, items);
    else
        linext_launch_train<1>(n, grid, st, x, seq_stride, frame_stride, start, w, bias, partials, B, items);
    RFN_LAUNCH_CHECK();
    hipLaunchKernelGGL(linext_finish_kernel, dim3(1), dim3(LX_THREADS), 0, st, (const float*)partials,
                       (int)(grid.x * grid.y), F, (double)B * (double)CHW, out);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_linext_rollout_f32(const float* x, long seq_stride, long frame_stride, int start, const float* w,
                                      const float* bias, float* out, int B, int T, int n, int P, long CHW,
                                      rfn_stream_t stream) {
    RFN_CHECK_ARG(n >= 1 && n <= RFN_LINEXT_MAX_FRAMES && P >= 1, -1);
    RFN_CHECK_ARG(B >= 1 && CHW >= 1 && start >= 0 && T >= 1 && (long)start + n <= T, -1);
    RFN_CHECK_ARG(frame_stride >= CHW && seq_stride >= (long)(T - 1) * frame_stride + CHW, -1);
    RFN_CHECK_ARG(x && w && bias && out, -2);
    const bool vec = CHW % 4 == 0 && seq_stride % 4 == 0 && frame_stride % 4 == 0 && aligned16(x) && aligned16(out);
    const long items = vec ? CHW / 4 : CHW;
    const dim3 grid = linext_grid(B, items, (long)device_cus() * 8);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        linext_launch_rollout<4>(n, grid, st, x, seq_stride, frame_stride, start, w, bias, out, B, P, CHW, items);
    else
        linext_launch_rollout<1>(n, grid, st, x, seq_stride, frame_stride, start, w, bias, out, B, P, CHW, items);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_gauss_quality_f32(const float* pred, const float* truth, float* ssim, float* mse, int N, int C, int H,
                                     int W, float scale, float lo, float hi, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 1 && C >= 1, -1);
    RFN_CHECK_ARG(H >= GQ_WIN && H <= GQ_MAX && W >= GQ_WIN && W <= GQ_MAX, -1);
    RFN_CHECK_ARG(lo <= hi, -1);
    RFN_CHECK_ARG(pred && truth && ssim && mse, -2);
    GaussWindow win;
    double sum = 0.0;
    for (int i = 0; i < GQ_WIN; ++i) {
        win.gd[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.gd[i];
    }
    for (int i = 0; i < GQ_WIN; ++i) {
        win.gd[i] /= sum;
        win.g[i] = (float)win.gd[i];
    }
    hipLaunchKernelGGL(gauss_quality_kernel, dim3((unsigned)N), dim3(LX_THREADS), 0, (hipStream_t)stream, pred, truth,
                       ssim, mse, C, H, W, scale, lo, hi, win);
    RFN_LAUNCH_CHECK();
    return 0;
}
