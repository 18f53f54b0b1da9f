// Kernels of the Inflated-3D Inception trunk (I3D, Kinetics-400, RGB stream) behind the Frechet Video Distance
// (the reference: evaluation_metrics/FVD.py, FVD_score.py, error_metrics.py:1006-1063; TF-hub module
// deepmind/i3d-kinetics-400/1, output RGB/inception_i3d/Mean).  The network's layer table lives in rfn_hip/i3d.py, which
// drives the four kernels of this file layer by layer; DESIGN.md section 14 is the definition.
//
// Activations are channels-last float32 [N, T, H, W, C].  Every convolution and pool pads as TF "SAME" does, per axis:
// out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before = pad_total / 2, the rest after.
//
// Convolution = implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fma chain per output value),
// the scheme of lpips.hip with the geometry in runtime arguments: rows = output positions of all videos of the call,
// columns = Cout, k = ((kt KH + ky) KW + kx) Cin + ci.  A block of 4 waves owns a 64 x 64 output tile (one 32 x 32 MFMA
// tile per wave) and walks K in chunks of 16: the gather of the chunk (64 rows x 16 k, lanes along k) and the 16 x 64
// slice of the packed [Kpad][Coutpad] weights go through registers into LDS while the previous chunk is multiplied.
// Kpad = K rounded up to 16 with zero weight rows (the gather writes zeros there too), Coutpad = Cout rounded up to 64
// with zero columns; stores are masked to Cout.  The epilogue adds the bias, applies the optional ReLU and writes at a
// channel offset into rows of a given channel pitch, so a branch of an inception block lands in the concatenated map.
// The kernel is instantiated per kernel-volume class (1, 27, 343 taps), not per layer; 1x1x1 gathers plain rows.
// Every output value is the same chain k = 0 .. Kpad-1 whatever its row in the tile, its video's index or the number of
// videos: results do not depend on batching.  The pool takes the maximum over the cells inside the map only; the head
// reduces in a fixed order; no atomics anywhere.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int I3_THREADS = 256;
constexpr int I3_BM = 64;            // output positions per block
constexpr int I3_BN = 64;            // output channels per block
constexpr int I3_KC = 16;            // k per chunk
constexpr int I3_LDA = I3_BM + 1;    // LDS row pitch of the gathered chunk (the gather writes down a column)
constexpr int I3_SIDE = 224;         // side of the resized frames
constexpr int I3_HEAD_C = 1024;      // most input channels of the head

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct I3Geom {
    int T, H, W, Cin;          // input map
    int To, Ho, Wo;            // output map
    int st, sh, sw;            // strides
    int pt, ph, pw;            // pads before
    int K, Kpad, Cout, ldw;    // ldw = Coutpad
    int out_coff, out_pitch, relu;
};

inline void i3_same(int in, int k, int s, int* out, int* pad_before) {
    *out = (in + s - 1) / s;
    int total = (*out - 1) * s + k - in;
    if (total < 0) total = 0;
    *pad_before = total / 2;
}

// out[m][out_coff + co] = act(bias[co] + sum_k A[m][k] w[k][co]), m = ((n To + ot) Ho + oy) Wo + ox.  KS = side of the
// cubic kernel (1, 3 or 7).
template <int KS>
__global__ __launch_bounds__(I3_THREADS) void i3d_conv_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              I3Geom g, int M) {
    __shared__ float As[I3_KC * I3_LDA];
    __shared__ float Bs[I3_KC * I3_BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * I3_BM, n0 = blockIdx.y * I3_BN;

    // gather role: k = tid & 15 of the chunk, rows (tid >> 4) + 16 j
    const int gk = tid & (I3_KC - 1), gr = tid >> 4;
    long gbase[4];              // KS == 1: offset of the row; otherwise offset of the video
    int git[4], giy[4], gix[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + gr + 16 * j;
        if constexpr (KS == 1) {
            gbase[j] = m < M ? (long)m * g.Cin : -1;   // stride 1, no padding: the output position is the input position
            git[j] = giy[j] = gix[j] = 0;
        } else if (m < M) {
            int t = m;
            const int ox = t % g.Wo;
            t /= g.Wo;
            const int oy = t % g.Ho;
            t /= g.Ho;
            const int ot = t % g.To;
            const int n = t / g.To;
            gbase[j] = (long)n * g.T * g.H * g.W * g.Cin;
            git[j] = ot * g.st - g.pt;
            giy[j] = oy * g.sh - g.ph;
            gix[j] = ox * g.sw - g.pw;
        } else {  // rows past the end gather zeros
            gbase[j] = 0;
            git[j] = giy[j] = gix[j] = -(1 << 30);
        }
    }
    // weight role: k = (tid >> 6) + 4 j of the chunk, column tid & 63
    const float* wp = w + (long)(tid >> 6) * g.ldw + n0 + (tid & 63);

    float ra[4], rb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + gk;
        if constexpr (KS == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ra[j] = (k < g.K && gbase[j] >= 0) ? in[gbase[j] + k] : 0.f;
        } else {
            const int tap = k / g.Cin, ci = k - tap * g.Cin;
            const int kt = tap / (KS * KS), r = tap - kt * (KS * KS);
            const int ky = r / KS, kx = r - ky * KS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int it = git[j] + kt, iy = giy[j] + ky, ix = gix[j] + kx;
                float v = 0.f;
                if (k < g.K && it >= 0 && it < g.T && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                    v = in[gbase[j] + (((long)it * g.H + iy) * g.W + ix) * g.Cin + ci];
                ra[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = wp[(long)(k0 + 4 * j) * g.ldw];
    };

    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, kk = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    fetch(0);
    for (int k0 = 0; k0 < g.Kpad; k0 += I3_KC) {
        __syncthreads();  // the previous chunk's readers are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[gk * I3_LDA + gr + 16 * j] = ra[j];
            Bs[((tid >> 6) + 4 * j) * I3_BN + (tid & 63)] = rb[j];
        }
        __syncthreads();
        if (k0 + I3_KC < g.Kpad) fetch(k0 + I3_KC);
#pragma unroll
        for (int s = 0; s < I3_KC / 2; ++s) {
            const float a = As[(2 * s + kk) * I3_LDA + wm * 32 + l31];
            const float b = Bs[(2 * s + kk) * I3_BN + wn * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }

    // D[i = position][j = co]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int co = n0 + wn * 32 + l31;
    if (co < g.Cout) {
        const float bv = bias[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
            if (m < M) {
                const float v = acc[r] + bv;
                out[(long)m * g.out_pitch + g.out_coff + co] = g.relu ? fmaxf(v, 0.f) : v;
            }
        }
    }
}

struct I3Pool {
    int T, H, W, C, To, Ho, Wo;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
};

// SAME max pool of a dense [n][T][H][W][C] map into a dense [n][To][Ho][Wo][C] one: the maximum over the window's cells
// that lie inside the map (a SAME window always holds at least one).
__global__ __launch_bounds__(I3_THREADS) void i3d_pool_kernel(const float* __restrict__ in, float* __restrict__ out, I3Pool p,
                                                              long total) {
    for (long i = (long)blockIdx.x * I3_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * I3_THREADS) {
        const int c = (int)(i % p.C);
        long t = i / p.C;
        const int ox = (int)(t % p.Wo);
        t /= p.Wo;
        const int oy = (int)(t % p.Ho);
        t /= p.Ho;
        const int ot = (int)(t % p.To);
        const long n = t / p.To;
        const int t0 = ot * p.st - p.pt, y0 = oy * p.sh - p.ph, x0 = ox * p.sw - p.pw;
        const float* src = in + n * p.T * p.H * p.W * p.C + c;
        float v = -INFINITY;
        for (int dt = 0; dt < p.kt; ++dt) {
            const int it = t0 + dt;
            if (it < 0 || it >= p.T) continue;
            for (int dy = 0; dy < p.kh; ++dy) {
                const int iy = y0 + dy;
                if (iy < 0 || iy >= p.H) continue;
                for (int dx = 0; dx < p.kw; ++dx) {
                    const int ix = x0 + dx;
                    if (ix < 0 || ix >= p.W) continue;
                    v = fmaxf(v, src[(((long)it * p.H + iy) * p.W + ix) * p.C]);
                }
            }
        }
        out[i] = v;
    }
}

// uint8 frames [f][C][H][W] -> float [f][224][224][3], TF1 resize_bilinear (align_corners=False, no half-pixel centres):
// src = dst * (in / 224) in float32, i0 = floor(src), i1 = min(i0 + 1, in - 1), weight src - i0; the two rows are
// interpolated along x, then the two results along y; then x = 2 v / 255 - 1.  C == 1: the stored channel thrice.
__global__ __launch_bounds__(I3_THREADS) void i3d_resize_kernel(const uint8_t* __restrict__ in, long frame_stride, int C,
                                                                int H, int W, float sy, float sx,
                                                                float* __restrict__ out, long total) {
#pragma clang fp contract(off)  // the lerps are a + (b - a) w with every operation rounded
    for (long i = (long)blockIdx.x * I3_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * I3_THREADS) {
        const int c = (int)(i % 3);
        long t = i / 3;
        const int ox = (int)(t % I3_SIDE);
        t /= I3_SIDE;
        const int oy = (int)(t % I3_SIDE);
        const long f = t / I3_SIDE;
        const float fy = (float)oy * sy, fx = (float)ox * sx;
        const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
        const float wy = fy - (float)y0, wx = fx - (float)x0;
        const uint8_t* src = in + f * frame_stride + (long)(C == 1 ? 0 : c) * H * W;
        const float tl = (float)src[(long)y0 * W + x0], tr = (float)src[(long)y0 * W + x1];
        const float bl = (float)src[(long)y1 * W + x0], br = (float)src[(long)y1 * W + x1];
        const float top = tl + (tr - tl) * wx;
        const float bot = bl + (br - bl) * wx;
        const float v = top + (bot - top) * wy;
        out[i] = 2.f * v / 255.f - 1.f;
    }
}

// Head: one block per video.  in [n][Tp][P][C] (P = 49 cells of the 7 x 7 map); per time window t = 0 .. Tp-2 the
// average over 2 x P cells (time-major, cells in order), the Cout logits bias + sum_c avg[c] w[c][o] (c in order), then
// the mean over the windows in order.
__global__ __launch_bounds__(I3_THREADS) void i3d_head_kernel(const float* __restrict__ in, int Tp, int P, int C,
                                                              const float* __restrict__ w, int ldw,
                                                              const float* __restrict__ bias, int Cout,
                                                              float* __restrict__ out) {
    __shared__ float avg[I3_HEAD_C];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* src = in + (long)n * Tp * P * C;
    float acc[2] = {0.f, 0.f};     // logits tid and tid + 256 (Cout <= 512)
    for (int t = 0; t + 1 < Tp; ++t) {
        __syncthreads();
        for (int c = tid; c < C; c += I3_THREADS) {
            float s = 0.f;
            for (int q = 0; q < 2 * P; ++q) s += src[((long)t * P + q) * C + c];
            avg[c] = s / (float)(2 * P);
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = tid + h * I3_THREADS;
            if (o < Cout) {
                float a = bias[o];
                for (int c = 0; c < C; ++c) a = fmaf(avg[c], w[(long)c * ldw + o], a);
                acc[h] += a;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int o = tid + h * I3_THREADS;
        if (o < Cout) out[(long)n * Cout + o] = acc[h] / (float)(Tp - 1);
    }
}

inline unsigned i3_blocks(long total) {
    long b = (total + I3_THREADS - 1) / I3_THREADS;
    return (unsigned)(b > 65536 ? 65536 : b);
}

}  // namespace

extern "C" int rfn_i3d_same(int in, int k, int s, long long* out) {
    RFN_CHECK_ARG(out != nullptr, -1);
    RFN_CHECK_ARG(in >= 1 && k >= 1 && s >= 1, -2);
    int o, p;
    i3_same(in, k, s, &o, &p);
    out[0] = o, out[1] = p;
    return 0;
}

extern "C" int rfn_i3d_conv_pack_dims(int Cin, int Cout, int k, long long* out) {
    RFN_CHECK_ARG(out != nullptr, -1);
    RFN_CHECK_ARG(Cin >= 1 && Cout >= 1 && (k == 1 || k == 3 || k == 7), -2);
    const long K = (long)Cin * k * k * k;
    out[0] = (K + I3_KC - 1) / I3_KC * I3_KC;
    out[1] = (Cout + I3_BN - 1) / I3_BN * I3_BN;
    return 0;
}

extern "C" int rfn_i3d_conv3d_f32(const float* in, long in_floats, int N, int T, int H, int W, int Cin, const float* wpack,
                                  long wpack_floats, const float* bias, int Cout, int k, int stride, int relu, float* out,
                                  long out_floats, int out_coff, int out_pitch, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0 && T >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, -1);
    RFN_CHECK_ARG(k == 1 || k == 3 || k == 7, -2);
    RFN_CHECK_ARG(stride == 1 || (stride == 2 && k > 1), -3);
    RFN_CHECK_ARG(out_coff >= 0 && out_coff + Cout <= out_pitch, -4);
    if (N == 0) return 0;
    I3Geom g;
    g.T = T, g.H = H, g.W = W, g.Cin = Cin;
    g.st = g.sh = g.sw = stride;
    i3_same(T, k, stride, &g.To, &g.pt);
    i3_same(H, k, stride, &g.Ho, &g.ph);
    i3_same(W, k, stride, &g.Wo, &g.pw);
    const long K = (long)Cin * k * k * k;
    RFN_CHECK_ARG(K <= (1L << 24), -5);
    g.K = (int)K;
    g.Kpad = (g.K + I3_KC - 1) / I3_KC * I3_KC;
    g.Cout = Cout;
    g.ldw = (Cout + I3_BN - 1) / I3_BN * I3_BN;
    g.out_coff = out_coff, g.out_pitch = out_pitch, g.relu = relu ? 1 : 0;
    const long M = (long)N * g.To * g.Ho * g.Wo;
    // GEMM rows are counted in int
    RFN_CHECK_ARG(M <= (1L << 30), -6);
    RFN_CHECK_ARG(in && wpack && bias && out, -7);
    RFN_CHECK_ARG(in_floats >= (long)N * T * H * W * Cin, -8);
    RFN_CHECK_ARG(wpack_floats >= (long)g.Kpad * g.ldw, -9);
    RFN_CHECK_ARG(out_floats >= M * out_pitch, -10);
    const dim3 grid((unsigned)ceil_div(M, I3_BM), (unsigned)(g.ldw / I3_BN));
    hipStream_t s = (hipStream_t)stream;
    if (k == 1)
        hipLaunchKernelGGL(i3d_conv_kernel<1>, grid, dim3(I3_THREADS), 0, s, in, wpack, bias, out, g, (int)M);
    else if (k == 3)
        hipLaunchKernelGGL(i3d_conv_kernel<3>, grid, dim3(I3_THREADS), 0, s, in, wpack, bias, out, g, (int)M);
    else
        hipLaunchKernelGGL(i3d_conv_kernel<7>, grid, dim3(I3_THREADS), 0, s, in, wpack, bias, out, g, (int)M);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_i3d_maxpool3d_f32(const float* in, long in_floats, int N, int T, int H, int W, int C, int kt, int khw,
                                     int st, int shw, float* out, long out_floats, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0 && T >= 1 && H >= 1 && W >= 1 && C >= 1, -1);
    RFN_CHECK_ARG(kt >= 1 && kt <= 3 && khw >= 1 && khw <= 3 && st >= 1 && st <= kt && shw >= 1 && shw <= khw, -2);
    if (N == 0) return 0;
    I3Pool p;
    p.T = T, p.H = H, p.W = W, p.C = C;
    p.kt = kt, p.kh = p.kw = khw, p.st = st, p.sh = p.sw = shw;
    i3_same(T, kt, st, &p.To, &p.pt);
    i3_same(H, khw, shw, &p.Ho, &p.ph);
    i3_same(W, khw, shw, &p.Wo, &p.pw);
    const long total = (long)N * p.To * p.Ho * p.Wo * C;
    RFN_CHECK_ARG(in && out, -3);
    RFN_CHECK_ARG(in_floats >= (long)N * T * H * W * C, -4);
    RFN_CHECK_ARG(out_floats >= total, -5);
    hipLaunchKernelGGL(i3d_pool_kernel, dim3(i3_blocks(total)), dim3(I3_THREADS), 0, (hipStream_t)stream, in, out, p, total);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_i3d_resize_u8(const void* frames, long frame_stride, int NF, int C, int H, int W, float* out,
                                 long out_floats, rfn_stream_t stream) {
    RFN_CHECK_ARG(NF >= 0 && H >= 1 && W >= 1, -1);
    RFN_CHECK_ARG(C == 1 || C == 3, -2);
    if (NF == 0) return 0;
    RFN_CHECK_ARG(frames && out, -3);
    RFN_CHECK_ARG(frame_stride >= (long)C * H * W, -4);
    const long total = (long)NF * I3_SIDE * I3_SIDE * 3;
    RFN_CHECK_ARG(out_floats >= total, -5);
    // the scales in / out are float32 quotients, as TF computes them
    const float sy = (float)H / (float)I3_SIDE, sx = (float)W / (float)I3_SIDE;
    hipLaunchKernelGGL(i3d_resize_kernel, dim3(i3_blocks(total)), dim3(I3_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)frames, frame_stride, C, H, W, sy, sx, out, total);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_i3d_head_f32(const float* in, long in_floats, int N, int Tp, int P, int C, const float* wpack,
                                long wpack_floats, const float* bias, int Cout, float* out, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0 && P >= 1, -1);
    // two time steps for the average pool
    RFN_CHECK_ARG(Tp >= 2, -2);
    RFN_CHECK_ARG(C >= 1 && C <= I3_HEAD_C && Cout >= 1 && Cout <= 2 * I3_THREADS, -3);
    if (N == 0) return 0;
    const int ldw = (Cout + I3_BN - 1) / I3_BN * I3_BN;
    RFN_CHECK_ARG(in && wpack && bias && out, -4);
    RFN_CHECK_ARG(in_floats >= (long)N * Tp * P * C, -5);
    RFN_CHECK_ARG(wpack_floats >= (long)C * ldw, -6);
    hipLaunchKernelGGL(i3d_head_kernel, dim3((unsigned)N), dim3(I3_THREADS), 0, (hipStream_t)stream, in, Tp, P, C, wpack,
                       ldw, bias, Cout, out);
    RFN_LAUNCH_CHECK();
    return 0;
}
