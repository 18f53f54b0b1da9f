// LPIPS with the AlexNet trunk (the reference scores every predicted frame with lpips.LPIPS(net='alex'),
// evaluation_metrics/error_metrics.py:72, :173-187; definition: `lpips` 0.1.3, net='alex', version 0.1, lpips=True,
// spatial=False, eval mode) over a whole batch of uint8 frames.
//
// Input frames [C, H, W] uint8, C in {1, 3} (one channel stands for all three).  Pixel p -> x = p/255*2 - 1 ->
// (x - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  Trunk, five taps, each after a
// ReLU, every convolution with bias and zero padding in the scaled domain:
//   1  conv 3->64 11x11 stride 4 pad 2                                 Ho = (H + 4 - 11) / 4 + 1
//   2  maxpool 3x3 stride 2 (floor, no pad), conv 64->192 5x5 pad 2
//   3  maxpool 3x3 stride 2, conv 192->384 3x3 pad 1
//   4  conv 384->256 3x3 pad 1
//   5  conv 256->256 3x3 pad 1
// Head: per tap l and pixel n(f) = f / (sqrt(sum_c f_c^2) + 1e-10); d_l = mean over pixels of
// sum_c w_l[c] (n(f0)_c - n(f1)_c)^2; d = sum_l d_l.  The second pool needs a 3x3 map: H, W >= 31.
//
// Feature pack of a frame: the five taps one after the other, each [Ho*Wo][Cout] (channels contiguous per pixel: what the
// GEMM epilogue writes and what the head reads).
//
// Convolution = implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fma chain per output value):
// rows = output pixels of all frames of the call, columns = Cout, k = (ky*KS + kx)*Cin + ci.  A block of 4 waves owns a
// 64 x 64 output tile (one 32 x 32 MFMA tile per wave) and walks K in chunks of 16: the im2col gather of the chunk
// (64 rows x 16 k) and the 16 x 64 slice of the packed [Kpad][Cout] weights go through registers into LDS while the
// previous chunk is multiplied.  K = 363 of the first convolution is padded to 368 with zero weights, and the gather
// writes zeros there.  Every output value is the same chain k = 0 .. Kpad-1 whatever its row in the tile, its frame's
// index or the number of frames: results do not depend on batching, and a one-channel frame gives the bits of three
// identical channels.  The head reduces in a fixed order (lanes over channels, xor butterfly, waves over pixels, taps in
// order), with contraction off so that (a, b) and (b, a) give the same bits; no atomics anywhere.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_BM = 64;            // output pixels per block
constexpr int LP_BN = 64;            // output channels per block
constexpr int LP_KC = 16;            // k per chunk
constexpr int LP_LDA = LP_BM + 1;    // LDS row pitch of the gathered chunk (the gather writes down a column)
constexpr int LP_TAPS = 5;
constexpr int LP_CIN[LP_TAPS] = {3, 64, 192, 384, 256};
constexpr int LP_COUT[LP_TAPS] = {64, 192, 384, 256, 256};
constexpr int LP_KS[LP_TAPS] = {11, 5, 3, 3, 3};
constexpr int LP_MIN_SIDE = 31;

constexpr int lp_kpad(int l) { return (LP_CIN[l] * LP_KS[l] * LP_KS[l] + LP_KC - 1) / LP_KC * LP_KC; }

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LpSizes {
    int h[LP_TAPS], w[LP_TAPS];  // map sizes of the taps
    int ph[2], pw[2];            // pooled maps in front of convolutions 2 and 3
    long feat;                   // floats per frame of the feature pack
    long work;                   // workspace floats per frame (the two pooled maps)
};

int lp_sizes(int H, int W, LpSizes* s) {
    if (H < LP_MIN_SIDE || W < LP_MIN_SIDE) return -1;
    s->h[0] = (H + 4 - 11) / 4 + 1;
    s->w[0] = (W + 4 - 11) / 4 + 1;
    s->ph[0] = (s->h[0] - 3) / 2 + 1;
    s->pw[0] = (s->w[0] - 3) / 2 + 1;
    s->h[1] = s->ph[0];
    s->w[1] = s->pw[0];
    s->ph[1] = (s->h[1] - 3) / 2 + 1;
    s->pw[1] = (s->w[1] - 3) / 2 + 1;
    for (int l = 2; l < LP_TAPS; ++l) {
        s->h[l] = s->ph[1];
        s->w[l] = s->pw[1];
    }
    s->feat = 0;
    for (int l = 0; l < LP_TAPS; ++l) s->feat += (long)s->h[l] * s->w[l] * LP_COUT[l];
    s->work = (long)s->ph[0] * s->pw[0] * LP_COUT[0] + (long)s->ph[1] * s->pw[1] * LP_COUT[1];
    return 0;
}

struct LpHeadSizes {
    int pix[LP_TAPS];
    long feat;
};

// out[f][pix][co] = relu(bias[co] + sum_k A[f, pix][k] * w[k][co]);  U8: the input is the uint8 NCHW frame batch, scaled in
// the gather; otherwise a float map [f][iy*Wi + ix][CIN] with frame pitch in_fs.
template <int CIN, int KS, int STRIDE, int PAD, int COUT, bool U8>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(const void* __restrict__ in_, long in_fs, int Cimg, int Hi,
                                                                int Wi, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ out,
                                                                long out_fs, int Ho, int Wo, int M) {
    constexpr int K = CIN * KS * KS;
    constexpr int KPAD = (K + LP_KC - 1) / LP_KC * LP_KC;
    static_assert(COUT % LP_BN == 0, "whole column tiles");
    __shared__ float As[LP_KC * LP_LDA];
    __shared__ float Bs[LP_KC * LP_BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;
    const int HoWo = Ho * Wo;

    // gather role: k = tid & 15 of the chunk, rows (tid >> 4) + 16 j
    const int gk = tid & (LP_KC - 1), gr = tid >> 4;
    long gbase[4];
    int giy[4], gix[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + gr + 16 * j;
        if (m < M) {
            const int f = m / HoWo, pix = m - f * HoWo;
            const int oy = pix / Wo, ox = pix - oy * Wo;
            gbase[j] = (long)f * in_fs;
            giy[j] = oy * STRIDE - PAD;
            gix[j] = ox * STRIDE - PAD;
        } else {  // rows past the end gather zeros
            gbase[j] = 0;
            giy[j] = -(1 << 30);
            gix[j] = -(1 << 30);
        }
    }
    // weight role: k = (tid >> 6) + 4 j of the chunk, column tid & 63
    const float* wp = w + (long)(tid >> 6) * COUT + n0 + (tid & 63);

    float ra[4], rb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + gk;
        const int tap = k / CIN, ci = k - tap * CIN;
        const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int iy = giy[j] + ky, ix = gix[j] + kx;
            float v = 0.f;
            if (k < K && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) {
                if constexpr (U8) {
                    const uint8_t* src = (const uint8_t*)in_;
                    const int cs = Cimg == 1 ? 0 : ci;
                    const float p = (float)src[gbase[j] + ((long)cs * Hi + iy) * Wi + ix];
                    const float shift = ci == 0 ? -.030f : ci == 1 ? -.088f : -.188f;
                    const float scale = ci == 0 ? .458f : ci == 1 ? .448f : .450f;
                    v = ((p / 255.f * 2.f - 1.f) - shift) / scale;
                } else {
                    const float* src = (const float*)in_;
                    v = src[gbase[j] + ((long)iy * Wi + ix) * CIN + ci];
                }
            }
            ra[j] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = wp[(long)(k0 + 4 * j) * COUT];
    };

    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, kk = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    fetch(0);
    for (int k0 = 0; k0 < KPAD; k0 += LP_KC) {
        __syncthreads();  // the previous chunk's readers are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[gk * LP_LDA + gr + 16 * j] = ra[j];
            Bs[((tid >> 6) + 4 * j) * LP_BN + (tid & 63)] = rb[j];
        }
        __syncthreads();
        if (k0 + LP_KC < KPAD) fetch(k0 + LP_KC);
#pragma unroll
        for (int s = 0; s < LP_KC / 2; ++s) {
            const float a = As[(2 * s + kk) * LP_LDA + wm * 32 + l31];
            const float b = Bs[(2 * s + kk) * LP_BN + wn * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }

    // D[i = pixel][j = co]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int co = n0 + wn * 32 + l31;
    const float bv = bias[co];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
        if (m < M) {
            const int f = m / HoWo, pix = m - f * HoWo;
            out[(long)f * out_fs + (long)pix * COUT + co] = fmaxf(acc[r] + bv, 0.f);
        }
    }
}

// 3x3 stride 2 max pool (floor, no padding) of a [f][Hi*Wi][C] map with frame pitch in_fs into a dense [f][Po*Qo][C] one
__global__ __launch_bounds__(LP_THREADS) void lpips_pool_kernel(const float* __restrict__ in, long in_fs, int Hi, int Wi,
                                                                int C, float* __restrict__ out, int Po, int Qo, long total) {
    for (long i = (long)blockIdx.x * LP_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LP_THREADS) {
        const int c = (int)(i % C);
        long t = i / C;
        const int qx = (int)(t % Qo);
        t /= Qo;
        const int py = (int)(t % Po);
        const long f = t / Po;
        const float* src = in + f * in_fs + ((long)(2 * py) * Wi + 2 * qx) * C + c;
        float v = src[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, src[((long)dy * Wi + dx) * C]);
        out[i] = v;
    }
}

// one block per frame pair; wave w takes pixels w, w + 4, ... of each tap, its lanes the channels
__global__ __launch_bounds__(LP_THREADS) void lpips_head_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                                const float* __restrict__ lin, LpHeadSizes sz,
                                                                float* __restrict__ per_layer, float* __restrict__ out) {
#pragma clang fp contract(off)  // x/da - y/db must be the exact negative of y/db - x/da
    __shared__ float sm[LP_THREADS / 64];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* a = fa + (long)n * sz.feat;
    const float* b = fb + (long)n * sz.feat;
    float total = 0.f;
    long off = 0;
    int loff = 0;
#pragma unroll
    for (int l = 0; l < LP_TAPS; ++l) {
        constexpr int Cs[LP_TAPS] = {64, 192, 384, 256, 256};
        const int C = Cs[l], P = sz.pix[l];
        float wacc = 0.f;
        for (int p = wave; p < P; p += LP_THREADS / 64) {
            const float* pa = a + off + (long)p * C;
            const float* pb = b + off + (long)p * C;
            float sa = 0.f, sb = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float x = pa[c], y = pb[c];
                sa += x * x;
                sb += y * y;
            }
            sa = wave_sum(sa);
            sb = wave_sum(sb);
            const float da = sqrtf(sa) + 1e-10f, db = sqrtf(sb) + 1e-10f;
            float s = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float d = pa[c] / da - pb[c] / db;
                s += lin[loff + c] * (d * d);
            }
            wacc += wave_sum(s);
        }
        __syncthreads();
        if (lane == 0) sm[wave] = wacc;
        __syncthreads();
        const float dl = (((sm[0] + sm[1]) + sm[2]) + sm[3]) / (float)P;
        total += dl;
        if (threadIdx.x == 0) per_layer[(long)n * LP_TAPS + l] = dl;
        off += (long)P * C;
        loff += C;
    }
    if (threadIdx.x == 0) out[n] = total;
}

struct LpWeightLayout {
    long w[LP_TAPS], b[LP_TAPS], total;
};

LpWeightLayout lp_weight_layout() {
    LpWeightLayout L;
    long o = 0;
    for (int l = 0; l < LP_TAPS; ++l) {
        L.w[l] = o;
        o += (long)lp_kpad(l) * LP_COUT[l];
        L.b[l] = o;
        o += LP_COUT[l];
    }
    L.total = o;
    return L;
}

template <int L, int STRIDE, int PAD, bool U8>
void lp_launch_conv(const void* in, long in_fs, int Cimg, int Hi, int Wi, const float* wpack, const LpWeightLayout& wl,
                    float* out, long out_fs, int Ho, int Wo, int N, hipStream_t s) {
    const int M = N * Ho * Wo;
    hipLaunchKernelGGL((lpips_conv_kernel<LP_CIN[L], LP_KS[L], STRIDE, PAD, LP_COUT[L], U8>),
                       dim3((unsigned)ceil_div(M, LP_BM), LP_COUT[L] / LP_BN), dim3(LP_THREADS), 0, s, in, in_fs, Cimg, Hi,
                       Wi, wpack + wl.w[L], wpack + wl.b[L], out, out_fs, Ho, Wo, M);
}

void lp_launch_pool(const float* in, long in_fs, int Hi, int Wi, int C, float* out, int Po, int Qo, int N, hipStream_t s) {
    const long total = (long)N * Po * Qo * C;
    long blocks = (total + LP_THREADS - 1) / LP_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, in, in_fs, Hi, Wi, C, out, Po, Qo,
                       total);
}

}  // namespace

extern "C" int rfn_lpips_alex_sizes(int H, int W, long long* out) {
    RFN_CHECK_ARG(out != nullptr, -1);
    LpSizes s;
    // the second max pool needs a 3x3 map
    RFN_CHECK_ARG(lp_sizes(H, W, &s) == 0, -2);
    for (int l = 0; l < LP_TAPS; ++l) {
        out[2 * l] = s.h[l];
        out[2 * l + 1] = s.w[l];
    }
    out[10] = s.feat;
    out[11] = s.work;
    return 0;
}

extern "C" int rfn_lpips_alex_weight_layout(long long* out) {
    RFN_CHECK_ARG(out != nullptr, -1);
    const LpWeightLayout wl = lp_weight_layout();
    for (int l = 0; l < LP_TAPS; ++l) {
        out[l] = wl.w[l];
        out[5 + l] = wl.b[l];
        out[10 + l] = lp_kpad(l);
    }
    out[15] = wl.total;
    return 0;
}

extern "C" int rfn_lpips_alex_features_u8(const void* frames, long frame_stride, int N, int C, int H, int W,
                                          const float* wpack, long wpack_floats, float* feats_out, float* workspace,
                                          long workspace_floats, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0, -1);
    RFN_CHECK_ARG(C == 1 || C == 3, -2);
    LpSizes z;
    RFN_CHECK_ARG(lp_sizes(H, W, &z) == 0, -3);
    if (N == 0) return 0;
    const LpWeightLayout wl = lp_weight_layout();
    RFN_CHECK_ARG(frames && wpack && feats_out && workspace, -4);
    RFN_CHECK_ARG(wpack_floats == wl.total, -5);
    RFN_CHECK_ARG(frame_stride >= (long)C * H * W, -6);
    RFN_CHECK_ARG(workspace_floats >= (long)N * z.work, -7);
    // GEMM rows are counted in int
    RFN_CHECK_ARG((long)N * z.h[0] * z.w[0] <= (1L << 30), -8);
    hipStream_t s = (hipStream_t)stream;
    const long F = z.feat;
    float* tap[LP_TAPS];
    long o = 0;
    for (int l = 0; l < LP_TAPS; ++l) {
        tap[l] = feats_out + o;
        o += (long)z.h[l] * z.w[l] * LP_COUT[l];
    }
    const long p1 = (long)z.ph[0] * z.pw[0] * LP_COUT[0], p2 = (long)z.ph[1] * z.pw[1] * LP_COUT[1];
    float* ws1 = workspace;
    float* ws2 = workspace + (long)N * p1;

    lp_launch_conv<0, 4, 2, true>(frames, frame_stride, C, H, W, wpack, wl, tap[0], F, z.h[0], z.w[0], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_pool(tap[0], F, z.h[0], z.w[0], LP_COUT[0], ws1, z.ph[0], z.pw[0], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_conv<1, 1, 2, false>(ws1, p1, 0, z.ph[0], z.pw[0], wpack, wl, tap[1], F, z.h[1], z.w[1], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_pool(tap[1], F, z.h[1], z.w[1], LP_COUT[1], ws2, z.ph[1], z.pw[1], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_conv<2, 1, 1, false>(ws2, p2, 0, z.ph[1], z.pw[1], wpack, wl, tap[2], F, z.h[2], z.w[2], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_conv<3, 1, 1, false>(tap[2], F, 0, z.h[2], z.w[2], wpack, wl, tap[3], F, z.h[3], z.w[3], N, s);
    RFN_LAUNCH_CHECK();
    lp_launch_conv<4, 1, 1, false>(tap[3], F, 0, z.h[3], z.w[3], wpack, wl, tap[4], F, z.h[4], z.w[4], N, s);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_lpips_alex_distance(const float* feats_a, const float* feats_b, const float* lin, int N, int H, int W,
                                       float* per_layer_out, float* out, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0, -1);
    LpSizes z;
    RFN_CHECK_ARG(lp_sizes(H, W, &z) == 0, -2);
    if (N == 0) return 0;
    RFN_CHECK_ARG(feats_a && feats_b && lin && per_layer_out && out, -3);
    LpHeadSizes hs;
    for (int l = 0; l < LP_TAPS; ++l) hs.pix[l] = z.h[l] * z.w[l];
    hs.feat = z.feat;
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)N), dim3(LP_THREADS), 0, (hipStream_t)stream, feats_a, feats_b,
                       lin, hs, per_layer_out, out);
    RFN_LAUNCH_CHECK();
    return 0;
}
