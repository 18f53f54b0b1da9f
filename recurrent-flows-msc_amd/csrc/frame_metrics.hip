// Per-frame video-prediction quality metrics (evaluation_metrics/error_metrics.py:154-171 of the reference, which scores
// every frame with skimage 0.17.2 one channel at a time in a Python loop on the CPU): MSE, PSNR and SSIM of uint8 frames.
//
// SSIM is skimage's `structural_similarity` with its defaults on uint8: 7x7 uniform window, data_range 255, K1 = 0.01,
// K2 = 0.03, sample covariance (x 49/48), S map averaged over the interior (H-6) x (W-6) (skimage crops the 3 pixels
// whose windows touch the reflected border).  Exactness: the window sums Sx, Sy, Sxx, Syy, Sxy of integer pixels are
// exact in int32 (<= 49 * 255^2), and so are the scaled (co)variances 49*Sxx - Sx^2 (<= 49^2 * 255^2 < 2^31); the S
// formula with its mean factors scaled by 49^2 and its (co)variance factors by 49 * 48 then runs in fp64 from these
// exact integers:
//   S = (2 Sx Sy + C1 * 49^2) (2 (49 Sxy - Sx Sy) + C2 * 49 * 48) / ((Sx^2 + Sy^2 + C1 * 49^2)
//       (49 Sxx - Sx^2 + 49 Syy - Sy^2 + C2 * 49 * 48)),   C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
// The squared-error sums are exact in uint64.  One workgroup per frame, reductions in a fixed order inside the
// workgroup, no atomics: the results are bit-reproducible.
//
// Large frames are walked in tiles of TH x TW output pixels (the 7-row column sums of a tile live in LDS: LDS use is
// bounded whatever the frame size).
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int FQ_THREADS = 256;
constexpr int FQ_WIN = 7;
constexpr int FQ_TH = 16;                // output rows per tile
constexpr int FQ_TW = 64;                // output columns per tile
constexpr int FQ_VW = FQ_TW + FQ_WIN - 1;  // columns of the column sums of a tile

__device__ __forceinline__ double block_sum_d(double v, double* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(FQ_THREADS) void frame_quality_u8_kernel(const uint8_t* __restrict__ a, long a_ns,
                                                                      const uint8_t* __restrict__ b, long b_ns,
                                                                      float* __restrict__ mse, float* __restrict__ psnr,
                                                                      float* __restrict__ ssim, int C, int H, int W) {
    // column sums over 7 rows of x, y, x^2, y^2, xy for the TH output rows of the current tile
    __shared__ int vx[FQ_TH][FQ_VW], vy[FQ_TH][FQ_VW], vxx[FQ_TH][FQ_VW], vyy[FQ_TH][FQ_VW], vxy[FQ_TH][FQ_VW];
    __shared__ double sm_d[FQ_THREADS / 64];
    __shared__ unsigned long long sm_u[FQ_THREADS / 64];

    const int n = blockIdx.x;
    const long HW = (long)H * W;
    const int Ho = H - (FQ_WIN - 1), Wo = W - (FQ_WIN - 1);
    const double C1s = (0.01 * 255.0) * (0.01 * 255.0) * 2401.0;  // C1 * 49^2
    const double C2s = (0.03 * 255.0) * (0.03 * 255.0) * 2352.0;  // C2 * 49 * 48

    unsigned long long sse_all = 0;
    double psnr_sum = 0.0, ssim_sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const uint8_t* __restrict__ x = a + (long)n * a_ns + (long)c * HW;
        const uint8_t* __restrict__ y = b + (long)n * b_ns + (long)c * HW;

        // squared error of the channel (exact)
        unsigned long long sse = 0;
        for (long i = threadIdx.x; i < HW; i += FQ_THREADS) {
            const int d = (int)x[i] - (int)y[i];
            sse += (unsigned long long)(d * d);
        }
        sse = block_sum_u64(sse, sm_u);

        // SSIM: sum of the S map over the interior, tile by tile
        double s_acc = 0.0;
        for (int r0 = 0; r0 < Ho; r0 += FQ_TH) {
            for (int c0 = 0; c0 < Wo; c0 += FQ_TW) {
                __syncthreads();  // the previous tile's readers are done with the column sums
                for (int k = threadIdx.x; k < FQ_TH * FQ_VW; k += FQ_THREADS) {
                    const int i = k / FQ_VW, j = k - i * FQ_VW;
                    const int row = r0 + i, col = c0 + j;
                    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
                    if (row < Ho && col < W) {
                        const uint8_t* px = x + (long)row * W + col;
                        const uint8_t* py = y + (long)row * W + col;
#pragma unroll
                        for (int t = 0; t < FQ_WIN; ++t) {
                            const int u = px[(long)t * W], v = py[(long)t * W];
                            sx += u;
                            sy += v;
                            sxx += u * u;
                            syy += v * v;
                            sxy += u * v;
                        }
                    }
                    vx[i][j] = sx;
                    vy[i][j] = sy;
                    vxx[i][j] = sxx;
                    vyy[i][j] = syy;
                    vxy[i][j] = sxy;
                }
                __syncthreads();
                for (int k = threadIdx.x; k < FQ_TH * FQ_TW; k += FQ_THREADS) {
                    const int i = k / FQ_TW, j = k - i * FQ_TW;
                    if (r0 + i >= Ho || c0 + j >= Wo) continue;
                    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
                    for (int t = 0; t < FQ_WIN; ++t) {
                        sx += vx[i][j + t];
                        sy += vy[i][j + t];
                        sxx += vxx[i][j + t];
                        syy += vyy[i][j + t];
                        sxy += vxy[i][j + t];
                    }
                    const int pxy = sx * sy;                          // <= (49*255)^2 < 2^31
                    const int covs = 49 * sxy - pxy;                  // 49*48 * sample covariance
                    const int vars = (49 * sxx - sx * sx) + (49 * syy - sy * sy);
                    const double num = (2.0 * (double)pxy + C1s) * (2.0 * (double)covs + C2s);
                    const double den = ((double)sx * sx + (double)sy * sy + C1s) * ((double)vars + C2s);
                    s_acc += num / den;
                }
            }
        }
        s_acc = block_sum_d(s_acc, sm_d);

        sse_all += sse;
        // skimage: 10 log10(data_range^2 / mean((x - y)^2)); +inf (numpy's division by zero) on identical channels
        psnr_sum += sse == 0 ? (double)INFINITY : 10.0 * log10(65025.0 / ((double)sse / (double)HW));
        ssim_sum += s_acc / ((double)Ho * (double)Wo);
    }
    if (threadIdx.x == 0) {
        mse[n] = (float)((double)sse_all / ((double)C * (double)HW));
        psnr[n] = (float)(psnr_sum / C);
        ssim[n] = (float)(ssim_sum / C);
    }
}

}  // namespace

extern "C" int rfn_frame_quality_u8(const void* a, long a_ns, const void* b, long b_ns, float* mse, float* psnr,
                                    float* ssim, int N, int C, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(N >= 0 && C >= 1, -1);
    // skimage: "win_size exceeds image extent"
    RFN_CHECK_ARG(H >= FQ_WIN && W >= FQ_WIN, -2);
    // the 7x7 window sums are exact in int32 for any frame size; the squared error of a channel (<= 255^2 * H*W) and
    // the S-map sum must stay exact / meaningful in uint64 and fp64
    RFN_CHECK_ARG((long)H * W <= (1L << 40), -3);
    if (N == 0) return 0;
    RFN_CHECK_ARG(a && b && mse && psnr && ssim, -4);
    RFN_CHECK_ARG(a_ns >= (long)C * H * W && b_ns >= (long)C * H * W, -5);
    hipLaunchKernelGGL(frame_quality_u8_kernel, dim3((unsigned)N), dim3(FQ_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)a, a_ns, (const uint8_t*)b, b_ns, mse, psnr, ssim, C, H, W);
    RFN_LAUNCH_CHECK();
    return 0;
}
