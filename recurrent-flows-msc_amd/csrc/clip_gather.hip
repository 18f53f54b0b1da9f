// Clips of a device-resident frame store as float32 batches: the per-item work of the reference's two file-backed
// datasets (data_generators/bair_push.py:66-109, data_generators/kth.py:34-65) and the collation of its DataLoader
// (RFN/trainer.py:132-161), for a whole batch in one launch.
//
//   store : uint8 [n_frames, H, W, Cs], channel-interleaved as an image decoder leaves it (Cs = 1 or 3)
//   first : int64 [B], the store index of each clip's first frame
//   out   : fp32 [B, T, C, H, W];  out[b,t,c,y,x] = float32(store[first[b]+t, y, x, c']) / float32(255)
//           c' = c when C == Cs; c' = 0 when Cs == 1 (C copies of the one plane)
//
// Pixels: the quotient is the correctly rounded float32 division, read from a 256-entry table built as in
// moving_mnist.hip.  It is BAIR's `astype(float32) / 255.` and also KTH's float64 `/ 255.` followed by `.float()`:
// float32(k) / float32(255) == float32(k / 255.) for all 256 bytes.
//
// Guard: a clip with first[b] < 0 or first[b] + T > n_frames reads nothing and all its T frames are NaN.
//
// One workgroup per (clip, frame, run of 1024 pixels).  Vector path (H*W a multiple of 4, the frame's byte count a
// multiple of 16, 16-byte aligned bases): the run's 1024 * Cs bytes arrive as one 16-byte load per lane, are parked in
// LDS, and lane q picks up the Cs dwords of pixels 4q .. 4q+3 (dword stride Cs, odd or 1: no bank conflict) and stores
// one float4 per channel plane, so that every store instruction of a wave writes 1 KiB of one plane.  Otherwise every
// lane handles single pixels.  No atomics, no scratch.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_PIX = 4 * CG_THREADS;   // pixels of one workgroup: one float4 per lane and channel plane

template <int CS>
__global__ __launch_bounds__(CG_THREADS) void clip_gather_kernel(const uint8_t* __restrict__ store, long n_frames,
                                                                 const long long* __restrict__ first,
                                                                 float* __restrict__ out, int T, int C, int HW,
                                                                 int chunks, int vec) {
    __shared__ float lut[256];
    __shared__ uint4 raw[CG_PIX * CS / 16];

    const int tid = threadIdx.x;
    const unsigned frame = blockIdx.x / (unsigned)chunks;
    const int p0 = (int)(blockIdx.x - frame * (unsigned)chunks) * CG_PIX;
    const unsigned b = frame / (unsigned)T;
    const int t = (int)(frame - b * (unsigned)T);
    const int n = HW - p0 < CG_PIX ? HW - p0 : CG_PIX;   // pixels of this run (a multiple of 4 on the vector path)
    float* dst = out + (long)frame * C * HW + p0;

    const long long f0 = first[b];
    if (f0 < 0 || f0 > (long long)n_frames - T) {   // (uniform over the workgroup) nothing is read
        const float q = __int_as_float(0x7fc00000);
        if (vec) {
            if (4 * tid < n)
                for (int c = 0; c < C; ++c) reinterpret_cast<float4*>(dst + (long)c * HW)[tid] = make_float4(q, q, q, q);
        } else {
            for (int p = tid; p < n; p += CG_THREADS)
                for (int c = 0; c < C; ++c) dst[(long)c * HW + p] = q;
        }
        return;
    }

    // k / 255 in float32, correctly rounded: the fp64 quotient is within 2^-53 (relative) of k / 255, which is never
    // that close to a float32 rounding boundary
    lut[tid] = (float)((double)tid / 255.0);
    const uint8_t* src = store + ((long)(f0 + t) * HW + p0) * CS;

    if (vec) {
        if (16 * tid < n * CS) raw[tid] = reinterpret_cast<const uint4*>(src)[tid];
        __syncthreads();
        if (4 * tid < n) {
            uint32_t w[CS];
#pragma unroll
            for (int k = 0; k < CS; ++k) w[k] = reinterpret_cast<const uint32_t*>(raw)[CS * tid + k];
            // byte m of the lane's 4 * CS: pixel m / CS, channel m % CS
            auto px = [&](int m) { return lut[(w[m >> 2] >> (8 * (m & 3))) & 0xffu]; };
            if (CS == 1) {
                const float4 v = make_float4(px(0), px(1), px(2), px(3));
                for (int c = 0; c < C; ++c) reinterpret_cast<float4*>(dst + (long)c * HW)[tid] = v;
            } else {
#pragma unroll
                for (int c = 0; c < CS; ++c)
                    reinterpret_cast<float4*>(dst + (long)c * HW)[tid] =
                        make_float4(px(c), px(CS + c), px(2 * CS + c), px(3 * CS + c));
            }
        }
    } else {
        __syncthreads();
        for (int p = tid; p < n; p += CG_THREADS)
            for (int c = 0; c < C; ++c) dst[(long)c * HW + p] = lut[src[(long)p * CS + (CS == 1 ? 0 : c)]];
    }
}

}  // namespace

extern "C" int rfn_clip_gather_u8_f32(const void* store, long n_frames, const void* first, float* out, int B, int T,
                                      int C, int Cs, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 0 && T >= 1 && H >= 1 && W >= 1 && n_frames >= 0, -1);
    RFN_CHECK_ARG((Cs == 1 && (C == 1 || C == 3)) || (Cs == 3 && C == 3), -2);
    RFN_CHECK_ARG((long)H * W <= 0x7fffffffL / 4, -3);
    const int HW = H * W;
    const int chunks = (HW + CG_PIX - 1) / CG_PIX;
    RFN_CHECK_ARG((long)B * T * chunks <= 0x7fffffffL, -4);
    if (B == 0) return 0;
    RFN_CHECK_ARG(store && first && out, -5);
    const int vec = HW % 4 == 0 && ((long)HW * Cs) % 16 == 0 && ((uintptr_t)store & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)((long)B * T * chunks)), block(CG_THREADS);
    if (Cs == 1)
        hipLaunchKernelGGL(clip_gather_kernel<1>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)store, n_frames,
                           (const long long*)first, out, T, C, HW, chunks, vec);
    else
        hipLaunchKernelGGL(clip_gather_kernel<3>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)store, n_frames,
                           (const long long*)first, out, T, C, HW, chunks, vec);
    RFN_LAUNCH_CHECK();
    return 0;
}

// ---- the same gather with a temporal stride and two per-clip augmentations (data_generators/clip_folder.py)
//
//   step  : frames between two frames of a clip (>= 1)
//   flags : int32 [B] or NULL (all 0): bit 0 mirrors x, bit 1 reverses time; other bits are ignored
//   out[b,t,c,y,x] = lut[ store[first[b] + tt*step, y, xx, c'] ],  tt = bit1 ? T-1-t : t,  xx = bit0 ? W-1-x : x
//
// Guard: a clip with first[b] < 0 or first[b] + (T-1)*step + 1 > n_frames reads nothing and is all NaN.  With
// flags == NULL and step == 1 every output bit is clip_gather_kernel's.
//
// The workgroup's run of 1024 pixels is a run of the SOURCE frame, loaded and parked in LDS exactly as above; a lane
// then holds four neighbouring source pixels.  Where W % 4 == 0 they lie in one row, so their mirror images are four
// neighbouring output pixels: the lane reverses them in registers and stores one float4 per plane at the mirrored group
// of that row (a wave still writes whole 1 KiB stretches of a plane, the groups of each row in descending order).  A
// mirrored clip of any other width, and whatever the kernel above handles pixel by pixel, goes pixel by pixel.
namespace {

template <int CS>
__global__ __launch_bounds__(CG_THREADS) void clip_gather_aug_kernel(const uint8_t* __restrict__ store, long n_frames,
                                                                     const long long* __restrict__ first,
                                                                     const int* __restrict__ flags,
                                                                     float* __restrict__ out, int T, int C, int W,
                                                                     int HW, int step, int chunks, int vec) {
    __shared__ float lut[256];
    __shared__ uint4 raw[CG_PIX * CS / 16];

    const int tid = threadIdx.x;
    const unsigned frame = blockIdx.x / (unsigned)chunks;
    const int p0 = (int)(blockIdx.x - frame * (unsigned)chunks) * CG_PIX;   // first source pixel of the run
    const unsigned b = frame / (unsigned)T;
    const int t = (int)(frame - b * (unsigned)T);
    const int n = HW - p0 < CG_PIX ? HW - p0 : CG_PIX;
    float* dst = out + (long)frame * C * HW;                                  // the output frame (b, t)

    const long long f0 = first[b];
    const int fl = flags ? flags[b] : 0;                                      // (uniform over the workgroup)
    const bool mirror = fl & 1;
    if (f0 < 0 || f0 > (long long)n_frames - 1 - (long long)(T - 1) * step) {   // nothing is read
        const float q = __int_as_float(0x7fc00000);
        if (vec) {
            if (4 * tid < n)
                for (int c = 0; c < C; ++c)
                    reinterpret_cast<float4*>(dst + (long)c * HW + p0)[tid] = make_float4(q, q, q, q);
        } else {
            for (int p = tid; p < n; p += CG_THREADS)
                for (int c = 0; c < C; ++c) dst[(long)c * HW + p0 + p] = q;
        }
        return;
    }

    lut[tid] = (float)((double)tid / 255.0);   // as above
    const int tt = fl & 2 ? T - 1 - t : t;
    const uint8_t* src = store + ((long)(f0 + (long long)tt * step) * HW + p0) * CS;

    if (vec && (!mirror || W % 4 == 0)) {
        if (16 * tid < n * CS) raw[tid] = reinterpret_cast<const uint4*>(src)[tid];
        __syncthreads();
        if (4 * tid < n) {
            uint32_t w[CS];
#pragma unroll
            for (int k = 0; k < CS; ++k) w[k] = reinterpret_cast<const uint32_t*>(raw)[CS * tid + k];
            auto px = [&](int m) { return lut[(w[m >> 2] >> (8 * (m & 3))) & 0xffu]; };
            int g = (p0 >> 2) + tid;           // the group of four pixels in the frame: source, then output
            if (mirror) {
                const int gw = W >> 2, gy = g / gw;
                g = gy * gw + (gw - 1 - (g - gy * gw));
            }
            if (CS == 1) {
                const float4 v = mirror ? make_float4(px(3), px(2), px(1), px(0)) : make_float4(px(0), px(1), px(2), px(3));
                for (int c = 0; c < C; ++c) reinterpret_cast<float4*>(dst + (long)c * HW)[g] = v;
            } else {
#pragma unroll
                for (int c = 0; c < CS; ++c)
                    reinterpret_cast<float4*>(dst + (long)c * HW)[g] =
                        mirror ? make_float4(px(3 * CS + c), px(2 * CS + c), px(CS + c), px(c))
                               : make_float4(px(c), px(CS + c), px(2 * CS + c), px(3 * CS + c));
            }
        }
    } else {
        __syncthreads();
        for (int p = tid; p < n; p += CG_THREADS) {
            int o = p0 + p;
            if (mirror) {
                const int y = o / W;
                o = y * W + (W - 1 - (o - y * W));
            }
            for (int c = 0; c < C; ++c) dst[(long)c * HW + o] = lut[src[(long)p * CS + (CS == 1 ? 0 : c)]];
        }
    }
}

}  // namespace

extern "C" int rfn_clip_gather_aug_u8_f32(const void* store, long n_frames, const void* first, const void* flags,
                                          float* out, int B, int T, int C, int Cs, int H, int W, int step,
                                          rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 0 && T >= 1 && H >= 1 && W >= 1 && n_frames >= 0 && step >= 1, -1);
    RFN_CHECK_ARG((Cs == 1 && (C == 1 || C == 3)) || (Cs == 3 && C == 3), -2);
    RFN_CHECK_ARG((long)H * W <= 0x7fffffffL / 4, -3);
    const int HW = H * W;
    const int chunks = (HW + CG_PIX - 1) / CG_PIX;
    RFN_CHECK_ARG((long)B * T * chunks <= 0x7fffffffL, -4);
    if (B == 0) return 0;
    RFN_CHECK_ARG(store && first && out, -5);
    RFN_CHECK_ARG(!flags || ((uintptr_t)flags & 3) == 0, -6);
    const int vec = HW % 4 == 0 && ((long)HW * Cs) % 16 == 0 && ((uintptr_t)store & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)((long)B * T * chunks)), block(CG_THREADS);
    if (Cs == 1)
        hipLaunchKernelGGL(clip_gather_aug_kernel<1>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)store,
                           n_frames, (const long long*)first, (const int*)flags, out, T, C, W, HW, step, chunks, vec);
    else
        hipLaunchKernelGGL(clip_gather_aug_kernel<3>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)store,
                           n_frames, (const long long*)first, (const int*)flags, out, T, C, W, HW, step, chunks, vec);
    RFN_LAUNCH_CHECK();
    return 0;
}
