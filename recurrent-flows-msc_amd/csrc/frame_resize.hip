// Frames of any size and channel count into the geometry of a frame store: the ingest step of
// data_generators/clip_folder.py, once per dataset.
//
//   src : uint8 [F, Hs, Ws, Cs], channel-interleaved (Cs = 1 or 3)
//   dst : uint8 [F, H, W, Cd]  (Cd = 1 or 3)
//   crop window (y0, x0, Hc, Wc) inside the source frame
//
// Exact integer area mean, rounded half up.  Output row y covers [y*Hc, (y+1)*Hc) on a grid where cropped source row i
// covers [i*H, (i+1)*H): wy(i) = min((y+1)*Hc, (i+1)*H) - max(y*Hc, i*H) for i = floor(y*Hc/H) .. ceil((y+1)*Hc/H) - 1,
// every wy(i) > 0 and their sum is Hc; wx(j) alike with W, Wc.  Per stored channel
//   out = (sum_i sum_j wy(i) * wx(j) * src[y0+i, x0+j, c] + (Hc*Wc)/2) / (Hc*Wc)
// and then, on the rounded bytes, 3 -> 1 channels as (19595 R + 38470 G + 7471 B + 32768) >> 16, 1 -> 3 as copies.
// All sizes are at most 32768, so every product of a position and a size fits an int; a row's sum_j wx(j) * byte is at
// most 255 * Wc (uint32), the sum over rows is kept in 64 bits.
//
// One workgroup per (frame, band of RB output rows); it walks the band in tiles of XT columns, RB * XT <= 256, one lane
// per output pixel.  The source rectangle under a tile is staged in LDS in passes of at most FR_SEG bytes of a row and
// as many rows as FR_STAGE bytes hold, and every lane adds the part of its footprint that the pass holds: a pixel may
// lie under any number of passes, so no source size is too large.  16-byte loads when the base is 16-byte aligned and
// the row pitch Ws*Cs a multiple of 16 (the staged range of a row is widened to 16-byte bounds, which stay inside the
// row), single bytes otherwise.  No atomics, no scratch.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_STAGE = 8192;   // bytes of LDS of one pass
constexpr int FR_SEG = 2048;     // most bytes of one source row in a pass, the 16-byte widening included
constexpr int FR_MAX_SIDE = 32768;

template <int CS>
__global__ __launch_bounds__(FR_THREADS) void frames_resize_kernel(const uint8_t* __restrict__ src,
                                                                   uint8_t* __restrict__ dst, int Hs, int Ws, int H,
                                                                   int W, int Cd, int y0, int x0, int Hc, int Wc,
                                                                   int RB, int XT, int bands, int vec) {
    __shared__ uint4 stage4[FR_STAGE / 16];
    const uint8_t* stage = reinterpret_cast<const uint8_t*>(stage4);

    const int tid = threadIdx.x;
    const unsigned f = blockIdx.x / (unsigned)bands;
    const int yb = (int)(blockIdx.x - f * (unsigned)bands) * RB;
    const int ye = yb + RB < H ? yb + RB : H;
    const long pitch = (long)Ws * CS;
    const uint8_t* fsrc = src + (long)f * Hs * pitch + (long)y0 * pitch;
    uint8_t* fdst = dst + (long)f * H * W * Cd;

    const int ty = tid / XT, tx = tid - ty * XT;
    const int y = yb + ty;
    const bool row_on = ty < RB && y < ye;
    // the band's source rows and this lane's (window coordinates)
    const int I0 = yb * Hc / H, I1 = (ye * Hc + H - 1) / H - 1;
    const int i_lo = row_on ? y * Hc / H : 0, i_hi = row_on ? ((y + 1) * Hc + H - 1) / H - 1 : -1;
    const uint32_t area = (uint32_t)Hc * (uint32_t)Wc;
    constexpr int SEG_PIX = (FR_SEG - 32) / CS;

    for (int xb = 0; xb < W; xb += XT) {
        const int xe = xb + XT < W ? xb + XT : W;
        const int x = xb + tx;
        const bool on = row_on && x < xe;
        const int J0 = xb * Wc / W, J1 = (xe * Wc + W - 1) / W - 1;
        const int j_lo = on ? x * Wc / W : 0, j_hi = on ? ((x + 1) * Wc + W - 1) / W - 1 : -1;
        unsigned long long acc[CS];
#pragma unroll
        for (int c = 0; c < CS; ++c) acc[c] = 0;

        for (int jb = J0; jb <= J1; jb += SEG_PIX) {
            const int je = jb + SEG_PIX - 1 < J1 ? jb + SEG_PIX - 1 : J1;
            const int b0 = (x0 + jb) * CS, b1 = (x0 + je + 1) * CS;   // the pass's bytes of a source row
            const int a0 = vec ? b0 & ~15 : b0, a1 = vec ? (b1 + 15) & ~15 : b1;
            const int seg = a1 - a0;                                   // <= FR_SEG
            const int rows = FR_STAGE / seg;
            for (int ib = I0; ib <= I1; ib += rows) {
                const int ie = ib + rows - 1 < I1 ? ib + rows - 1 : I1;
                const int nr = ie - ib + 1;
                __syncthreads();   // the pass before has been read
                if (vec) {
                    const int n16 = seg >> 4;
                    for (int k = tid; k < nr * n16; k += FR_THREADS) {
                        const int r = k / n16, q = k - r * n16;
                        stage4[k] = *reinterpret_cast<const uint4*>(fsrc + (long)(ib + r) * pitch + a0 + 16 * q);
                    }
                } else {
                    uint8_t* st = reinterpret_cast<uint8_t*>(stage4);
                    for (int k = tid; k < nr * seg; k += FR_THREADS) {
                        const int r = k / seg, q = k - r * seg;
                        st[k] = fsrc[(long)(ib + r) * pitch + a0 + q];
                    }
                }
                __syncthreads();
                const int ia = i_lo > ib ? i_lo : ib, iz = i_hi < ie ? i_hi : ie;
                const int ja = j_lo > jb ? j_lo : jb, jz = j_hi < je ? j_hi : je;
                for (int i = ia; i <= iz; ++i) {
                    const int top = y * Hc > i * H ? y * Hc : i * H;
                    const int bot = (y + 1) * Hc < (i + 1) * H ? (y + 1) * Hc : (i + 1) * H;
                    const uint8_t* row = stage + (i - ib) * seg + (b0 - a0) - jb * CS;
                    uint32_t r[CS];
#pragma unroll
                    for (int c = 0; c < CS; ++c) r[c] = 0;
                    for (int j = ja; j <= jz; ++j) {
                        const int lft = x * Wc > j * W ? x * Wc : j * W;
                        const int rgt = (x + 1) * Wc < (j + 1) * W ? (x + 1) * Wc : (j + 1) * W;
#pragma unroll
                        for (int c = 0; c < CS; ++c) r[c] += (uint32_t)(rgt - lft) * row[j * CS + c];
                    }
#pragma unroll
                    for (int c = 0; c < CS; ++c) acc[c] += (unsigned long long)(uint32_t)(bot - top) * r[c];
                }
            }
        }

        if (on) {
            uint32_t v[CS];
#pragma unroll
            for (int c = 0; c < CS; ++c) {
                const unsigned long long s = acc[c] + (area >> 1);
                // (32-bit division where the rounded sum fits: 256 * Hc * Wc <= 2^32)
                v[c] = area <= (1u << 24) ? (uint32_t)s / area : (uint32_t)(s / area);
            }
            uint8_t* o = fdst + ((long)y * W + x) * Cd;
            if constexpr (CS == 3) {
                if (Cd == 1) {
                    o[0] = (uint8_t)((19595u * v[0] + 38470u * v[1] + 7471u * v[2] + 32768u) >> 16);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
                }
            } else {
                for (int c = 0; c < Cd; ++c) o[c] = (uint8_t)v[0];
            }
        }
    }
}

}  // namespace

extern "C" int rfn_frames_resize_u8(const void* src, long dst_addr, long F, int Hs, int Ws, int Cs, int H, int W, int Cd,
                                    int y0, int x0, int Hc, int Wc, rfn_stream_t stream) {
    RFN_CHECK_ARG(F >= 0 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, -1);
    RFN_CHECK_ARG(Hs <= FR_MAX_SIDE && Ws <= FR_MAX_SIDE && H <= FR_MAX_SIDE && W <= FR_MAX_SIDE, -1);
    RFN_CHECK_ARG((Cs == 1 || Cs == 3) && (Cd == 1 || Cd == 3), -2);
    RFN_CHECK_ARG(Hc >= 1 && Wc >= 1 && y0 >= 0 && x0 >= 0 && y0 <= Hs - Hc && x0 <= Ws - Wc, -3);
    const int XT = W < FR_THREADS ? W : FR_THREADS;
    int RB = FR_THREADS / XT;
    if (RB > H) RB = H;
    const int bands = (H + RB - 1) / RB;
    RFN_CHECK_ARG(F * bands <= 0x7fffffffL, -4);
    if (F == 0) return 0;
    RFN_CHECK_ARG(src && dst_addr, -5);
    uint8_t* dst = reinterpret_cast<uint8_t*>(dst_addr);
    const int vec = ((uintptr_t)src & 15) == 0 && ((long)Ws * Cs) % 16 == 0;
    const dim3 grid((unsigned)(F * bands)), block(FR_THREADS);
    if (Cs == 1)
        hipLaunchKernelGGL(frames_resize_kernel<1>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)src,
                           dst, Hs, Ws, H, W, Cd, y0, x0, Hc, Wc, RB, XT, bands, vec);
    else
        hipLaunchKernelGGL(frames_resize_kernel<3>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)src,
                           dst, Hs, Ws, H, W, Cd, y0, x0, Hc, Wc, RB, XT, bands, vec);
    RFN_LAUNCH_CHECK();
    return 0;
}
