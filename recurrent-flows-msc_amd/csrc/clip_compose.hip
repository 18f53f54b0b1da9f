// An animation of prediction draws as 8-bit RGB pixels, all T frames composed on the device in one launch: every frame
// is a grid of R x N cells like a sheet (sheet.hip), each cell a sequence of frames that moves with t -- the ground
// truth, one draw, the MEAN of a group of draws or their SPREAD -- zoomed, with a coloured ring around it that switches
// colour where the given frames end and the generated ones begin (the coloured subplot frames of the reference's
// figures).  DESIGN.md section 28 is the pixel contract; include/rfn_hip.h states it at rfn_clip_compose_u8.
//
//   frame : R x N cells of Hc x Wc = (zoom*H + 2*border) x (zoom*W + 2*border) pixels, `gutter` pixels of the grey `bg`
//           between the cells and around the grid: Hs = R*Hc + (R+1)*gutter, Ws = N*Wc + (N+1)*gutter.
//   cells : DEVICE table of R*N records of eight int64 words (cell (r, i) at r*N + i):
//           w0 byte address of member 0, frame 0;  w1, w2 elements between frames / between group members;  w3 count
//           (0: an empty cell, all bg);  w4 group size G;  w5 kind | mode << 8 | gain << 16;  w6 switch_at;
//           w7 rgb_before | rgb_after << 32.
//   out   : lead = 0: uint8 [T, Hs, Ws, 3];  lead = 1: [T, Hs, 1 + 3*Ws], byte 0 of every line 0: T raw PNG streams.
//
// One workgroup per (t, line), as sheet.hip has one per line: a lane owns one aligned dword of the line at a time and
// stores its four bytes at once; the ragged ends of a line, which starts at any byte address, are byte stores of the
// first lanes.  A byte finds its cell from its x, reads the cell's record from the table (the same cache lines for the
// whole workgroup) and sums the G member bytes in member order in integers.  Every byte of `out` is written exactly
// once, nothing outside it; only listed frames are read.  No atomics, no LDS, no scratch.
#include "common.h"
#include "pixel_quant.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int CLIP_THREADS = 256;

struct ClipGeom {
    int R, N, C, H, W, zoom, border, gutter, bg, lead, range_half;
    int Hc, Wc, Hs;  // cell and frame extents in pixels
    int line;        // bytes of one output line: lead + 3*Ws
    float n_bins;    // 2^n_bits
    float scale;     // 256 / 2^n_bits
};

// floor(sqrt(v)), v < 2^52: the double root is within one of it, the two loops settle the last unit
__device__ __forceinline__ unsigned long long clip_isqrt(unsigned long long v) {
    unsigned long long r = (unsigned long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// byte `xb` of a line of frame t; row = the records of the line's cell row (nullptr: a gutter line), cy = the line's
// y inside the cell
__device__ __forceinline__ uint32_t clip_byte(int xb, const ClipGeom& g, const long long* __restrict__ row, int cy,
                                              int t) {
    xb -= g.lead;
    if (xb < 0) return 0u;                      // the filter-type byte of a scanline
    const int px = xb / 3, ch = xb - 3 * px;
    const int cx = px - g.gutter;
    if (row == nullptr || cx < 0) return (uint32_t)g.bg;
    const int pitch = g.Wc + g.gutter;
    const int i = cx / pitch, xx = cx - i * pitch;
    if (xx >= g.Wc || i >= g.N) return (uint32_t)g.bg;
    const long long* rec = row + 8L * i;
    const long long count = rec[3];
    if (count <= 0) return (uint32_t)g.bg;      // an empty cell, border included
    const int by = cy - g.border, bx = xx - g.border;
    if (by < 0 || bx < 0 || by >= g.zoom * g.H || bx >= g.zoom * g.W) {   // the ring
        const unsigned long long rgb2 = (unsigned long long)rec[7];
        const uint32_t rgb = (long long)t < rec[6] ? (uint32_t)rgb2 : (uint32_t)(rgb2 >> 32);
        return (rgb >> (8 * ch)) & 255u;
    }
    const int sy = by / g.zoom, sx = bx / g.zoom;
    const long long f = (long long)t < count ? (long long)t : count - 1;
    const long long step_g = rec[2];
    const int G = (int)rec[4];
    const int w5 = (int)rec[5];
    const int kind = w5 & 255, mode = (w5 >> 8) & 255, gain = (w5 >> 16) & 255;
    long long e = f * rec[1] + (g.C == 3 ? (long long)ch * g.H * g.W : 0LL) + (long long)sy * g.W + sx;
    const uint8_t* base8 = reinterpret_cast<const uint8_t*>(rec[0]);
    const float* base32 = reinterpret_cast<const float*>(rec[0]);
    const int n = mode == 0 ? 1 : G;
    unsigned long long s1 = 0, s2 = 0;
    for (int m = 0; m < n; ++m, e += step_g) {
        const unsigned long long b = kind == 1 ? (unsigned long long)base8[e]
                                               : (unsigned long long)rfn_quantise_u8(base32[e], g.range_half, g.n_bins, g.scale);
        s1 += b;
        s2 += b * b;
    }
    if (mode == 0) return (uint32_t)s1;
    const unsigned long long Gu = (unsigned long long)G;
    if (mode == 1) return (uint32_t)((s1 + Gu / 2) / Gu);
    const unsigned long long sd = clip_isqrt((unsigned long long)(gain * gain) * (Gu * s2 - s1 * s1)) / Gu;
    return sd > 255ull ? 255u : (uint32_t)sd;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_compose_kernel(const long long* __restrict__ cells,
                                                                    const ClipGeom g, uint8_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const int t = (int)(blockIdx.x / (unsigned)g.Hs), y = (int)(blockIdx.x - (unsigned)t * (unsigned)g.Hs);
    // the line's cell row (uniform over the workgroup)
    const int ry = y - g.gutter, pitch_y = g.Hc + g.gutter;
    const long long* row = nullptr;
    int cy = 0;
    if (ry >= 0) {
        const int r = ry / pitch_y;
        cy = ry - r * pitch_y;
        if (r < g.R && cy < g.Hc) row = cells + 8L * r * g.N;
    }
    uint8_t* line = out + (long)blockIdx.x * g.line;
    int head = (int)((4u - (unsigned)((uintptr_t)line & 3u)) & 3u);   // bytes in front of the first aligned dword
    if (head > g.line) head = g.line;
    const int nd = (g.line - head) >> 2;                                // aligned dwords of the line
    const int tail0 = head + 4 * nd;                                    // first byte behind them
    // ragged ends: at most 3 + 3 single bytes, one lane each
    if (tid < head) line[tid] = (uint8_t)clip_byte(tid, g, row, cy, t);
    else if (tid >= 4 && tid - 4 < g.line - tail0)
        line[tail0 + tid - 4] = (uint8_t)clip_byte(tail0 + tid - 4, g, row, cy, t);
    uint32_t* words = reinterpret_cast<uint32_t*>(line + head);
    for (int w = tid; w < nd; w += CLIP_THREADS) {
        const int xb = head + 4 * w;
        const uint32_t b0 = clip_byte(xb, g, row, cy, t);
        const uint32_t b1 = clip_byte(xb + 1, g, row, cy, t);
        const uint32_t b2 = clip_byte(xb + 2, g, row, cy, t);
        const uint32_t b3 = clip_byte(xb + 3, g, row, cy, t);
        words[w] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
}

}  // namespace

extern "C" int rfn_clip_max_group(void) { return RFN_CLIP_MAX_GROUP; }
extern "C" int rfn_clip_max_gain(void) { return RFN_CLIP_MAX_GAIN; }

extern "C" int rfn_clip_compose_u8(const void* cells, int R, int N, int T, int C, int H, int W, int zoom, int border,
                                   int gutter, int bg, int n_bits, int range_half, int lead, long out_addr,
                                   rfn_stream_t stream) {
    RFN_CHECK_ARG(R >= 1 && N >= 1 && T >= 1 && H >= 1 && W >= 1, -1);
    RFN_CHECK_ARG(C == 1 || C == 3, -2);
    RFN_CHECK_ARG(zoom >= 1 && zoom <= 16 && border >= 0 && border <= 64 && gutter >= 0 && bg >= 0 && bg <= 255, -3);
    RFN_CHECK_ARG(n_bits >= 1 && n_bits <= 8 && (lead == 0 || lead == 1), -4);
    const long Hc = (long)zoom * H + 2L * border, Wc = (long)zoom * W + 2L * border;
    RFN_CHECK_ARG(Hc <= 0x7fffffffL / R && Wc <= 0x7fffffffL / N && gutter <= 0x7fffffffL / ((long)(R > N ? R : N) + 1), -5);
    const long Hs = (long)R * Hc + ((long)R + 1) * gutter, Ws = (long)N * Wc + ((long)N + 1) * gutter;
    RFN_CHECK_ARG(Ws <= 0x7fffffffL / 3 && 3 * Ws + lead <= 0x7fffffffL && Hs <= 0x7fffffffL / T, -5);
    RFN_CHECK_ARG(cells && out_addr, -6);
    ClipGeom g;
    g.R = R, g.N = N, g.C = C, g.H = H, g.W = W, g.zoom = zoom, g.border = border, g.gutter = gutter, g.bg = bg;
    g.lead = lead, g.range_half = range_half != 0;
    g.Hc = (int)Hc, g.Wc = (int)Wc, g.Hs = (int)Hs;
    g.line = (int)(3 * Ws + lead);
    g.n_bins = (float)(1 << n_bits);
    g.scale = 256.f / g.n_bins;
    hipLaunchKernelGGL(clip_compose_kernel, dim3((unsigned)((long)T * Hs)), dim3(CLIP_THREADS), 0, (hipStream_t)stream,
                       static_cast<const long long*>(cells), g, reinterpret_cast<uint8_t*>(out_addr));
    RFN_LAUNCH_CHECK();
    return 0;
}
