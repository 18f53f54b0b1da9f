// A line chart as 8-bit RGB pixels, rendered on the device in one launch from a display list: the figures the
// reference draws with matplotlib in Evaluator.plot_eval_values and .test_temp_values (evaluation_metrics/
// error_metrics.py:600-1003) -- lines, translucent bands, markers, dashed lines, grids, frames and text.
// DESIGN.md section 25 is the pixel contract; tests/chart_ref.py restates it in int64 numpy.
//
//   table : n records of 12 int32 {type, rgba, p0 .. p9}, painted in list order.  rgba = r | g<<8 | b<<16 | alpha<<24.
//           Geometry is in 1/16 pixel, x to the right, y down; every coordinate lies in [-4096, 36864] (the largest
//           canvas and 256 pixels around it), every length (capsule half-width) in [0, 4096]: with those bounds each
//           product below fits 64 bits (|d x p| <= 2 * 40960 * 36864 < 2^31.5).
//             0 BOX        p0..p3 = x0, y0, x1, y1: x0 <= sx < x1 and y0 <= sy < y1;  p4, p5 = dash on / off lengths:
//                          with on + off > 0 also ((s - start) mod (on + off)) < on, s the sample's coordinate along the
//                          long axis (x if x1 - x0 >= y1 - y0, else y) and start that axis' x0 / y0
//             1 CAPSULE    p0..p3 = ax, ay, bx, by, p4 = hw;  d = b - a, p = s - a:
//                          p.d <= 0: |p|^2 <= hw^2;  p.d >= |d|^2: |s - b|^2 <= hw^2;  else (d x p)^2 <= hw^2 |d|^2
//             2 TRAPEZOID  p0..p5 = x0, x1, lo0, lo1, hi0, hi1:  x0 <= sx < x1,
//                          (sy - lo0)(x1 - x0) >= (lo1 - lo0)(sx - x0),  (sy - hi0)(x1 - x0) < (hi1 - hi0)(sx - x0)
//             3 TRIANGLE   p0..p5 = x0, y0, x1, y1, x2, y2:  e_i = (x_j - x_i)(sy - y_i) - (y_j - y_i)(sx - x_i) for the
//                          edges (0,1), (1,2), (2,0); inside iff all e_i >= 0 or all e_i <= 0; a triangle of zero
//                          area, (x1 - x0)(y2 - y0) == (y1 - y0)(x2 - x0), paints nothing
//             4 GLYPH      p0, p1 = x, y of the top-left corner, p2 = character (32..126), p3 = scale k >= 1 (pixels per
//                          dot), p4 = 0 upright / 1 rotated by 90 degrees counter-clockwise.  u = sx - x, v = sy - y,
//                          q = 16 k.  Upright: 0 <= u < 5q, 0 <= v < 7q, dot (floor(u/q), floor(v/q)).  Rotated:
//                          0 <= u < 7q, 0 <= v < 5q, dot (4 - floor(v/q), floor(u/q)).  Inside iff the dot is set.
//           Any other type, a character outside 32..126 and a scale outside 1..128 paint nothing.
//   pixel : the samples of pixel (px, py) are (16 px + i, 16 py + j), i, j in {2, 6, 10, 14};  c = number of samples
//           inside (0..16), w = alpha * c,  dst = (dst * (4080 - w) + src * w + 2040) / 4080 per channel in integers,
//           starting from the background colour.
//   out   : lead = 0: uint8 [H, W, 3];  lead = 1: uint8 [H, 1 + 3 W], byte 0 of every line being 0 (PNG filter "None").
//
// One workgroup of 256 lanes owns a 16 x 16 pixel tile, one lane a pixel.  The list is walked in chunks of 256
// records: lane t takes record t of the chunk, bounds it (conservatively) and tests the bounds against the tile; the
// survivors are packed into LDS in list order by wave ballots and the four waves' counts (no atomics); every lane then
// shades its pixel over the survivors, keeping r, g, b in registers into the next chunk.  A primitive that covers no
// sample leaves the pixel as it is (w = 0 is the identity), so the culling, and with it the chunk size, cannot change a
// byte.  A glyph's 35 dots are packed into its survivor record while culling (one read of the font per glyph and
// tile).  Every byte of `out` is written exactly once, by byte stores: three per pixel and the lead byte by the lanes of
// column 0.  12 KiB of LDS, no atomics, no scratch; whatever the table holds, nothing outside `out` is written and
// nothing outside the table is read.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int CHART_TILE = 16;                         // pixels per tile side
constexpr int CHART_THREADS = CHART_TILE * CHART_TILE;  // lanes of a workgroup = records of a chunk
constexpr int CHART_REC = 12;                          // int32 per record
constexpr int CHART_MAX_SIDE = 2048;
constexpr int CHART_MAX_SCALE = 128;                   // pixels per glyph dot
constexpr int CHART_FONT_FIRST = 32, CHART_FONT_COUNT = 95;

enum { CHART_BOX = 0, CHART_CAPSULE = 1, CHART_TRAPEZOID = 2, CHART_TRIANGLE = 3, CHART_GLYPH = 4 };

const uint8_t CHART_FONT[CHART_FONT_COUNT][5] = {
#include "chart_font.inc"
};
__constant__ uint8_t d_chart_font[CHART_FONT_COUNT][5] = {
#include "chart_font.inc"
};

struct ChartRec {
    int type, rgba, p[10];
};

// The bounds and the inside-tests are plain integer C++, compiled for the host as well: a stand-alone CPU program that
// includes this file can run them under a host sanitizer.
// conservative bounds [x0, x1) x [y0, y1) of a record in 1/16 pixel; false: it paints nothing anywhere
__host__ __device__ __forceinline__ bool chart_bounds(const ChartRec& r, long& x0, long& y0, long& x1, long& y1) {
    const int* p = r.p;
    switch (r.type) {
    case CHART_BOX:
        x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3];
        return true;
    case CHART_CAPSULE:
        x0 = (long)min(p[0], p[2]) - p[4], x1 = (long)max(p[0], p[2]) + p[4] + 1;
        y0 = (long)min(p[1], p[3]) - p[4], y1 = (long)max(p[1], p[3]) + p[4] + 1;
        return p[4] >= 0;
    case CHART_TRAPEZOID:
        x0 = p[0], x1 = p[1], y0 = min(p[2], p[3]), y1 = max(p[4], p[5]);
        return true;
    case CHART_TRIANGLE:
        x0 = min(p[0], min(p[2], p[4])), x1 = (long)max(p[0], max(p[2], p[4])) + 1;
        y0 = min(p[1], min(p[3], p[5])), y1 = (long)max(p[1], max(p[3], p[5])) + 1;
        // zero area: the three edge functions vanish together on a whole line; such a record paints nothing
        return ((long)p[2] - p[0]) * ((long)p[5] - p[1]) != ((long)p[3] - p[1]) * ((long)p[4] - p[0]);
    case CHART_GLYPH: {
        if (p[2] < CHART_FONT_FIRST || p[2] >= CHART_FONT_FIRST + CHART_FONT_COUNT || p[3] < 1 || p[3] > CHART_MAX_SCALE)
            return false;
        const long q = 16L * p[3];
        x0 = p[0], y0 = p[1], x1 = x0 + (p[4] ? 7 : 5) * q, y1 = y0 + (p[4] ? 5 : 7) * q;
        return true;
    }
    default:
        return false;
    }
}

// samples of the four at X + {2, 6, 10, 14} that lie in [lo, hi) and, with a dash period, on a dash
__host__ __device__ __forceinline__ int chart_box_axis(int X, int lo, int hi, int on, int period) {
    int n = 0;
#pragma unroll
    for (int k = 2; k < 16; k += 4) {
        const int s = X + k;
        bool in = s >= lo && s < hi;
        if (in && period > 0) in = (int)(((unsigned)s - (unsigned)lo) % (unsigned)period) < on;
        n += in ? 1 : 0;
    }
    return n;
}

// number of the pixel's 16 samples inside the record; X, Y = 16 * (px, py)
__host__ __device__ __forceinline__ int chart_coverage(int type, const int (&p)[10], int X, int Y) {
    int c = 0;
    if (type == CHART_BOX) {
        // the test is a product of one in x and one in y (the dash follows one axis), and so is the count
        const long period = (long)p[4] + (long)p[5];
        const bool dashed = period > 0 && period <= 0x7fffffffL && p[4] >= 0;
        const bool along_x = (long)p[2] - p[0] >= (long)p[3] - p[1];
        const int per = dashed ? (int)period : 0;
        return chart_box_axis(X, p[0], p[2], p[4], along_x ? per : 0) *
               chart_box_axis(Y, p[1], p[3], p[4], along_x ? 0 : per);
    }
    if (type == CHART_CAPSULE) {
        const long dx = (long)p[2] - p[0], dy = (long)p[3] - p[1];
        const long dd = dx * dx + dy * dy, hh = (long)p[4] * p[4];
#pragma unroll
        for (int j = 2; j < 16; j += 4)
#pragma unroll
            for (int i = 2; i < 16; i += 4) {
                const long px = (long)(X + i) - p[0], py = (long)(Y + j) - p[1];
                const long t = px * dx + py * dy;
                bool in;
                if (t <= 0) in = px * px + py * py <= hh;
                else if (t >= dd) {
                    const long qx = (long)(X + i) - p[2], qy = (long)(Y + j) - p[3];
                    in = qx * qx + qy * qy <= hh;
                } else {
                    const long cr = dx * py - dy * px;
                    in = cr * cr <= hh * dd;
                }
                c += in ? 1 : 0;
            }
        return c;
    }
    if (type == CHART_TRAPEZOID) {
        const long w = (long)p[1] - p[0], dlo = (long)p[3] - p[2], dhi = (long)p[5] - p[4];
#pragma unroll
        for (int i = 2; i < 16; i += 4) {
            const int sx = X + i;
            if (sx < p[0] || sx >= p[1]) continue;
            const long u = (long)sx - p[0];
#pragma unroll
            for (int j = 2; j < 16; j += 4) {
                const long sy = Y + j;
                c += ((sy - p[2]) * w >= dlo * u && (sy - p[4]) * w < dhi * u) ? 1 : 0;
            }
        }
        return c;
    }
    if (type == CHART_TRIANGLE) {
        const long ax = (long)p[2] - p[0], ay = (long)p[3] - p[1];
        const long bx = (long)p[4] - p[2], by = (long)p[5] - p[3];
        const long cx = (long)p[0] - p[4], cy = (long)p[1] - p[5];
#pragma unroll
        for (int j = 2; j < 16; j += 4)
#pragma unroll
            for (int i = 2; i < 16; i += 4) {
                const long sx = X + i, sy = Y + j;
                const long e0 = ax * (sy - p[1]) - ay * (sx - p[0]);
                const long e1 = bx * (sy - p[3]) - by * (sx - p[2]);
                const long e2 = cx * (sy - p[5]) - cy * (sx - p[4]);
                c += ((e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0)) ? 1 : 0;
            }
        return c;
    }
    if (type == CHART_GLYPH) {
        // p[5], p[6]: the character's 35 dots, bit c*7 + r (packed while culling); 1 <= p[3] <= 128 was checked there
        const unsigned long long dots = (unsigned long long)(unsigned)p[5] | ((unsigned long long)(unsigned)p[6] << 32);
        const int q = 16 * p[3];   // <= 2048
        const int nu = (p[4] ? 7 : 5) * q, nv = (p[4] ? 5 : 7) * q;
#pragma unroll
        for (int j = 2; j < 16; j += 4)
#pragma unroll
            for (int i = 2; i < 16; i += 4) {
                const long u = (long)(X + i) - p[0], v = (long)(Y + j) - p[1];
                if (u < 0 || v < 0 || u >= nu || v >= nv) continue;
                const int a = (int)u / q, b = (int)v / q;
                const int col = p[4] ? 4 - b : a, row = p[4] ? a : b;
                c += (int)((dots >> (col * 7 + row)) & 1ull);
            }
        return c;
    }
    return 0;
}

__global__ __launch_bounds__(CHART_THREADS) void chart_render_kernel(const int* __restrict__ table, int n, int H, int W,
                                                                     int bg, int lead, uint8_t* __restrict__ out) {
    __shared__ int s_rec[CHART_REC][CHART_THREADS];   // survivors of the chunk, field-major: stores without conflicts,
                                                      // the shading loop's loads are broadcasts
    __shared__ int s_cnt[CHART_THREADS / RFN_WAVE];
    const int tid = threadIdx.x, lane = tid & (RFN_WAVE - 1), wave = tid / RFN_WAVE;
    const int px = (int)blockIdx.x * CHART_TILE + (tid & (CHART_TILE - 1));
    const int py = (int)blockIdx.y * CHART_TILE + tid / CHART_TILE;
    const int X = 16 * px, Y = 16 * py;
    // the tile in 1/16 pixel
    const long tx0 = 16L * CHART_TILE * blockIdx.x, ty0 = 16L * CHART_TILE * blockIdx.y;
    const long tx1 = tx0 + 16L * CHART_TILE, ty1 = ty0 + 16L * CHART_TILE;
    int cr = bg & 255, cg = (bg >> 8) & 255, cb = (bg >> 16) & 255;

    for (int base = 0; base < n; base += CHART_THREADS) {
        // ---- cull: lane t bounds record base + t
        ChartRec r;
        bool keep = false;
        if (base + tid < n) {
            const int4* src = reinterpret_cast<const int4*>(table + (long)(base + tid) * CHART_REC);   // 48-byte records
            const int4 a = src[0], b = src[1], c = src[2];
            r.type = a.x, r.rgba = a.y;
            r.p[0] = a.z, r.p[1] = a.w, r.p[2] = b.x, r.p[3] = b.y, r.p[4] = b.z, r.p[5] = b.w;
            r.p[6] = c.x, r.p[7] = c.y, r.p[8] = c.z, r.p[9] = c.w;
            long x0, y0, x1, y1;
            keep = ((unsigned)r.rgba >> 24) != 0 && chart_bounds(r, x0, y0, x1, y1) && x1 > tx0 && x0 < tx1 &&
                   y1 > ty0 && y0 < ty1;
            if (keep && r.type == CHART_GLYPH) {
                const uint8_t* col = d_chart_font[r.p[2] - CHART_FONT_FIRST];
                unsigned long long dots = 0;
#pragma unroll
                for (int k = 0; k < 5; ++k) dots |= (unsigned long long)(col[k] & 0x7f) << (7 * k);
                r.p[5] = (int)(unsigned)(dots & 0xffffffffull), r.p[6] = (int)(unsigned)(dots >> 32);
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(kept);
        __syncthreads();
        int slot = __popcll(kept & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < CHART_THREADS / RFN_WAVE; ++w) {
            const int cw = s_cnt[w];
            slot += w < wave ? cw : 0;
            total += cw;
        }
        if (keep) {
            s_rec[0][slot] = r.type, s_rec[1][slot] = r.rgba;
#pragma unroll
            for (int k = 0; k < 10; ++k) s_rec[2 + k][slot] = r.p[k];
        }
        __syncthreads();
        // ---- shade: every lane its pixel, over the survivors in list order
        if (px < W && py < H) {
            for (int i = 0; i < total; ++i) {
                const int type = __builtin_amdgcn_readfirstlane(s_rec[0][i]);
                const int rgba = s_rec[1][i];
                int p[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) p[k] = s_rec[2 + k][i];
                const int c = chart_coverage(type, p, X, Y);
                if (c) {
                    const int w = (int)((unsigned)rgba >> 24) * c;
                    cr = (cr * (4080 - w) + (rgba & 255) * w + 2040) / 4080;
                    cg = (cg * (4080 - w) + ((rgba >> 8) & 255) * w + 2040) / 4080;
                    cb = (cb * (4080 - w) + ((rgba >> 16) & 255) * w + 2040) / 4080;
                }
            }
        }
        __syncthreads();   // the next chunk overwrites s_rec and s_cnt
    }
    if (px < W && py < H) {
        uint8_t* line = out + (long)py * (lead + 3L * W);
        if (lead && px == 0) line[0] = 0;
        uint8_t* dst = line + lead + 3L * px;
        dst[0] = (uint8_t)cr, dst[1] = (uint8_t)cg, dst[2] = (uint8_t)cb;
    }
}

}  // namespace

extern "C" int rfn_chart_chunk(void) { return CHART_THREADS; }

extern "C" int rfn_chart_font(long long* out) {
    RFN_CHECK_ARG(out != nullptr, -1);
    for (int ch = 0; ch < CHART_FONT_COUNT; ++ch)
        for (int k = 0; k < 5; ++k) out[5 * ch + k] = CHART_FONT[ch][k];
    return 0;
}

extern "C" int rfn_chart_render_u8(const int* table, int n, int H, int W, int bg, int lead, long out_addr,
                                   rfn_stream_t stream) {
    RFN_CHECK_ARG(H >= 1 && H <= CHART_MAX_SIDE && W >= 1 && W <= CHART_MAX_SIDE, -1);
    RFN_CHECK_ARG(n >= 0 && (n == 0 || table), -2);
    RFN_CHECK_ARG(n == 0 || ((uintptr_t)table & 15) == 0, -3);
    RFN_CHECK_ARG(bg >= 0 && bg <= 0xffffff && (lead == 0 || lead == 1), -4);
    RFN_CHECK_ARG(out_addr, -5);
    const dim3 grid((unsigned)ceil_div(W, CHART_TILE), (unsigned)ceil_div(H, CHART_TILE));
    hipLaunchKernelGGL(chart_render_kernel, grid, dim3(CHART_THREADS), 0, (hipStream_t)stream, table, n, H, W, bg, lead,
                       reinterpret_cast<uint8_t*>(out_addr));
    RFN_LAUNCH_CHECK();
    return 0;
}
