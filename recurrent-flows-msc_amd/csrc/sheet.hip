// A sheet of frames as 8-bit RGB pixels, composed on the device in one launch: the picture the reference's plotter()
// (RFN/trainer.py:325-417) and Evaluator.plot_samples (evaluation_metrics/error_metrics.py:128-152) lay out with
// matplotlib subplots, without text, axes or titles.
//
//   sheet : R rows x N columns of H x W cells, `gutter` background pixels between cells and around the sheet:
//           Hs = R*H + (R+1)*gutter,  Ws = N*W + (N+1)*gutter;  cell (r, i) has its top-left corner at
//           (gutter + r*(H+gutter), gutter + i*(W+gutter)).
//   row r : rfn_sheet_row {ptr, step, kind, count}: the frame of cell (r, i) is the dense [C, H, W] block at
//           ptr + i*step (elements) for i < count; the cells i >= count are background.  kind 0: fp32 in model space,
//           kind 1: uint8.  C = 1 puts the one value into R, G and B.
//   out   : lead = 0: uint8 [Hs, Ws, 3];  lead = 1: uint8 [Hs, 1 + 3*Ws], byte 0 of every line being 0 (the PNG filter
//           type "None"): the buffer is a PNG's raw stream before deflate.
//
// Pixel rule of kind 0 = Solver.preprocess(x, reverse=True) (RFN/trainer.py:165-188 of the reference):
//   v = x + 0.5 (range_half) or x;  v = v * 2^n_bits;  q = floor(v) * (256 / 2^n_bits);  byte = clamp(q, 0, 255), NaN -> 0,
// every operation rounded to fp32 on its own.  All factors are powers of two, so the products are exact and the result
// equals torch's on any device bit for bit.
//
// One workgroup per output line.  The line's cell row, the row's descriptor and the y inside the cell are the same for
// the whole workgroup (scalar registers); a lane owns one 4-byte-aligned dword of the line at a time, builds its four
// bytes and stores them with one dword store.  Lines of 1 + 3*Ws bytes start at any byte address: the up to 3 bytes in
// front of the first aligned dword and the up to 3 behind the last one are stored as bytes by the first lanes.  Every
// byte of `out` is written exactly once (background and lead bytes included: nothing is zeroed first), nothing outside
// it is touched, and only the listed frames are read.  No atomics, no LDS, no scratch.
#include "common.h"
#include "pixel_quant.h"
#include "../../include/rfn_hip.h"

static_assert(sizeof(rfn_sheet_row) == 24, "rfn_sheet_row layout is part of the ABI");

namespace {

constexpr int SHEET_THREADS = 256;

struct SheetRows {
    rfn_sheet_row row[RFN_SHEET_MAX_ROWS];
};

struct SheetGeom {
    int R, N, C, H, W, gutter, bg, lead, range_half;
    int line;        // bytes of one output line: lead + 3*Ws
    float n_bins;    // 2^n_bits
    float scale;     // 256 / 2^n_bits
};

__device__ __forceinline__ uint32_t sheet_quantise(float x, const SheetGeom& g) {
    return rfn_quantise_u8(x, g.range_half, g.n_bins, g.scale);   // (shared with clip_compose.hip)
}

// byte `xb` of the current line; src = channel 0 of the line's pixel row in column 0's frame (nullptr: a gutter line)
__device__ __forceinline__ uint32_t sheet_byte(int xb, const SheetGeom& g, const void* src, int kind, long step,
                                               int count, int plane) {
    xb -= g.lead;
    if (xb < 0) return 0u;                      // the filter-type byte of a scanline
    const int px = xb / 3, ch = xb - 3 * px;
    const int cx = px - g.gutter;
    if (src == nullptr || cx < 0) return (uint32_t)g.bg;
    const int pitch = g.W + g.gutter;
    const int i = cx / pitch, xx = cx - i * pitch;
    if (xx >= g.W || i >= count) return (uint32_t)g.bg;
    const long e = (long)i * step + (g.C == 3 ? (long)ch * plane : 0L) + xx;
    if (kind == 1) return (uint32_t)static_cast<const uint8_t*>(src)[e];
    return sheet_quantise(static_cast<const float*>(src)[e], g);
}

__global__ __launch_bounds__(SHEET_THREADS) void sheet_compose_kernel(const SheetRows rows, const SheetGeom g,
                                                                      uint8_t* __restrict__ out) {
    const int y = (int)blockIdx.x;
    const int tid = threadIdx.x;
    // the line's cell row (uniform over the workgroup)
    const int ry = y - g.gutter, pitch_y = g.H + g.gutter;
    const void* src = nullptr;
    int kind = 0, count = 0;
    long step = 0;
    const int plane = g.H * g.W;
    if (ry >= 0) {
        const int r = ry / pitch_y, yy = ry - r * pitch_y;
        if (r < g.R && yy < g.H) {
            const rfn_sheet_row d = rows.row[r];
            kind = d.kind;
            count = d.count;
            step = d.step;
            if (count > 0)
                src = kind == 1 ? static_cast<const void*>(static_cast<const uint8_t*>(d.ptr) + (long)yy * g.W)
                                : static_cast<const void*>(static_cast<const float*>(d.ptr) + (long)yy * g.W);
        }
    }
    uint8_t* line = out + (long)y * g.line;
    int head = (int)((4u - (unsigned)((uintptr_t)line & 3u)) & 3u);   // bytes in front of the first aligned dword
    if (head > g.line) head = g.line;
    const int nd = (g.line - head) >> 2;                                // aligned dwords of the line
    const int tail0 = head + 4 * nd;                                    // first byte behind them
    // ragged ends: at most 3 + 3 single bytes, one lane each
    if (tid < head) line[tid] = (uint8_t)sheet_byte(tid, g, src, kind, step, count, plane);
    else if (tid >= 4 && tid - 4 < g.line - tail0)
        line[tail0 + tid - 4] = (uint8_t)sheet_byte(tail0 + tid - 4, g, src, kind, step, count, plane);
    uint32_t* words = reinterpret_cast<uint32_t*>(line + head);
    for (int w = tid; w < nd; w += SHEET_THREADS) {
        const int xb = head + 4 * w;
        const uint32_t b0 = sheet_byte(xb, g, src, kind, step, count, plane);
        const uint32_t b1 = sheet_byte(xb + 1, g, src, kind, step, count, plane);
        const uint32_t b2 = sheet_byte(xb + 2, g, src, kind, step, count, plane);
        const uint32_t b3 = sheet_byte(xb + 3, g, src, kind, step, count, plane);
        words[w] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
}

}  // namespace

extern "C" int rfn_sheet_max_rows(void) { return RFN_SHEET_MAX_ROWS; }

extern "C" int rfn_sheet_compose_u8(const void* rows_table, int R, int N, int C, int H, int W, int gutter, int bg,
                                    int n_bits, int range_half, int lead, long out_addr, rfn_stream_t stream) {
    RFN_CHECK_ARG(R >= 1 && R <= RFN_SHEET_MAX_ROWS && N >= 1 && H >= 1 && W >= 1, -1);
    RFN_CHECK_ARG(C == 1 || C == 3, -2);
    RFN_CHECK_ARG(gutter >= 0 && bg >= 0 && bg <= 255, -3);
    RFN_CHECK_ARG(n_bits >= 1 && n_bits <= 8 && (lead == 0 || lead == 1), -4);
    const long Hs = (long)R * H + ((long)R + 1) * gutter, Ws = (long)N * W + ((long)N + 1) * gutter;
    RFN_CHECK_ARG(Hs <= 0x7fffffffL && 3 * Ws + lead <= 0x7fffffffL && (long)C * H * W <= 0x7fffffffL, -5);
    RFN_CHECK_ARG(rows_table && out_addr, -6);
    SheetRows rows;
    memset(&rows, 0, sizeof(rows));
    const rfn_sheet_row* tab = static_cast<const rfn_sheet_row*>(rows_table);
    for (int r = 0; r < R; ++r) {
        RFN_CHECK_ARG(tab[r].kind == 0 || tab[r].kind == 1, -7);
        RFN_CHECK_ARG(tab[r].count >= 0 && tab[r].count <= N, -8);
        RFN_CHECK_ARG(tab[r].count == 0 || tab[r].ptr, -9);
        RFN_CHECK_ARG(tab[r].kind == 1 || ((uintptr_t)tab[r].ptr & 3) == 0, -10);
        rows.row[r] = tab[r];
    }
    SheetGeom g;
    g.R = R, g.N = N, g.C = C, g.H = H, g.W = W, g.gutter = gutter, g.bg = bg, g.lead = lead;
    g.range_half = range_half != 0;
    g.line = (int)(3 * Ws + lead);
    g.n_bins = (float)(1 << n_bits);
    g.scale = 256.f / g.n_bins;
    hipLaunchKernelGGL(sheet_compose_kernel, dim3((unsigned)Hs), dim3(SHEET_THREADS), 0, (hipStream_t)stream, rows, g,
                       reinterpret_cast<uint8_t*>(out_addr));
    RFN_LAUNCH_CHECK();
    return 0;
}
