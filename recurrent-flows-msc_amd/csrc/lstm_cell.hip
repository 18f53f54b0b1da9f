// One torch.nn.LSTMCell call (SVG/SVG.py:131,149 and :163,185 of the reference: the frame predictor, the posterior and
// the prior, each `Linear -> LSTMCell(h, h)` per layer) as one kernel each way.  Layout and gate order of nn.LSTMCell:
// w_ih [4H, I], w_hh [4H, H], rows gH .. gH+H-1 belong to gate g, g = 0..3 = i, f, g, o.
//
// Forward: a workgroup of four waves owns a 16-row x 16-unit tile of the output and every wave keeps the four
// accumulators of that tile, one per gate, on the float32-input MFMA 16x16x4 (exact float32 products, one k-ordered fma
// chain per output).  The k range is cut into chunks of 16: first those of x . w_ih, then those of h . w_hh; wave w takes
// the chunks w, w + 4, ...  A lane reads 16 bytes along k of its row of the activations and of its row of each gate's
// weights (lane l: row l & 15, k = 4 (l >> 4) .. + 3 of the chunk); MFMA s of a chunk takes element s, so the k order
// inside a chunk is permuted the same way for both operands.  The three partial tiles of waves 1..3 go through LDS and
// wave 0 adds them in wave order, then b_ih, then b_hh.  The lane that holds pre_i[b, j] holds pre_f, pre_g and pre_o of
// the same (b, j): the pointwise part is lane-local and the pre-activations never reach memory.  The order of summation
// of an output depends on I and H alone, not on B or on where the tile lies; tails are zero-filled (exact) and masked.
//
// Backward: the pointwise part and the bias gradient.  A workgroup owns 16 units over ALL rows: thread (unit t & 15, row
// group t >> 4) walks the rows rg, rg + 16, ... in order, the 16 row-group sums are added in row-group order through
// LDS.  No atomics, nothing waits on another workgroup.
#include "common.h"
#include "../../include/rfn_hip.h"

typedef float lc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RFN_LC_TILE = 16;   // rows and units of a tile (the MFMA's M and N)
constexpr int RFN_LC_KC = 16;     // k values of a chunk: 4 MFMAs of k = 4
constexpr int RFN_LC_WAVES = 4;   // waves of a workgroup: the k chunks are dealt round robin

// 16 bytes along k of one row, zero outside the row range and past K.  VEC: K % 4 == 0 and the base is 16-byte aligned,
// so the four values are inside or outside together.
template <bool VEC>
__device__ __forceinline__ lc_f32x4 lc_load4(const float* __restrict__ p, bool row_ok, long row_off, int k, int K) {
    lc_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if (VEC) {
        if (k < K) v = *reinterpret_cast<const lc_f32x4*>(p + row_off + k);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) v[e] = p[row_off + k + e];
    }
    return v;
}

// the chunks ch, ch + RFN_LC_WAVES, ... < n_chunks of act [rows, K] . w[4H, K]^T into acc; returns the first chunk index
// not taken (>= n_chunks)
template <bool VEC>
__device__ __forceinline__ int lc_accumulate(lc_f32x4 (&acc)[4], const float* __restrict__ act,
                                             const float* __restrict__ w, int K, int H, int ch, int n_chunks, bool a_ok,
                                             long a_row, bool u_ok, long u, int kq) {
    for (; ch < n_chunks; ch += RFN_LC_WAVES) {
        const int k = ch * RFN_LC_KC + 4 * kq;
        const lc_f32x4 a = lc_load4<VEC>(act, a_ok, a_row * K, k, K);
        lc_f32x4 b[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = lc_load4<VEC>(w, u_ok, ((long)g * H + u) * K, k, K);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[g][s], acc[g], 0, 0, 0);
    }
    return ch;
}

__device__ __forceinline__ float lc_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <bool VX, bool VH>
__global__ void __launch_bounds__(64 * RFN_LC_WAVES)
lstm_cell_fwd_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ c,
                     const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                     const float* __restrict__ b_hh, float* __restrict__ h_out, float* __restrict__ c_out,
                     float* __restrict__ gates, int B, int I, int H) {
    __shared__ float part[RFN_LC_WAVES - 1][16][64];   // [wave - 1][gate * 4 + reg][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    // a one-dimensional grid of tiles, the unit tiles of a row tile side by side
    const unsigned tiles_h = (unsigned)((H + RFN_LC_TILE - 1) / RFN_LC_TILE);
    const long b0 = (long)(blockIdx.x / tiles_h) * RFN_LC_TILE, j0 = (long)(blockIdx.x % tiles_h) * RFN_LC_TILE;
    const long a_row = b0 + r, u = j0 + r;   // this lane's operand rows: of the activations, of each gate's weights
    const bool a_ok = a_row < B, u_ok = u < H;
    lc_f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = lc_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nx = (I + RFN_LC_KC - 1) / RFN_LC_KC, nh = (H + RFN_LC_KC - 1) / RFN_LC_KC;
    int ch = lc_accumulate<VX>(acc, x, w_ih, I, H, wave, nx, a_ok, a_row, u_ok, u, kq);
    lc_accumulate<VH>(acc, h, w_hh, H, H, ch - nx, nh, a_ok, a_row, u_ok, u, kq);
    if (wave > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) part[wave - 1][g * 4 + q][lane] = acc[g][q];
    }
    __syncthreads();
    if (wave > 0) return;
    // C/D map of the 16x16 forms: column (unit) = lane & 15, row = 4 (lane >> 4) + reg
    const long j = j0 + r;
    if (j >= H) return;
    float bias[4], bias2[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = b_ih[(long)g * H + j], bias2[g] = b_hh[(long)g * H + j];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long b = b0 + 4 * kq + q;
        if (b >= B) continue;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v = acc[g][q];
#pragma unroll
            for (int w = 0; w < RFN_LC_WAVES - 1; ++w) v += part[w][g * 4 + q][lane];
            pre[g] = (v + bias[g]) + bias2[g];
        }
        const float ig = lc_sigmoid(pre[0]), fg = lc_sigmoid(pre[1]), gg = tanhf(pre[2]), og = lc_sigmoid(pre[3]);
        const long e = b * H + j, ge = b * 4 * H + j;
        const float cn = fg * c[e] + ig * gg;
        c_out[e] = cn;
        h_out[e] = og * tanhf(cn);
        gates[ge] = ig;
        gates[ge + H] = fg;
        gates[ge + 2L * H] = gg;
        gates[ge + 3L * H] = og;
    }
}

constexpr int RFN_LC_BW_UNITS = 16, RFN_LC_BW_GROUPS = 16;   // backward: units x row groups of a workgroup (256 threads)

__global__ void __launch_bounds__(RFN_LC_BW_UNITS * RFN_LC_BW_GROUPS)
lstm_cell_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ gc, const float* __restrict__ gates,
                     const float* __restrict__ c, const float* __restrict__ c_out, float* __restrict__ D,
                     float* __restrict__ g_c, float* __restrict__ g_bias, int B, int H) {
    __shared__ float sm[4][RFN_LC_BW_GROUPS][RFN_LC_BW_UNITS];
    const int jc = threadIdx.x & (RFN_LC_BW_UNITS - 1), rg = threadIdx.x / RFN_LC_BW_UNITS;
    const long j = (long)blockIdx.x * RFN_LC_BW_UNITS + jc;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < H) {
        for (long b = rg; b < B; b += RFN_LC_BW_GROUPS) {
            const long e = b * H + j, ge = b * 4 * H + j;
            const float ig = gates[ge], fg = gates[ge + H], gg = gates[ge + 2L * H], og = gates[ge + 3L * H];
            const float ghv = gh ? gh[e] : 0.f, gcv = gc ? gc[e] : 0.f;
            const float t = tanhf(c_out[e]);
            const float gct = gcv + ghv * og * (1.f - t * t);
            const float d_i = gct * gg * ig * (1.f - ig);
            const float d_f = gct * c[e] * fg * (1.f - fg);
            const float d_g = gct * ig * (1.f - gg * gg);
            const float d_o = ghv * t * og * (1.f - og);
            D[ge] = d_i;
            D[ge + H] = d_f;
            D[ge + 2L * H] = d_g;
            D[ge + 3L * H] = d_o;
            g_c[e] = gct * fg;
            s[0] += d_i;
            s[1] += d_f;
            s[2] += d_g;
            s[3] += d_o;
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) sm[g][rg][jc] = s[g];
    __syncthreads();
    if (rg < 4 && j < H) {   // row group g of the first four finishes gate g
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < RFN_LC_BW_GROUPS; ++q) v += sm[rg][q][jc];
        g_bias[(long)rg * H + j] = v;
    }
}

static inline bool lc_vec_ok(const void* a, const void* w, int K) {
    return K % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)w % 16) == 0;
}

extern "C" int rfn_lstm_cell_fwd_f32(const float* x, const float* h, const float* c, const float* w_ih, const float* w_hh,
                                     const float* b_ih, const float* b_hh, float* h_out, float* c_out, float* gates,
                                     int B, int I, int H, rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 1 && I >= 1 && H >= 1, -1);
    const long tiles = (long)ceil_div(B, RFN_LC_TILE) * ceil_div(H, RFN_LC_TILE);
    RFN_CHECK_ARG(I <= (1 << 28) && H <= (1 << 28) && tiles <= 0x7fffffffL, -1);   // (2^39 outputs: beyond any memory)
    RFN_CHECK_ARG(x && h && c && w_ih && w_hh && b_ih && b_hh && h_out && c_out && gates, -2);
    const dim3 grid((unsigned)tiles), block(64 * RFN_LC_WAVES);
    const bool vx = lc_vec_ok(x, w_ih, I), vh = lc_vec_ok(h, w_hh, H);
    hipStream_t s = (hipStream_t)stream;
#define RFN_LC_LAUNCH(VX, VH)                                                                                         \
    hipLaunchKernelGGL((lstm_cell_fwd_kernel<VX, VH>), grid, block, 0, s, x, h, c, w_ih, w_hh, b_ih, b_hh, h_out, c_out, \
                       gates, B, I, H)
    if (vx && vh) RFN_LC_LAUNCH(true, true);
    else if (vx) RFN_LC_LAUNCH(true, false);
    else if (vh) RFN_LC_LAUNCH(false, true);
    else RFN_LC_LAUNCH(false, false);
#undef RFN_LC_LAUNCH
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_lstm_cell_bwd_f32(const float* gh, const float* gc, const float* gates, const float* c,
                                     const float* c_out, float* D, float* g_c, float* g_bias, int B, int H,
                                     rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 1 && H >= 1 && H <= (1 << 28), -1);
    RFN_CHECK_ARG(gates && c && c_out && D && g_c && g_bias, -2);
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((unsigned)ceil_div(H, RFN_LC_BW_UNITS)),
                       dim3(RFN_LC_BW_UNITS * RFN_LC_BW_GROUPS), 0, (hipStream_t)stream, gh, gc, gates, c, c_out, D, g_c,
                       g_bias, B, H);
    RFN_LAUNCH_CHECK();
    return 0;
}
