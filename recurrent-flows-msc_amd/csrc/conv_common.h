// Shared pieces of the MFMA convolution kernels (fp32 and bf16x3).
#pragma once
#include "common.h"
#include "../../include/rfn_hip.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ConvParams {
    const float* in1;
    const float* in2;
    long in1_ns, in2_ns;
    int C1, C2;
    const float* wpk;
    float* out1;
    float* out2;
    long out1_ns, out2_ns;
    int Cout, cout_split, acc1, acc2;
    int N, H, W;
    int CoutP, Cin8;
    int ep_mode, act;
    const float* p0;
    const float* p1;
    int TWp, TH, TF, tw_shift, th_shift;
    int n_wtiles, n_htiles, n_ftiles;
    int ksplit;        // gridDim.z: the K (input channel chunk) range is split over z; slice z writes its partial outputs to
                       // ws + z * ws_stride (out1's elements, then out2's, both dense) and splitk_reduce_kernel adds
                       // the slices in order (deterministic: no float atomics)
    int w_lds_off;     // float offset of the weight tile inside dynamic LDS (16-byte aligned)
    // ep_mode 4 (data-gradient conv fused with the backward of the producer's ActNorm+activation epilogue):
    const float* ybuf;  // saved forward activation y = act((u+b)*exp(l)), same shape as the output
    long ybuf_ns;
    int npl;            // split-precision planes per operand: 0 / 2 = bf16x3, 3 = bf16x6 (generic tile kernel only)
    float* part;        // [2][Cout] sums Σ gu, Σ g*y, accumulated with float atomics (caller zeroes)
    float* ws;          // split-K partial outputs (rfn_workspace), ksplit slices of ws_stride floats
    long ws_stride;
};

// out[i] = sum_z ws[z * stride + i], z ascending (the second pass of a split-K convolution); n % 4 == 0 not required
static __global__ void splitk_reduce_kernel(const float* __restrict__ ws, long stride, int ksplit, float* __restrict__ out1,
                                            long n1, float* __restrict__ out2, long n2) {
    const long n = n1 + n2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float a = ws[i];
        for (int z = 1; z < ksplit; ++z) a += ws[(long)z * stride + i];
        if (i < n1) out1[i] = a;
        else out2[i - n1] = a;
    }
}
static inline void splitk_reduce(const ConvParams& p, hipStream_t s) {
    const long HW = (long)p.H * p.W, n1 = (long)p.N * p.cout_split * HW, n2 = (long)p.N * (p.Cout - p.cout_split) * HW;
    long blocks = (n1 + n2 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p.ws, p.ws_stride, p.ksplit, p.out1, n1,
                       p.out2, n2);
}

// ------------------------------------------------------------------------------------------------ tile-kernel skeleton
// What conv_mfma_kernel (conv.hip) and conv_b3_kernel (conv_bf16x3.hip) share up to the LDS image: the pixel tile of a
// workgroup, the halo staging descriptors, the weight-tile copy, the epilogue parameters and the K range of a split-K
// slice.  Every register array below is indexed by unrolled compile-time indices only.

// the pixel tile of workgroup blockIdx.x and its zero-padded LDS image
struct ConvTile {
    int x0, y0, f0;     // first column / row / frame
    int RW, FRM, IMG;   // padded row, one frame's padded image, the tile's padded image (slots per channel)
};
template <int PAD>
__device__ __forceinline__ ConvTile conv_tile_origin(const ConvParams& p) {
    int pt = blockIdx.x;
    const int wt = pt % p.n_wtiles;
    pt /= p.n_wtiles;
    const int ht = pt % p.n_htiles;
    const int ft = pt / p.n_htiles;
    ConvTile tl;
    tl.x0 = wt * p.TWp, tl.y0 = ht * p.TH, tl.f0 = ft * p.TF;
    tl.RW = p.TWp + 2 * PAD;
    tl.FRM = (p.TH + 2 * PAD) * tl.RW;
    tl.IMG = p.TF * tl.FRM;
    return tl;
}

// pixel q of the tile (a lane's pixels are q = (wpx * TPX + t) * 32 + l31, t < TPX)
struct ConvPixel {
    int lds_off;  // LDS offset of the top-left tap inside a channel's image
    int n, pix;   // frame, offset inside the channel plane
    bool valid;   // inside the image and the batch
};
__device__ __forceinline__ ConvPixel conv_pixel(const ConvParams& p, const ConvTile& tl, const int q) {
    const int col = q & (p.TWp - 1);
    const int row = (q >> p.tw_shift) & (p.TH - 1);
    const int f = q >> (p.tw_shift + p.th_shift);
    return {f * tl.FRM + row * tl.RW + col, tl.f0 + f, (tl.y0 + row) * p.W + tl.x0 + col,
            (tl.x0 + col < p.W) && (tl.y0 + row < p.H) && (tl.f0 + f < p.N)};
}

// Halo staging descriptors, computed ONCE per workgroup (the integer divisions live here, not in the K loop):
// thread -> image slot(s) r = slot + P2*j (j < NPOS) and channel phase; per chunk it then only adds a channel offset.
// P2 = slots per pass: a 1x1 tile of fewer than 256 pixels is covered by part of the block, so the parts take alternate
// channels (GROUPS of them); every other case uses all 256 threads as slots.  (P2 >= 64 keeps `phase` wave-uniform.)
// A launcher must refuse IMG > P2 * NPOS.
template <int KS, int BPX, int NPOS>
struct HaloSlots {
    static constexpr int GROUPS = (KS == 1 && BPX < 256) ? (BPX >= 64 ? 256 / BPX : 4) : 1;
    static constexpr int P2 = 256 / GROUPS;
    // the value of one slot of a channel plane: loaded unconditionally, zero where slot or channel does not exist
    static __device__ __forceinline__ float load(const float* src, const int off, const bool ok) {
        const float v = src[off];
        return ok ? v : 0.f;
    }
    // soff1 / soff2: element offset inside a channel plane of source 1 / 2; sok: inside the image and the batch; sin:
    // inside the tile's LDS image
    static __device__ __forceinline__ void fill(const ConvParams& p, const ConvTile& tl, const int slot,
                                                int (&soff1)[NPOS], int (&soff2)[NPOS], bool (&sok)[NPOS],
                                                bool (&sin)[NPOS]) {
        constexpr int PAD = KS / 2;
#pragma unroll
        for (int j = 0; j < NPOS; ++j) {
            const int r = slot + P2 * j;
            sin[j] = r < tl.IMG;
            const int f = r / tl.FRM;
            const int rr = r - f * tl.FRM;
            const int yy = rr / tl.RW;
            const int xx = rr - yy * tl.RW;
            const int gy = tl.y0 + yy - PAD, gx = tl.x0 + xx - PAD;
            sok[j] = sin[j] && (tl.f0 + f < p.N) && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            // invalid slots read element 0 of the channel plane (always mapped) and are zeroed after the load, so the
            // loads of a chunk are unconditional and the compiler can keep all of them in flight (no per-load wait)
            soff1[j] = sok[j] ? (int)(f * p.in1_ns) + gy * p.W + gx : 0;
            soff2[j] = sok[j] ? (int)(f * p.in2_ns) + gy * p.W + gx : 0;
        }
    }
};

// The weight tile of one K chunk: ITS_PER_CHUNK iterations of RUNS_PER_IT runs of BCO 16-byte units, copied verbatim
// from the packed buffer (unit index (it * RUNS_PER_IT + run) * CoutP + cout) into LDS, through registers so that the
// global loads of the next chunk stay in flight under the MFMAs.  Iterations past total_it are zero.
// tid is the kernel's thread index, handed over from its wprefetch / wcommit lambdas as it was before these were
// shared: the register allocation of the K loop follows it (profiles/README.md, conv_skeleton_*).
template <int RUNS_PER_IT, int ITS_PER_CHUNK, int BCO>
struct WeightTileCopy {
    static constexpr int UNITS = ITS_PER_CHUNK * RUNS_PER_IT * BCO;
    static constexpr int WPT = (UNITS + 255) / 256;  // units per thread per chunk
    u32x4 wstg[WPT];
    __device__ __forceinline__ void prefetch(const ConvParams& p, const int chunk, const int total_it, const int tid) {
        const u32x4* wp4 = reinterpret_cast<const u32x4*>(p.wpk);
        const long wblk = (long)blockIdx.y * BCO;
        const int it0 = chunk * ITS_PER_CHUNK;
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int e = tid + 256 * j;
            const int run = e / BCO, col = e % BCO;  // BCO is a power of two
            const int itg = it0 + run / RUNS_PER_IT;
            const bool ok = (UNITS % 256 == 0 || e < UNITS) && itg < total_it;
            const u32x4 v = wp4[((long)(ok ? itg : 0) * RUNS_PER_IT + run % RUNS_PER_IT) * p.CoutP + wblk + col];
            wstg[j] = ok ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    __device__ __forceinline__ void commit(u32x4* Ws4, const int tid) const {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int e = tid + 256 * j;
            if (UNITS % 256 == 0 || e < UNITS) Ws4[e] = wstg[j];
        }
    }
};

// epilogue parameters of this workgroup's BCO channels -> ep[2][BCO] in LDS (read after the K loop: a barrier orders
// the write)
template <int BCO, int THREADS = 256>
__device__ __forceinline__ void load_epilogue_params(const ConvParams& p, float* ep) {
    if (p.ep_mode != 0) {
        for (int c = threadIdx.x; c < BCO; c += THREADS) {
            const int co = blockIdx.y * BCO + c;
            float e0 = 0.f, e1 = 1.f;
            if (co < p.Cout) {
                if (p.ep_mode != 4) e0 = p.p0[co];
                if (p.ep_mode == 1 || p.ep_mode == 4) e1 = expf(p.p1[co]);
                if (p.ep_mode == 2) e1 = expf(3.f * p.p1[co]);
            }
            ep[c] = e0;
            ep[BCO + c] = e1;
        }
    }
}

// K chunks [begin, end) of split-K slice blockIdx.z; Cin8 counts groups of K_PER_GROUP channels, a chunk holds KC
struct ChunkRange { int begin, end; };
__device__ __forceinline__ ChunkRange chunk_range(const ConvParams& p, const int K_PER_GROUP, const int KC) {
    const int nchunks_all = (p.Cin8 * K_PER_GROUP + KC - 1) / KC;
    const int cps = (nchunks_all + p.ksplit - 1) / p.ksplit;  // chunks per K split
    const int chunk0 = blockIdx.z * cps;
    return {chunk0, chunk0 + cps < nchunks_all ? chunk0 + cps : nchunks_all};
}

// v = hi + mid (+ lo): hi = RNE_bf16(v), mid = RNE_bf16(v - hi), lo = RNE_bf16((v - hi) - mid); the fp32 subtractions
// are exact.  NPL = 2 leaves lo zero (16 significant bits: bf16x3), NPL = 3 gives 24 (bf16x6).
struct Bf16Split { __bf16 hi, mid, lo; };
template <int NPL>
__device__ __forceinline__ Bf16Split split_bf16(const float v) {
    const __bf16 h = (__bf16)v;
    const float r1 = v - (float)h;
    const __bf16 m = (__bf16)r1;
    return {h, m, NPL == 3 ? (__bf16)(r1 - (float)m) : (__bf16)0.f};
}

// Epilogue shared by the fp32 and the bf16x3 kernels (the C/D register layout of the 32x32 MFMA tile does not depend
// on the input dtype): per-channel affine + activation, bounds, output split over two tensors, accumulate / atomic.
// lds_part: the workgroup's [BCO][2] sums of ep_mode 4 in LDS (lds_shared: several waves share a channel); nullptr only
// from a kernel whose entry point refuses ep_mode 4.
// FASTONLY: the caller guarantees full cout tiles, one output tensor, no accumulate / split-K and ep_mode <= 3 -- only the
// straight store path is instantiated (the weight-stationary kernels have no registers to spare for the others).
template <int TCO, int TPX, int BCO, bool FASTONLY = false>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[TCO][TPX], const float* ep,
                                              const int co_base, const int wco, const int kk, const int HW,
                                              const int (&pn)[TPX], const int (&ppix)[TPX],
                                              const bool (&pvalid)[TPX], float* const lds_part,
                                              const bool lds_shared) {
    const int cl_base = wco * (32 * TCO) + 4 * kk;  // channel index inside the block for (a=0, r=0)
    const bool fast = FASTONLY || ((co_base + 32 * TCO <= p.Cout) && (p.cout_split == p.Cout));  // wave-uniform
    if (!FASTONLY && p.ep_mode == 4) {
        // g = this conv's result = grad wrt y = act((u+b)*exp(l)).  Emit gu = g*act'(y)*exp(l) (what the weight- and
        // data-gradient of the producer conv consume) and this wave's per-channel Σ gu (-> grad b) and Σ g*y (-> grad l),
        // so the separate elementwise+reduction pass over the 256-channel hidden tensors disappears.  Host guarantees
        // full cout tiles, a single output tensor and no split-K.
        if (co_base + 32 * TCO > p.Cout) return;  // whole wave past Cout (Cout % 64 == 0: never a partial tile)
        const float* ybase[TPX];
        float* obase[TPX];
#pragma unroll
        for (int t = 0; t < TPX; ++t) {
            const long off = (long)(co_base + 4 * kk) * HW + ppix[t];
            // masked pixels read frame 0 (always mapped) so that every load below is unconditional and batched
            ybase[t] = pvalid[t] ? p.ybuf + pn[t] * p.ybuf_ns + off : p.ybuf + (long)(co_base + 4 * kk) * HW;
            obase[t] = p.out1 + pn[t] * p.out1_ns + off;
        }
        const int l31 = threadIdx.x & 31;
#pragma unroll
        for (int a = 0; a < TCO; ++a) {
            float yv[16][TPX];
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < TPX; ++t)
                    yv[r][t] = ybase[t][(long)(a * 32 + (r & 3) + 8 * (r >> 2)) * HW];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cidx = a * 32 + (r & 3) + 8 * (r >> 2);
                const float e1 = ep[BCO + cl_base + cidx];
                float sb = 0.f, sl = 0.f;
#pragma unroll
                for (int t = 0; t < TPX; ++t) {
                    const float g = acc[a][t][r];
                    const float y = yv[r][t];
                    float slope = 1.f;
                    if (p.act == 1) slope = y > 0.f ? 1.f : 0.f;
                    if (p.act == 2) slope = y > 0.f ? 1.f : 0.2f;
                    const float gu = pvalid[t] ? g * slope * e1 : 0.f;
                    if (pvalid[t]) obase[t][(long)cidx * HW] = gu;
                    sb += gu;
                    sl += pvalid[t] ? g * y : 0.f;
                }
                sb = half_wave_sum_dpp(sb);  // lanes of one 32-lane half share the channel
                sl = half_wave_sum_dpp(sl);
                if (l31 == 16) {
                    // every ep_mode-4 caller hands over its workgroup's sums lds_part [BCO][2]
                    float* dst = lds_part + (cl_base + cidx) * 2;
                    if (lds_shared) {
                        // generic kernel: the workgroup's waves along the pixel axis share a channel -> LDS atomics; the
                        // workgroup then flushes [BCO][2] with full-width atomic instructions (a global float atomic is
                        // charged per WAVE INSTRUCTION, ~50 ns per CU, however few lanes are active: issuing them from
                        // here, two lanes at a time, cost 60-100 us per launch at the 8x8 / 4x4 levels)
                        atomicAdd(dst, sb);
                        atomicAdd(dst + 1, sl);
                    } else {
                        // persistent kernels: running sums of the workgroup (this lane is the only owner of its
                        // channel), flushed once per workgroup instead of one row per pixel tile
                        dst[0] += sb;
                        dst[1] += sl;
                    }
                }
            }
        }
        return;
    }
    if (fast) {
        float* obase[TPX];
        // (split-K: slice z stores into its own dense copy of out1 inside the workspace; out1 is dense then)
        float* const o1 = (!FASTONLY && p.ksplit > 1) ? p.ws + (long)blockIdx.z * p.ws_stride : p.out1;
#pragma unroll
        for (int t = 0; t < TPX; ++t)
            obase[t] = o1 + pn[t] * p.out1_ns + (long)(co_base + 4 * kk) * HW + ppix[t];
#pragma unroll
        for (int a = 0; a < TCO; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cidx = a * 32 + (r & 3) + 8 * (r >> 2);  // compile time
                float e0 = 0.f, e1 = 1.f;
                if (p.ep_mode != 0) {
                    e0 = blockIdx.z == 0 ? ep[cl_base + cidx] : 0.f;  // the additive term enters once per output
                    e1 = ep[BCO + cl_base + cidx];
                }
#pragma unroll
                for (int t = 0; t < TPX; ++t) {
                    float v = acc[a][t][r];
                    if (p.ep_mode != 0) v = (v + e0) * e1;
                    if (p.ep_mode == 1) {
                        if (p.act == 1) v = v > 0.f ? v : 0.f;
                        if (p.act == 2) v = v > 0.f ? v : 0.2f * v;
                    }
                    if (pvalid[t]) {
                        float* dst = obase[t] + (long)cidx * HW;
                        if (FASTONLY || p.ksplit > 1) {
                            *dst = v;
                        } else {
                            if (p.acc1) v += *dst;
                            *dst = v;
                        }
                    }
                }
            }
        }
        return;
    }
    if (FASTONLY) return;
    // general path: ragged Cout and/or output split over two tensors
#pragma unroll
    for (int a = 0; a < TCO; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cidx = a * 32 + (r & 3) + 8 * (r >> 2);
            const int co = co_base + cidx + 4 * kk;
            if (co >= p.Cout) continue;
            float e0 = 0.f, e1 = 1.f;
            if (p.ep_mode != 0) {
                e0 = blockIdx.z == 0 ? ep[cl_base + cidx] : 0.f;
                e1 = ep[BCO + cl_base + cidx];
            }
            const bool first = co < p.cout_split;
            float* obase = first ? p.out1 : p.out2;
            if (p.ksplit > 1)   // slice z of the workspace: [out1 dense | out2 dense]
                obase = p.ws + (long)blockIdx.z * p.ws_stride + (first ? 0 : (long)p.N * p.cout_split * HW);
            const long ons = first ? p.out1_ns : p.out2_ns;
            const int oc = first ? co : co - p.cout_split;
            const int accm = first ? p.acc1 : p.acc2;
#pragma unroll
            for (int t = 0; t < TPX; ++t) {
                if (!pvalid[t]) continue;
                float v = acc[a][t][r];
                if (p.ep_mode != 0) v = (v + e0) * e1;
                if (p.ep_mode == 1) {
                    if (p.act == 1) v = v > 0.f ? v : 0.f;
                    if (p.act == 2) v = v > 0.f ? v : 0.2f * v;
                }
                float* dst = obase + pn[t] * ons + (long)oc * HW + ppix[t];
                if (p.ksplit > 1) {
                    *dst = v;
                } else {
                    if (accm) v += *dst;
                    *dst = v;
                }
            }
        }
    }
}

static inline void tile_geometry(int H, int W, int BPX, int* TWp, int* TH, int* TF) {
    int tw = next_pow2(W);
    if (tw > 32) tw = 32;
    if (tw > BPX) tw = BPX;
    int th = next_pow2(H);
    if (th > BPX / tw) th = BPX / tw;
    *TWp = tw;
    *TH = th;
    *TF = BPX / (tw * th);
}

// ------------------------------------------------------------------------------------------------ shared host pieces
// tile geometry, shifts and tile counts into p (ConvParams or WgradParams); returns IMG, the padded LDS image's slots
template <class Params>
static inline int conv_tile_setup(Params& p, int BPX, int PAD) {
    tile_geometry(p.H, p.W, BPX, &p.TWp, &p.TH, &p.TF);
    p.tw_shift = ilog2(p.TWp);
    p.th_shift = ilog2(p.TH);
    p.n_wtiles = ceil_div(p.W, p.TWp);
    p.n_htiles = ceil_div(p.H, p.TH);
    p.n_ftiles = ceil_div(p.N, p.TF);
    return p.TF * (p.TH + 2 * PAD) * (p.TWp + 2 * PAD);
}

// The one split-K rule: split K over gridDim.z when the (pixel, cout) grid alone cannot fill 256 CUs (ConvLSTM: 128
// pixels x 800 couts x K = 6408).  Needs a linear epilogue (not ep_mode 1, nor the fused activation backward 4), dense
// zero-initialisable outputs and no accumulate flag.  Sets p.ksplit (and ws, ws_stride); -8 when no workspace.
static inline int conv_splitk_plan(ConvParams& p, int workgroups, int nchunks, hipStream_t s) {
    p.ksplit = 1;
    const int HW = p.H * p.W;
    const bool dense = p.out1_ns == (long)p.cout_split * HW &&
                       (p.cout_split == p.Cout || p.out2_ns == (long)(p.Cout - p.cout_split) * HW);
    if (workgroups < 128 && nchunks >= 8 && p.ep_mode != 1 && p.ep_mode != 4 && !p.acc1 && !p.acc2 && dense) {
        int ks_ = 512 / workgroups;
        if (ks_ > nchunks / 2) ks_ = nchunks / 2;
        if (ks_ > 1) {
            p.ksplit = ks_;
            p.ws_stride = (long)p.N * p.Cout * HW;
            p.ws = rfn_workspace(s, (size_t)ks_ * (size_t)p.ws_stride);
            if (!p.ws) return -8;
        }
    }
    return 0;
}

// launch of a generic tile kernel after conv_tile_setup: one workgroup per (pixel tile, BCO couts, K slice), then the
// split-K reduce (slices added in order: deterministic)
template <class Kern>
static int conv_tile_launch(Kern kern, ConvParams& p, int BCO, int nchunks, size_t lds, hipStream_t s) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    dim3 grid(p.n_wtiles * p.n_htiles * p.n_ftiles, ceil_div(p.Cout, BCO));
    const int rc = conv_splitk_plan(p, grid.x * grid.y, nchunks, s);
    if (rc) return rc;
    grid.z = p.ksplit;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, p);
    if (p.ksplit > 1) splitk_reduce(p, s);
    return 0;
}

// argument checks and ConvParams fill of the forward entry points (fn: the entry's name, for the error text); the
// caller adds its packed dimensions.  N == 0 passes: the caller returns early.  CONV_FWD_CHECK is RFN_CHECK_ARG of
// common.h with the entry's name in place of __func__: keep the two formats the same.
#define CONV_FWD_CHECK(cond, code)                                        \
    do {                                                                  \
        if (!(cond)) {                                                    \
            rfn_set_error("%s: argument check failed: %s", fn, #cond);    \
            return (code);                                                \
        }                                                                 \
    } while (0)
static int conv_fwd_params(ConvParams& p, const char* fn, const float* in1, long in1_ns, int C1, const float* in2,
                           long in2_ns, int C2, const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns,
                           int Cout, int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                           const float* p0, const float* p1, int act) {
    CONV_FWD_CHECK(in1 && wpk && out1 && C1 > 0 && C2 >= 0 && Cout > 0 && N >= 0 && H > 0 && W > 0, -1);
    CONV_FWD_CHECK(ks == 1 || ks == 3, -2);
    CONV_FWD_CHECK(C2 == 0 || in2, -3);
    CONV_FWD_CHECK(cout_split >= 0 && cout_split <= Cout && (cout_split == Cout || out2), -4);
    CONV_FWD_CHECK(ep_mode >= 0 && ep_mode <= 3 && (ep_mode == 0 || p0) && ((ep_mode != 1 && ep_mode != 2) || p1), -5);
    CONV_FWD_CHECK(((uintptr_t)wpk & 15) == 0, -6);
    memset(&p, 0, sizeof(p));
    p.in1 = in1; p.in2 = in2; p.in1_ns = in1_ns; p.in2_ns = in2_ns; p.C1 = C1; p.C2 = C2;
    p.wpk = wpk; p.out1 = out1; p.out2 = out2; p.out1_ns = out1_ns; p.out2_ns = out2_ns;
    p.Cout = Cout; p.cout_split = cout_split; p.acc1 = acc1; p.acc2 = acc2;
    p.N = N; p.H = H; p.W = W;
    p.ep_mode = ep_mode; p.act = act; p.p0 = p0; p.p1 = p1;
    return 0;
}
#undef CONV_FWD_CHECK
