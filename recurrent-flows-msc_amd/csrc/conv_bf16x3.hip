// Split-precision ("bf16x3") implicit-GEMM convolution for gfx950.
//
// fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 MFMA rate.  Every fp32 operand is split into two bf16
// numbers  x = hi + lo  (hi = RNE_bf16(x), lo = RNE_bf16(x - hi), 16 significant bits together) and the product is
// formed as  a*b ≈ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi  with three v_mfma_f32_32x32x16_bf16 accumulating in fp32
// (the dropped a_lo*b_lo term is ≤ 2^-16 relative).  Measured on the oracle (tools/ notes in DESIGN.md): the nll /
// bits-per-dim error against an fp64 reference is ~1e-5 relative — ten times the plain fp32 error and a tenth of the
// 1e-4 budget — for 3/16 of the fp32-MFMA cycles.
//
// Same GEMM orientation, pixel tiling, halo staging, descriptors, register prefetch, split-K and epilogue as conv.hip,
// shared through conv_common.h (D[cout][pixel], C/D register layout is dtype independent).  What differs is the LDS
// image: an MFMA operand lane needs 8 consecutive k (channels) of one row/column in one 16-byte register quad, so
// activations are stored as [plane hi|lo][8-channel group][slot][8 x bf16] and weights (pre-split on the device by the
// pack kernel) as [iteration][plane][k-group][cout][8 x bf16]; both fragments are single ds_read_b128.
#include "conv_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

static inline void packed_dims_b3(int Cout_l, int Cin_l, int* CoutP, int* Cin16) {
    *CoutP = ((Cout_l + 255) / 256) * 256;
    *Cin16 = (Cin_l + 15) / 16;
}

extern "C" long rfn_packed_weight_size_bf16x3(int Cout, int Cin, int ks) {
    // in FLOATS (4 bytes), large enough for both orientations
    int a, b, c, d;
    packed_dims_b3(Cout, Cin, &a, &b);
    packed_dims_b3(Cin, Cout, &c, &d);
    long s0 = (long)b * ks * ks * 4 * a * 4, s1 = (long)d * ks * ks * 4 * c * 4;  // units * 16 B / 4 B
    return s0 > s1 ? s0 : s1;
}
extern "C" long rfn_packed_weight_size_bf16x6(int Cout, int Cin, int ks) {
    return rfn_packed_weight_size_bf16x3(Cout, Cin, ks) / 2 * 3;  // three planes instead of two
}

// ---- the weight pack: up to PACK_TABLE_MAX weights per launch, the descriptors by value in the kernel arguments,
// blockIdx.y = descriptor.  mode 0: forward conv, 1: data-gradient conv (transposed + mirrored taps), 2: tap-expanded 1x1
// form of a 3x3 conv with tiny Cout (logical weight w'[tap*Cout + co][ci] = w[co][ci][tap], see rfn_tap_gather_f32);
// mode + 4: NPL = 3 planes.
// packed unit (16 bytes = 8 bf16) index: (((c16*T + tap)*NPL + plane)*2 + g)*CoutP + co ; element j <-> cin = c16*16+g*8+j
// NPL = 2: (hi, lo) -- bf16x3;  NPL = 3: (hi, mid, lo), 24 significant bits -- "bf16x6" (six products per fp32 product)
using PackDesc = rfn_pack_desc;
static_assert(sizeof(rfn_pack_desc) == 32, "rfn_pack_desc layout is part of the ABI");
#define PACK_TABLE_MAX 64
struct PackTable { PackDesc d[PACK_TABLE_MAX]; };
__global__ void pack_weights_table_b3_kernel(const PackTable t) {
    const PackDesc d = t.d[blockIdx.y];
    const int T_src = d.ks * d.ks;
    const int NPL = (d.mode & 4) ? 3 : 2, mode = d.mode & 3;  // (mode + 4: three planes = bf16x6)
    int Co_l, Ci_l, T;
    if (mode == 0) { Co_l = d.Cout; Ci_l = d.Cin; T = T_src; }
    else if (mode == 1) { Co_l = d.Cin; Ci_l = d.Cout; T = T_src; }
    else { Co_l = T_src * d.Cout; Ci_l = d.Cin; T = 1; }
    const int CoutP = ((Co_l + 255) / 256) * 256, Cin16 = (Ci_l + 15) / 16;
    bf16x8* wpk = reinterpret_cast<bf16x8*>(d.wpk);
    const long total = (long)Cin16 * T * 2 * CoutP;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int co = (int)(idx % CoutP);
        long r = idx / CoutP;
        const int g = (int)(r & 1);
        r >>= 1;
        const int tap = (int)(r % T);
        const int c16 = (int)(r / T);
        bf16x8 hi, lo, l3;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = c16 * 16 + g * 8 + j;
            float v = 0.f;
            if (co < Co_l && ci < Ci_l) {
                if (mode == 0)
                    v = d.w[((long)co * d.Cin + ci) * T_src + tap];
                else if (mode == 1)
                    v = d.w[((long)ci * d.Cin + co) * T_src + (T_src - 1 - tap)];
                else
                    v = d.w[((long)(co % d.Cout) * d.Cin + ci) * T_src + co / d.Cout];
            }
            const Bf16Split sp = split_bf16<3>(v);
            hi[j] = sp.hi;
            lo[j] = sp.mid;
            l3[j] = sp.lo;
        }
        const long base = ((long)(c16 * T + tap) * NPL) * 2 * CoutP;
        wpk[base + (long)(0 * 2 + g) * CoutP + co] = hi;
        wpk[base + (long)(1 * 2 + g) * CoutP + co] = lo;
        if (NPL == 3) wpk[base + (long)(2 * 2 + g) * CoutP + co] = l3;
    }
}
/* n descriptors in HOST memory: ceil(n / 64) launches, the table travels in the kernel arguments */
extern "C" int rfn_pack_conv_weights_hostdescs_bf16x3(const void* descs_host, int n, rfn_stream_t stream) {
    RFN_CHECK_ARG(descs_host && n >= 0, -1);
    const PackDesc* d = reinterpret_cast<const PackDesc*>(descs_host);
    for (int i = 0; i < n; ++i)
        RFN_CHECK_ARG(d[i].w && d[i].wpk && d[i].Cout > 0 && d[i].Cin > 0 && (d[i].ks == 1 || d[i].ks == 3) &&
                      ((uintptr_t)d[i].wpk & 15) == 0, -2);
    for (int i0 = 0; i0 < n; i0 += PACK_TABLE_MAX) {
        const int m = n - i0 < PACK_TABLE_MAX ? n - i0 : PACK_TABLE_MAX;
        PackTable t;
        memset(&t, 0, sizeof(t));
        long most = 0;   // blocks per matrix follow the LARGEST one of the launch (a 2 M-element weight on 24 blocks is 0.1 ms)
        for (int i = 0; i < m; ++i) {
            t.d[i] = d[i0 + i];
            const int T_src = t.d[i].ks * t.d[i].ks, mode = t.d[i].mode & 3;
            const int Co_l = mode == 0 ? t.d[i].Cout : (mode == 1 ? t.d[i].Cin : T_src * t.d[i].Cout);
            const int Ci_l = mode == 1 ? t.d[i].Cout : t.d[i].Cin, T = mode == 2 ? 1 : T_src;
            const long total = (long)((Ci_l + 15) / 16) * T * 2 * (((Co_l + 255) / 256) * 256);
            most = total > most ? total : most;
        }
        int gx = (int)((most + 255) / 256);
        gx = gx < 24 ? 24 : (gx > 1024 ? 1024 : gx);
        while ((long)gx * m > 16384) gx = (gx + 1) / 2;   // (many matrices: the launch stays a few thousand blocks)
        hipLaunchKernelGGL(pack_weights_table_b3_kernel, dim3(gx, m), dim3(256), 0, (hipStream_t)stream, t);
    }
    RFN_LAUNCH_CHECK();
    return 0;
}
// one weight: a one-descriptor table
extern "C" int rfn_pack_conv_weight_bf16x3(const float* w, float* wpk, int Cout, int Cin, int ks, int transpose_flip,
                                           rfn_stream_t stream) {
    const PackDesc d = {w, wpk, Cout, Cin, ks, transpose_flip ? 1 : 0};
    return rfn_pack_conv_weights_hostdescs_bf16x3(&d, 1, stream);
}
extern "C" int rfn_pack_conv_weight_bf16x6(const float* w, float* wpk, int Cout, int Cin, int ks, int transpose_flip,
                                           rfn_stream_t stream) {
    const PackDesc d = {w, wpk, Cout, Cin, ks, (transpose_flip ? 1 : 0) + 4};
    return rfn_pack_conv_weights_hostdescs_bf16x3(&d, 1, stream);
}

// Image slots per staging thread (HaloSlots): a slot holds eight floats per channel group here (one in conv.hip), so
// the 64-pixel 3x3 tile stages a single slot -- its image has at most 256 slots down to 2x2 maps (16 frames x 16);
// smaller maps are refused (-7) and belong to the small-map kernels.  conv_f32_npos (conv.hip) keeps 2 below 128
// pixels; the difference is historical.
static constexpr int conv_b3_npos(int KS, int BPX) { return KS == 1 ? 1 : (BPX >= 256 ? 4 : (BPX >= 128 ? 2 : 1)); }

// NPL = 2: two bf16 pieces per operand, three products (bf16x3); NPL = 3: three pieces, six products ("bf16x6", 24
// significant bits: the fp32-grade arithmetic of the forward convolutions at the levels the fused kernel does not take)
template <int KS, int WCO, int WPX, int TCO, int TPX, int KC, int NPL = 2>
__global__ __launch_bounds__(256) void conv_b3_kernel(const ConvParams p) {
    constexpr int T = KS * KS, PAD = KS / 2;
    constexpr int BCO = 32 * TCO * WCO, BPX = 32 * TPX * WPX;
    constexpr int NG = KC / 8;    // 8-channel groups per chunk
    constexpr int NS = KC / 16;   // k16 steps per chunk and tap
    static_assert(WCO * WPX == 4 && KC % 16 == 0, "4 waves, whole k16 steps");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wco = wave / WPX, wpx = wave % WPX;
    const int l31 = lane & 31, kk = lane >> 5;
    const int HW = p.H * p.W;
    const int Cin = p.C1 + p.C2;

    const ConvTile tl = conv_tile_origin<PAD>(p);
    const int RW = tl.RW, IMG = tl.IMG;
    const int co_base = blockIdx.y * BCO + wco * (32 * TCO);

    // LDS: Bs[plane][NG][IMG] units | Ws[NS*T][plane][2][BCO] units | ep[2][BCO] floats
    bf16x8* Bs = reinterpret_cast<bf16x8*>(lds_raw);
    bf16x8* Ws = Bs + NPL * NG * IMG;
    float* ep = reinterpret_cast<float*>(Ws + NS * T * NPL * 2 * BCO);

    int lds_off[TPX], pn[TPX], ppix[TPX];
    bool pvalid[TPX];
#pragma unroll
    for (int t = 0; t < TPX; ++t) {
        const ConvPixel px = conv_pixel(p, tl, (wpx * TPX + t) * 32 + l31);
        lds_off[t] = px.lds_off, pn[t] = px.n, ppix[t] = px.pix, pvalid[t] = px.valid;
    }

    f32x16 acc[TCO][TPX];
#pragma unroll
    for (int a = 0; a < TCO; ++a)
#pragma unroll
        for (int t = 0; t < TPX; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][t][r] = 0.f;
    constexpr bool SINGLE = TCO * TPX == 1;
    f32x16 accx[2];
    if (SINGLE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[0][r] = accx[1][r] = 0.f;
    }

    // ---- activations: eight channels (one group) per slot in registers, split into planes on the way into LDS
    constexpr int NPOS = conv_b3_npos(KS, BPX);
    typedef HaloSlots<KS, BPX, NPOS> Halo;
    constexpr int GROUPS = Halo::GROUPS, P2 = Halo::P2;
    const int slot = tid & (P2 - 1);
    const int phase = __builtin_amdgcn_readfirstlane(tid / P2);  // wave-uniform: keeps channel math scalar
    int soff1[NPOS], soff2[NPOS];
    bool sok[NPOS], sin[NPOS];
    Halo::fill(p, tl, slot, soff1, soff2, sok, sin);
    const float* in1b = p.in1 + (long)tl.f0 * p.in1_ns;
    const float* in2b = p.in2 ? p.in2 + (long)tl.f0 * p.in2_ns : p.in1;
    constexpr int NGT = (NG + GROUPS - 1) / GROUPS;  // channel groups per thread
    float stg[NGT][NPOS][8];
    auto prefetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < NGT; ++i) {
            const int gi = phase + GROUPS * i;  // scalar: 8-channel group inside the chunk
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int ch = chunk * KC + gi * 8 + c;
                const bool chv = gi < NG && ch < Cin;
                const int chc = chv ? ch : 0;
                const bool first = chc < p.C1;
                const float* src = first ? in1b + (long)chc * HW : in2b + (long)(chc - p.C1) * HW;
#pragma unroll
                for (int j = 0; j < NPOS; ++j)
                    stg[i][j][c] = Halo::load(src, first ? soff1[j] : soff2[j], sok[j] && chv);
            }
        }
    };
    auto commit = [&]() {  // split to (hi, mid[, lo]) and store the 16-byte units
#pragma unroll
        for (int i = 0; i < NGT; ++i) {
            const int gi = phase + GROUPS * i;
            if (gi < NG) {
#pragma unroll
                for (int j = 0; j < NPOS; ++j) {
                    if (sin[j]) {
                        bf16x8 hi, lo, l3;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const Bf16Split sp = split_bf16<NPL>(stg[i][j][c]);
                            hi[c] = sp.hi;
                            lo[c] = sp.mid;
                            if (NPL == 3) l3[c] = sp.lo;
                        }
                        const int r = slot + P2 * j;
                        Bs[(0 * NG + gi) * IMG + r] = hi;
                        Bs[(1 * NG + gi) * IMG + r] = lo;
                        if (NPL == 3) Bs[(2 * NG + gi) * IMG + r] = l3;
                    }
                }
            }
        }
    };

    // ---- weight tile of a chunk: NS*T iterations of NPL*2 runs (plane, k-group) of BCO units
    const int total_it = p.Cin8 * T;  // Cin8 holds Cin16 for this kernel
    WeightTileCopy<NPL * 2, NS * T, BCO> wtile;
    u32x4* Ws4 = reinterpret_cast<u32x4*>(Ws);
    auto wprefetch = [&](int chunk) { wtile.prefetch(p, chunk, total_it, tid); };
    auto wcommit = [&]() { wtile.commit(Ws4, tid); };

    load_epilogue_params<BCO>(p, ep);

    const ChunkRange kr = chunk_range(p, 16, KC);
    if (kr.begin < kr.end) {
        prefetch(kr.begin);
        wprefetch(kr.begin);
    }
    const bf16x8* wa = Ws + kk * BCO + wco * (32 * TCO) + l31;  // + ((itl*2 + plane)*2)*BCO + a*32
    for (int chunk = kr.begin; chunk < kr.end; ++chunk) {
        __syncthreads();
        commit();
        wcommit();
        __syncthreads();
        if (chunk + 1 < kr.end) {
            prefetch(chunk + 1);
            wprefetch(chunk + 1);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int tap = 0; tap < T; ++tap) {
                const int itl = s * T + tap;
                const int tapoff = (tap / KS) * RW + (tap % KS);
                bf16x8 ah[TCO], al[TCO], a3[TCO], bh[TPX], bl[TPX], b3[TPX];
#pragma unroll
                for (int a = 0; a < TCO; ++a) {
                    ah[a] = wa[((itl * NPL + 0) * 2) * BCO + a * 32];
                    al[a] = wa[((itl * NPL + 1) * 2) * BCO + a * 32];
                    if (NPL == 3) a3[a] = wa[((itl * NPL + 2) * 2) * BCO + a * 32];
                }
                const bf16x8* bb = Bs + (2 * s + kk) * IMG + tapoff;
#pragma unroll
                for (int t = 0; t < TPX; ++t) {
                    bh[t] = bb[lds_off[t]];
                    bl[t] = bb[NG * IMG + lds_off[t]];
                    if (NPL == 3) b3[t] = bb[2 * NG * IMG + lds_off[t]];
                }
#pragma unroll
                for (int a = 0; a < TCO; ++a)
#pragma unroll
                    for (int t = 0; t < TPX; ++t) {
                        if (NPL == 3) {
                            // six products, smallest first: mid*mid, hi*lo3, lo3*hi, hi*mid, mid*hi, hi*hi
                            if (SINGLE) {
                                accx[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bl[t], accx[0], 0, 0, 0);
                                accx[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], b3[t], accx[1], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[a], bh[t], acc[a][t], 0, 0, 0);
                                accx[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[t], accx[0], 0, 0, 0);
                                accx[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[t], accx[1], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[t], acc[a][t], 0, 0, 0);
                            } else {
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bl[t], acc[a][t], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], b3[t], acc[a][t], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[a], bh[t], acc[a][t], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[t], acc[a][t], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[t], acc[a][t], 0, 0, 0);
                                acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[t], acc[a][t], 0, 0, 0);
                            }
                        } else if (SINGLE) {
                            // one accumulator tile per wave: three independent chains instead of one of 3*T*NS
                            // dependent MFMAs per chunk (each waits for the previous result)
                            acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[t], acc[a][t], 0, 0, 0);
                            accx[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[t], accx[0], 0, 0, 0);
                            accx[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[t], accx[1], 0, 0, 0);
                        } else {
                            acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[t], acc[a][t], 0, 0, 0);
                            acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[t], acc[a][t], 0, 0, 0);
                            acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[t], acc[a][t], 0, 0, 0);
                        }
                    }
            }
        }
    }
    if (SINGLE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] += accx[0][r] + accx[1][r];
    }

    float* psum = ep + 2 * BCO;  // [BCO][2] sums of the fused activation backward (ep_mode 4)
    if (p.ep_mode == 4)
        for (int c = tid; c < 2 * BCO; c += 256) psum[c] = 0.f;
    __syncthreads();
    conv_epilogue<TCO, TPX, BCO>(p, acc, ep, co_base, wco, kk, HW, pn, ppix, pvalid, psum, true);
    if (p.ep_mode == 4) {
        __syncthreads();
        for (int c = tid; c < 2 * BCO; c += 256) {
            const int co = blockIdx.y * BCO + (c >> 1);
            if (co < p.Cout) atomicAdd(&p.part[(long)(c & 1) * p.Cout + co], psum[c]);
        }
    }
}

template <int KS, int WCO, int WPX, int TCO, int TPX, int KC, int NPL = 2>
static int launch_conv_b3(ConvParams& p, hipStream_t s) {
    constexpr int BCO = 32 * TCO * WCO, BPX = 32 * TPX * WPX;
    const int IMG = conv_tile_setup(p, BPX, KS / 2);
    constexpr int SLOTS = HaloSlots<KS, BPX, conv_b3_npos(KS, BPX)>::P2 * conv_b3_npos(KS, BPX);
    if (IMG > SLOTS) {
        rfn_set_error("conv2d(bf16x3): map %dx%d needs %d LDS slots (> %d supported)", p.H, p.W, IMG, SLOTS);
        return -7;
    }
    const size_t lds =
        (size_t)NPL * (KC / 8) * IMG * 16 + (size_t)(KC / 16) * KS * KS * NPL * 2 * BCO * 16 + 4 * BCO * 4;
    const int nchunks = (p.Cin8 * 16 + KC - 1) / KC;
    return conv_tile_launch(conv_b3_kernel<KS, WCO, WPX, TCO, TPX, KC, NPL>, p, BCO, nchunks, lds, s);
}

// ------------------------------------------------------------------------------------------------ kernel choice
// Every instantiation a split-precision convolution can run is one route: choose_conv_b3 is the only place a shape is
// mapped to a route (it launches nothing), dispatch_conv_b3 the only place a route is mapped to a launch, and the label
// queries of the C ABI read the same table.  Generic tile kernel: <KS,WCO,WPX,TCO,TPX,KC>, BPX = 32 * TPX * WPX pixels
// per workgroup; weight-stationary kernels: BPX pixels per tile of a persistent workgroup, WPX = 0.
enum ConvB3Route { G3_32x128, G3_64x64, G3_64x128, G1_32x128, G1_64x64, G1_128x128, G1_256x64, WS1, WS3_ACTBWD, WS3_27,
                   WS3_45 };
static const struct { const char* label; int BPX, WPX; } kConvB3Routes[] = {
    {"conv_b3_kernel<3,1,4,1,1,16>", 128, 4},   // 32 co x 128 px
    {"conv_b3_kernel<3,2,2,1,1,16>", 64, 2},    // 64 co x 64 px (32-channel chunks measured 1.6x slower)
    {"conv_b3_kernel<3,2,2,1,2,16>", 128, 2},   // 64 co x 128 px
    {"conv_b3_kernel<1,1,4,1,1,32>", 128, 4},
    {"conv_b3_kernel<1,2,2,1,1,32>", 64, 2},    // 64 co x 64 px
    {"conv_b3_kernel<1,2,2,2,2,32>", 128, 2},   // 128 co x 128 px
    {"conv_b3_kernel<1,4,1,2,2,32>", 64, 1},    // 256 co x 64 px: the input tile is read once for 256 couts
    {"conv1x1_ws_kernel<16>", 32, 0},
    {"conv3x3_ws_kernel<1,2,0>", 64, 0},        // 9 units, fused activation backward (ep_mode 4)
    {"conv3x3_ws_kernel<3,2,1>", 64, 0},        // Cin <= 24: 27 units (112 weight registers), two accumulator tiles per step
    {"conv3x3_ws_kernel<5,1,1>", 32, 0},        // Cin <= 40: 45 units (184), one
};
static_assert(sizeof(kConvB3Routes) / sizeof(kConvB3Routes[0]) == WS3_45 + 1, "one row per route");

// needs of p: N, H, W, C1, C2, Cout, cout_split, acc1, ep_mode, npl
static ConvB3Route choose_conv_b3(const ConvParams& p, int ks) {
    static const bool ws_off = getenv("RFN_CONV_WS") && atoi(getenv("RFN_CONV_WS")) == 0;
    const int Cin = p.C1 + p.C2, Cout = p.Cout;
    const long npix = (long)p.N * p.H * p.W;
    // bf16x6 (npl == 3): the generic tile kernel only (forward convolutions of the middle flow levels)
    if (p.npl != 3 && !ws_off && Cout % 256 == 0 && npix >= 64L * 256) {
        if (ks == 1 && p.C2 == 0 && Cin > 128 && Cin <= 256) return WS1;
        // the tile launch_conv3x3_ws_t cuts: TW = min(W, 32) columns by TH = 32 * PT / TW rows (PT = 2 for the 9- and
        // 27-unit variants, 1 for the 45-unit one).  A frame must hold at least one: a 1 x W map with W >= 64 and PT = 2
        // has TH = 2 and would get zero tiles
        const int PT = (p.ep_mode == 4 || Cin <= 24) ? 2 : 1;
        const int TH = 32 * PT / (p.W >= 32 ? 32 : (p.W > 0 ? p.W : 1));
        const bool pow2 = (p.H & (p.H - 1)) == 0 && (p.W & (p.W - 1)) == 0;
        if (ks == 3 && pow2 && p.W >= 8 && (long)p.H * p.W >= 64 && p.H >= TH && p.cout_split == Cout && !p.acc1) {
            if (p.ep_mode == 4 && Cin <= 8 && p.C2 == 0) return WS3_ACTBWD;
            if (p.ep_mode >= 0 && p.ep_mode <= 3 && Cin <= 40) return Cin <= 24 ? WS3_27 : WS3_45;
        }
    }
    const bool few_px = npix * ((Cout + 127) / 128) < 256L * 128;
    if (ks == 3) return Cout <= 32 ? G3_32x128 : (few_px ? G3_64x64 : G3_64x128);
    if (Cout <= 32) return G1_32x128;
    if (few_px || Cout <= 64) return G1_64x64;
    return Cout <= 128 ? G1_128x128 : G1_256x64;
}
static int dispatch_conv_b3(ConvParams& p, int ks, hipStream_t s);

static ConvParams conv_b3_shape(int npl, int C1, int C2, int Cout, int cout_split, int acc1, int ep_mode, int N, int H,
                                int W) {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.npl = npl; p.C1 = C1; p.C2 = C2; p.Cout = Cout; p.cout_split = cout_split; p.acc1 = acc1; p.ep_mode = ep_mode;
    p.N = N; p.H = H; p.W = W;
    return p;
}
extern "C" const char* rfn_conv2d_kernel_label_bf16x3(int npl, int ks, int C1, int C2, int Cout, int cout_split, int acc1,
                                                     int ep_mode, int N, int H, int W) {
    return kConvB3Routes[choose_conv_b3(conv_b3_shape(npl, C1, C2, Cout, cout_split, acc1, ep_mode, N, H, W), ks)].label;
}
// number of partial-sum rows rfn_conv2d_dgrad_act_bf16x3 writes for (N,H,W,ks,Cout): pixel tiles x waves along pixels,
// or one row per persistent workgroup of a weight-stationary kernel
extern "C" int rfn_conv2d_dgrad_act_rows_bf16x3(int N, int H, int W, int ks, int Cout, int Cin) {
    const auto& r = kConvB3Routes[choose_conv_b3(conv_b3_shape(2, Cin, 0, Cout, Cout, 0, 4, N, H, W), ks)];
    if (r.WPX == 0) {
        const long nt = ((long)N * H * W + r.BPX - 1) / r.BPX;
        return (int)(nt < 256 ? nt : 256);
    }
    int TWp, TH, TF;
    tile_geometry(H, W, r.BPX, &TWp, &TH, &TF);
    return ceil_div(W, TWp) * ceil_div(H, TH) * ceil_div(N, TF) * r.WPX;
}

// data-gradient conv fused with the backward of the producer's Conv2dNorm epilogue (ActNorm + activation):
//   g  = conv(gin, wpk)                      (wpk packed with transpose_flip = 1)
//   gu = g * act'(y) * exp(logs[c])          -> out        (y = saved forward activation, same shape as out)
//   part[0][c] += Σ_pixels gu ,  part[1][c] += Σ g*y     (float atomics; the caller zeroes part [2][Cout])
// Cout must be a multiple of 64.
extern "C" int rfn_conv2d_dgrad_act_bf16x3(const float* gin, long gin_ns, int Cin, const float* wpk, const float* y,
                                           long y_ns, const float* logs, int act, float* out, long out_ns, float* part,
                                           int Cout, int N, int H, int W, int ks, rfn_stream_t stream) {
    RFN_CHECK_ARG(gin && wpk && y && logs && out && part && Cin > 0 && Cout > 0 && Cout % 64 == 0, -1);
    RFN_CHECK_ARG((ks == 1 || ks == 3) && N >= 0 && H > 0 && W > 0 && ((uintptr_t)wpk & 15) == 0, -2);
    if (N == 0) return 0;
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in1 = gin; p.in1_ns = gin_ns; p.C1 = Cin; p.wpk = wpk; p.out1 = out; p.out1_ns = out_ns;
    p.Cout = Cout; p.cout_split = Cout; p.N = N; p.H = H; p.W = W;
    packed_dims_b3(Cout, Cin, &p.CoutP, &p.Cin8);
    p.ep_mode = 4; p.act = act; p.p1 = logs; p.ybuf = y; p.ybuf_ns = y_ns; p.part = part;
    int rc = dispatch_conv_b3(p, ks, (hipStream_t)stream);
    if (rc) return rc;
    RFN_LAUNCH_CHECK();
    return 0;
}

// shared body of rfn_conv2d_fwd_bf16x3 (npl = 2) and rfn_conv2d_fwd_bf16x6 (npl = 3)
static int conv2d_fwd_split(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                            const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                            int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                            const float* p0, const float* p1, int act, int npl, rfn_stream_t stream) {
    ConvParams p;
    int rc = conv_fwd_params(p, __func__, in1, in1_ns, C1, in2, in2_ns, C2, wpk, out1, out1_ns, out2, out2_ns, Cout,
                             cout_split, acc1, acc2, N, H, W, ks, ep_mode, p0, p1, act);
    if (rc || N == 0) return rc;
    packed_dims_b3(Cout, C1 + C2, &p.CoutP, &p.Cin8);
    p.npl = npl;
    rc = dispatch_conv_b3(p, ks, (hipStream_t)stream);
    if (rc) return rc;
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_conv2d_fwd_bf16x3(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                                     const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                                     int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                                     const float* p0, const float* p1, int act, rfn_stream_t stream) {
    return conv2d_fwd_split(in1, in1_ns, C1, in2, in2_ns, C2, wpk, out1, out1_ns, out2, out2_ns, Cout, cout_split, acc1,
                            acc2, N, H, W, ks, ep_mode, p0, p1, act, 2, stream);
}
// same convolution on three bf16 pieces per operand and six MFMAs per product (24 significant bits, fp32-grade): wpk from
// rfn_pack_conv_weight_bf16x6
extern "C" int rfn_conv2d_fwd_bf16x6(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                                     const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                                     int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                                     const float* p0, const float* p1, int act, rfn_stream_t stream) {
    return conv2d_fwd_split(in1, in1_ns, C1, in2, in2_ns, C2, wpk, out1, out1_ns, out2, out2_ns, Cout, cout_split, acc1,
                            acc2, N, H, W, ks, ep_mode, p0, p1, act, 3, stream);
}


// ------------------------------------------------------------------------------------------------ weight-stationary 1x1
// The flow's hidden 1x1 convolution (Hd -> Hd = 256 -> 256, forward and data gradient, 60 launches per step on up to
// 622 592 pixels) with the weights held in REGISTERS: 8 waves, wave w owns output channels [32w, 32w+32) and keeps their
// 32 x 256 (hi, lo) slab in 128 VGPRs for the whole launch, so the only LDS traffic is the activation tile (staged once,
// read by all 8 waves) and nothing but activations is streamed.  One persistent workgroup per CU sweeps 64-pixel
// tiles; the loads of tile t+1 are in flight while tile t is multiplied and stored (double-buffered LDS, one barrier
// per tile).  Per tile and CU: 96 MFMAs per wave against 64 KB read + 64 KB written -> the kernel sits on the HBM roof
// instead of the issue / LDS / barrier overheads of the generic tile kernel above (which re-stages the 256 x 32
// weight chunk for every 64 pixels).
template <int NSTEPS>
__global__ __launch_bounds__(512) void conv1x1_ws_kernel(const ConvParams p, const int n_tiles, const int hw_shift) {
    constexpr int NG = NSTEPS * 2;  // 8-channel units per pixel
    constexpr int TP = 32;          // pixels per tile
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16x8* Bs = reinterpret_cast<bf16x8*>(lds_raw);                       // [2 buffers][plane][NG][TP]
    float* ep = reinterpret_cast<float*>(Bs + 2 * 2 * NG * TP);            // [2][256]
    float* psum = ep + 2 * 256;                                            // [256][2] running sums of ep_mode 4
    for (int c = threadIdx.x; c < 512; c += 512) psum[c] = 0.f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int HW = p.H * p.W;
    const long total = (long)p.N * HW;
    const int co_base = blockIdx.y * 256 + wave * 32;

    // weights -> registers (packed unit index ((s*2 + plane)*2 + kk)*CoutP + co, see pack_weights_table_b3_kernel)
    bf16x8 wh[NSTEPS], wl[NSTEPS];
    {
        const bf16x8* wp = reinterpret_cast<const bf16x8*>(p.wpk) + co_base + l31;
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            const bool ok = s < p.Cin8;  // Cin8 holds the number of 16-channel steps
            const int sc = ok ? s : 0;
            const bf16x8 h = wp[(long)((sc * 2 + 0) * 2 + kk) * p.CoutP];
            const bf16x8 l = wp[(long)((sc * 2 + 1) * 2 + kk) * p.CoutP];
            const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            wh[s] = ok ? h : z;
            wl[s] = ok ? l : z;
        }
    }
    load_epilogue_params<256, 512>(p, ep);

    // Staging role: pixel l31 of the tile, channel units 2*wave + kk + 16*i (i < NG/16).  Loads go through one buffer
    // descriptor: a per-lane 32-bit byte offset (frame, pixel, kk) plus a scalar channel offset, so the loads of a tile
    // need no per-load 64-bit address registers (they would not fit next to the weights).
    constexpr int NU = NG / 16;  // units per thread and tile
    const int Cin = p.C1;
    const unsigned long in_bytes = (unsigned long)p.N * (unsigned long)p.in1_ns * 4ul;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in1), 0,
                                                        in_bytes > 0xFFFFFFFFul ? 0xFFFFFFFFu : (unsigned)in_bytes, 0x00020000);
    float stg[NU][8];
    bool sval = false;
    auto split_q = [&](long q, int& n, int& pix) {
        if (hw_shift >= 0) {
            n = (int)(q >> hw_shift);
            pix = (int)(q & (HW - 1));
        } else {
            n = (int)(q / HW);
            pix = (int)(q - (long)n * HW);
        }
    };
    auto prefetch = [&](int tile) {
        const long q = (long)tile * TP + l31;
        sval = tile < n_tiles && q < total;
        int n, pix;
        split_q(sval ? q : 0, n, pix);
        const unsigned voff = (unsigned)(((long)n * p.in1_ns + pix + (long)kk * 8 * HW) * 4);
#pragma unroll
        for (int i = 0; i < NU; ++i)
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int ch0 = (2 * wave + 16 * i) * 8 + c;  // scalar; + 8*kk per lane (in voff)
                const int soff = (ch0 < Cin ? ch0 : 0) * HW * 4;  // kk = 1 lanes past Cin: in-bounds or zero (descriptor), masked in commit
                stg[i][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0));
            }
    };
    auto commit = [&](int buf) {
        bf16x8* dst = Bs + (long)buf * 2 * NG * TP + l31;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int g = 2 * wave + kk + 16 * i;
            bf16x8 hi, lo;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const Bf16Split sp = split_bf16<2>((sval && g * 8 + c < Cin) ? stg[i][c] : 0.f);
                hi[c] = sp.hi;
                lo[c] = sp.mid;
            }
            dst[(0 * NG + g) * TP] = hi;
            dst[(1 * NG + g) * TP] = lo;
        }
    };

    int tile = blockIdx.x, buf = 0;
    prefetch(tile);
    for (; tile < n_tiles; tile += gridDim.x, buf ^= 1) {
        commit(buf);
        prefetch(tile + gridDim.x);         // unconditional (clamped): in flight during the MFMAs and stores below
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        const bf16x8* bb = Bs + (long)buf * 2 * NG * TP + kk * TP + l31;
        f32x16 acc[1][1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            const bf16x8 bh = bb[(0 * NG + 2 * s) * TP];
            const bf16x8 bl = bb[(1 * NG + 2 * s) * TP];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[s], bh, acc[0][0], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], bl, acc[0][0], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], bh, acc[0][0], 0, 0, 0);
        }
        int pn[1], ppix[1];
        bool pvalid[1];
        const long q = (long)tile * TP + l31;
        pvalid[0] = q < total;
        split_q(pvalid[0] ? q : 0, pn[0], ppix[0]);
        conv_epilogue<1, 1, 256>(p, acc, ep, co_base, wave, kk, HW, pn, ppix, pvalid, psum, false);
    }
    if (p.ep_mode == 4) {  // the workgroup's partial sums: one atomic per (sum, channel)
        __syncthreads();
        for (int c = tid; c < 512; c += 512)  // psum is [256][2]; part rows are [2][Cout]
            atomicAdd(&p.part[(long)(c & 1) * p.Cout + blockIdx.y * 256 + (c >> 1)], psum[c]);
    }
}


// ------------------------------------------------------------------------------------------------ weight-stationary 3x3
// The coupling net's FIRST convolution at the shallow levels (z1 | condition -> Hd: 18 -> 256 on 622 592 pixels at level
// 0): K = 9 * Cin is tiny, the output (637 MB) is everything.  The generic kernel pads every tap to 16-channel chunks
// (18 -> 32: 44 % wasted MFMAs), re-stages a weight chunk per 128 pixels and runs four cout blocks per pixel tile.
// Here the K dimension is the dense list of (tap, 8-channel unit) pairs (27 units for Cin <= 24), the 256 x K weights
// live in registers (8 waves x 32 output channels), and one persistent workgroup per CU walks 32-pixel tiles whose
// haloed input image (<= 102 positions x NG units) is double-buffered in LDS.
template <int NG, int PT, bool FASTEP = true>
__global__ __launch_bounds__(512) void conv3x3_ws_kernel(const ConvParams p, const int n_tiles, const int tw_shift,
                                                         const int tpf_shift, const int wt_shift) {
    constexpr int NU = 9 * NG, NSTEPS = (NU + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int TW = 1 << tw_shift, TH = (32 * PT) >> tw_shift;  // PT independent 32-pixel accumulator tiles per step
    const int IMGW = TW + 2, IMG = IMGW * (TH + 2);
    const int IMGP = (IMG + 3) & ~3;
    bf16x8* Bs = reinterpret_cast<bf16x8*>(lds_raw);                        // [2 buffers][plane][NG][IMGP]
    float* ep = reinterpret_cast<float*>(Bs + 2 * 2 * NG * IMGP);           // [2][256]
    float* psum = ep + 2 * 256;                                             // [256][2] running sums of ep_mode 4
    for (int c = threadIdx.x; c < 512; c += 512) psum[c] = 0.f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int HW = p.H * p.W, Cin = p.C1 + p.C2;
    const int co_base = blockIdx.y * 256 + wave * 32;

    // weights -> registers: k-step s covers units 2s (lanes 0-31) and 2s+1 (lanes 32-63); unit u = (tap u / NG, group
    // u % NG) sits in the packed buffer at (((c16*9 + tap)*2 + plane)*2 + g)*CoutP + co with c16 = group/2, g = group%2
    bf16x8 wh[NSTEPS], wl[NSTEPS];
    {
        const bf16x8* wp = reinterpret_cast<const bf16x8*>(p.wpk) + co_base + l31;
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            const int u = 2 * s + kk;
            const bool ok = u < NU && (u % NG) / 2 < p.Cin8;
            const int uc = ok ? u : 0;
            const int tap = uc / NG, grp = uc % NG;
            const long base = (long)(((grp / 2) * 9 + tap) * 2) * 2 + (grp & 1);
            const bf16x8 h = wp[(base + 0) * p.CoutP];
            const bf16x8 l = wp[(base + 2) * p.CoutP];
            wh[s] = ok ? h : z;
            wl[s] = ok ? l : z;
        }
    }
    load_epilogue_params<256, 512>(p, ep);

    // staging role: one (unit, image position) pair per thread (NG * IMG <= 512)
    const bool srole = tid < NG * IMG;
    const int sg = srole ? tid / IMG : 0, spos = srole ? tid - sg * IMG : 0;
    const int syy = spos / IMGW, sxx = spos - syy * IMGW;
    float stg[8];
    bool sval = false;
    auto tile_origin = [&](int tile, int& n, int& y0, int& x0) {
        n = tile >> tpf_shift;
        const int r = tile & ((1 << tpf_shift) - 1);
        y0 = (r >> wt_shift) * TH;
        x0 = (r & ((1 << wt_shift) - 1)) * TW;
    };
    auto prefetch = [&](int tile) {
        int n, y0, x0;
        tile_origin(tile < n_tiles ? tile : 0, n, y0, x0);
        const int gy = y0 + syy - 1, gx = x0 + sxx - 1;
        sval = srole && tile < n_tiles && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        const long off = sval ? (long)gy * p.W + gx : 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ch = sg * 8 + c;
            const int chc = ch < Cin ? ch : 0;
            const float* src = chc < p.C1 ? p.in1 + (long)n * p.in1_ns + (long)chc * HW
                                          : p.in2 + (long)n * p.in2_ns + (long)(chc - p.C1) * HW;
            stg[c] = src[off];
        }
    };
    auto commit = [&](int buf) {
        if (!srole) return;
        bf16x8 hi, lo;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const Bf16Split sp = split_bf16<2>((sval && sg * 8 + c < Cin) ? stg[c] : 0.f);
            hi[c] = sp.hi;
            lo[c] = sp.mid;
        }
        bf16x8* dst = Bs + (long)buf * 2 * NG * IMGP + spos;
        dst[(0 * NG + sg) * IMGP] = hi;
        dst[(1 * NG + sg) * IMGP] = lo;
    };

    // this lane's pixels inside the tile and their image positions (centre tap)
    int pcol[PT], prow[PT], pbase[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const int px = t * 32 + l31;
        pcol[t] = px & (TW - 1);
        prow[t] = px >> tw_shift;
        pbase[t] = (prow[t] + 1) * IMGW + pcol[t] + 1;
    }
    int tile = blockIdx.x, buf = 0;
    prefetch(tile);
    for (; tile < n_tiles; tile += gridDim.x, buf ^= 1) {
        commit(buf);
        prefetch(tile + gridDim.x);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        const bf16x8* bb = Bs + (long)buf * 2 * NG * IMGP;
        f32x16 acc[1][PT];
#pragma unroll
        for (int t = 0; t < PT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][t][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            // compile-time unit pair of this k-step; the padding unit past 9*NG reads unit 0 (its weights are zero)
            const int uA = 2 * s, uB = (2 * s + 1 < NU) ? 2 * s + 1 : 0;
            const int offA = (uA % NG) * IMGP + (uA / NG / 3 - 1) * IMGW + (uA / NG % 3 - 1);
            const int offB = (uB % NG) * IMGP + (uB / NG / 3 - 1) * IMGW + (uB / NG % 3 - 1);
            const int off = kk ? offB : offA;
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                const bf16x8 bh = bb[pbase[t] + off];
                const bf16x8 bl = bb[NG * IMGP + pbase[t] + off];
                acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[s], bh, acc[0][t], 0, 0, 0);
                acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], bl, acc[0][t], 0, 0, 0);
                acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], bh, acc[0][t], 0, 0, 0);
            }
        }
        int n, y0, x0;
        tile_origin(tile, n, y0, x0);
        int pn[PT], ppix[PT];
        bool pvalid[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            pn[t] = n;
            ppix[t] = (y0 + prow[t]) * p.W + x0 + pcol[t];
            pvalid[t] = true;
        }
        conv_epilogue<1, PT, 256, FASTEP>(p, acc, ep, co_base, wave, kk, HW, pn, ppix, pvalid, psum, false);
    }
    if (!FASTEP && p.ep_mode == 4) {  // the workgroup's partial sums: one atomic per (sum, channel)
        __syncthreads();
        for (int c = tid; c < 512; c += 512)  // psum is [256][2]; part rows are [2][Cout]
            atomicAdd(&p.part[(long)(c & 1) * p.Cout + blockIdx.y * 256 + (c >> 1)], psum[c]);
    }
}

template <int NG, int PT, bool FASTEP = true>
static int launch_conv3x3_ws_t(ConvParams& p, hipStream_t s) {
    const int TW = p.W < 32 ? p.W : 32, TH = 32 * PT / TW;
    const int tw_shift = ilog2(TW);
    const int wt = p.W / TW, ht = p.H / TH;  // tiles per row / column of a frame
    const int wt_shift = ilog2(wt), tpf_shift = ilog2(wt * ht);
    const int n_tiles = p.N * wt * ht;
    const int IMG = (TW + 2) * (TH + 2), IMGP = (IMG + 3) & ~3;
    if (NG * IMG > 512) {
        rfn_set_error("conv3x3_ws: %d staging items", NG * IMG);
        return -8;
    }
    p.ksplit = 1;
    const size_t lds = (size_t)2 * 2 * NG * IMGP * 16 + 4 * 256 * 4;
    auto kern = conv3x3_ws_kernel<NG, PT, FASTEP>;
    dim3 grid(n_tiles < 256 ? n_tiles : 256, p.Cout / 256);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p, n_tiles, tw_shift, tpf_shift, wt_shift);
    return 0;
}

static int launch_conv1x1_ws(ConvParams& p, hipStream_t s) {
    const int HW = p.H * p.W;
    const long total = (long)p.N * HW;
    const int n_tiles = (int)((total + 31) / 32);
    int hw_shift = -1;
    if ((HW & (HW - 1)) == 0) hw_shift = ilog2(HW);
    p.ksplit = 1;
    const size_t lds = (size_t)2 * 2 * 32 * 32 * 16 + 4 * 256 * 4;
    auto kern = conv1x1_ws_kernel<16>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    dim3 grid(n_tiles < 256 ? n_tiles : 256, p.Cout / 256);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p, n_tiles, hw_shift);
    return 0;
}

// the generic tile kernel on two (bf16x3) or three (bf16x6) planes per operand
template <int KS, int WCO, int WPX, int TCO, int TPX, int KC>
static int launch_conv_b3_npl(ConvParams& p, hipStream_t s) {
    return p.npl == 3 ? launch_conv_b3<KS, WCO, WPX, TCO, TPX, KC, 3>(p, s) : launch_conv_b3<KS, WCO, WPX, TCO, TPX, KC>(p, s);
}

static int dispatch_conv_b3(ConvParams& p, int ks, hipStream_t s) {
    switch (choose_conv_b3(p, ks)) {
        case G3_32x128:  return launch_conv_b3_npl<3, 1, 4, 1, 1, 16>(p, s);
        case G3_64x64:   return launch_conv_b3_npl<3, 2, 2, 1, 1, 16>(p, s);
        case G3_64x128:  return launch_conv_b3_npl<3, 2, 2, 1, 2, 16>(p, s);
        case G1_32x128:  return launch_conv_b3_npl<1, 1, 4, 1, 1, 32>(p, s);
        case G1_64x64:   return launch_conv_b3_npl<1, 2, 2, 1, 1, 32>(p, s);
        case G1_128x128: return launch_conv_b3_npl<1, 2, 2, 2, 2, 32>(p, s);
        case G1_256x64:  return launch_conv_b3_npl<1, 4, 1, 2, 2, 32>(p, s);
        case WS1:        return launch_conv1x1_ws(p, s);
        case WS3_ACTBWD: return launch_conv3x3_ws_t<1, 2, false>(p, s);
        case WS3_27:     return launch_conv3x3_ws_t<3, 2>(p, s);
        case WS3_45:     return launch_conv3x3_ws_t<5, 1>(p, s);
    }
    return -9;
}
