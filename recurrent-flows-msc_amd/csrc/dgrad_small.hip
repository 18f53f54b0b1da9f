// 3x3 convolution with FEW output channels and many input channels on 32x32 / 16x16 / 8x8 maps, bf16x3 arithmetic:
// the data gradient of the first coupling-net convolution at the three finest flow levels (256 -> 18 / 36 / 72
// channels, Flow/glow_modules.py:232-238 backwards).
//
// The three x-taps are ROWS of one MFMA product, not three products at shifted positions.  With
//   E_dx[co][y][x'] = sum_c sum_dy w'[co][c][dy][dx] * in[c][y + dy][x']          (dx = -1, 0, +1)
// the result is out[co][y][x] = sum_dx E_dx[co][y][x + dx], E_dx taken as zero outside [0, W).  The GEMM is
// D[(dx, co)][pixel], K = (input-channel chunk of 16) x (3 y-taps): 3 x CP4 rows (CP4 = Cout rounded up to 4, so that a
// register quad of the accumulator belongs to one dx) instead of 9 products of 32-row tiles that are half empty.
//   * a block owns BPIX = 32 x TPX x PG pixels: a band of whole rows of one frame (W = 32) or 1 / 2 whole frames
//     (W = 16 / 8).  Its 4 waves are PG pixel groups x RS row groups: a wave owns TPX tiles of 32 pixels (1 / 2 / 4 image
//     rows) and MTW of the MTW x RS row tiles;
//   * per 16-channel chunk the band with its two halo ROWS (no halo columns: every fragment is the unshifted input) is
//     staged in LDS pre-split into bf16 hi / lo as [plane][8-channel group][position][8 x bf16]; an MFMA B fragment is one
//     ds_read_b128 of 32 consecutive positions, and the fragment of input row i serves the output rows i-1, i, i+1;
//   * staging issues only what it loads: the body is BPIX / 64 dwordx4 loads per thread (CPI channels x 4 pixels, all 256
//     threads live), the two halo rows of a band are one single-channel dwordx4 per thread written in 16-bit pieces; whole
//     frames have no halo to load (the rows outside the frame are zeroed once);
//   * the weights of a chunk (3 y-taps x row tiles, hi and lo) arrive by LDS-DMA straight from the pack buffer the
//     generic kernel uses (rfn_pack_conv_weight_bf16x3 layout): lane row R -> (dx, co) picks its own pack unit, padding
//     rows read a row in [Cout, CoutP) that the pack kernel wrote as zeros;
//   * three-stage software pipeline over the chunks: MFMAs of chunk c | split + LDS write of chunk c+1 | loads of chunk
//     c+2, the writes ahead of the loads inside a chunk (see the chunk loop);
//   * epilogue, once per block: the accumulators pass through the then idle LDS as E[row][pixel]; a lane gathers
//     E_-1[x-1] + E_0[x] + E_+1[x+1] for four pixels of one channel (zero, not the neighbouring row's value, beyond
//     the row ends) and reads / writes the outputs as dwordx4.
// Registers (VGPR + AGPR of the unified file, tools/kernel_resources.py; ScratchSize 0 for every instantiation; one wave
// per SIMD, so up to 512 are there): <32,2,4,1> 256+12, <32,2,4,2> 256+9, <32,3,4,2> 256+204, <16,2,2,1> 182,
// <16,4,2,1> 256+48, <16,3,4,2> 256+216, <8,4,1,1> 228, <8,7,1,1> 256+138, <8,4,1,2> 256+1, <8,5,1,2> 256+60.  hipcc
// keeps the first 256 as VGPRs and the rest as AGPRs: <8,7,1,1> (level 2) has 124 VGPRs spilled to AGPRs, and it,
// <16,4,2,1> and <32,3,4,2> carry v_accvgpr_read / _write copies inside the chunk loop (extra VALU issue); <8,4,1,2> /
// <8,5,1,2> / <8,7,1,1> spill 11 / 20 / 4 SGPRs to VGPR lanes.  The cause is A[3][MTW][2], held for a whole chunk (168
// registers at MTW = 7); loading it per dy would shorten those live ranges (not done).
// Order of the vector-memory operations (tools/check_dgrad_dma_order.py reads it off the compiled ISA of all ten
// instantiations): in every chunk all weight-DMA pieces are issued before the first image load, and the vmcnt
// immediate in front of the chunk barrier equals the number of image loads issued after the last DMA piece.
#include "conv_common.h"
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct DgradSmallParams {
    const float* in;   // [N, Cin, H, W] (frame stride in_ns)
    long in_ns;
    const unsigned char* wpk;  // rfn_pack_conv_weight_bf16x3 buffer of the [Cout][Cin][3][3] logical weight
    float* out1;
    float* out2;
    long out1_ns, out2_ns;
    int Cin, Cout, cout_split, acc1, acc2, CoutP;
    int N, H;
    int CP4;  // rows per dx block: Cout rounded up to a multiple of 4
    int vec;  // outputs are 16-byte aligned with frame strides % 4 == 0: dwordx4 epilogue
};

#define DS_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0)

// CPI consecutive bf16 values -> LDS
template <int CPI>
__device__ __forceinline__ void ds_store_bf16(unsigned char* dst, const __bf16 (&v)[CPI]) {
    if constexpr (CPI == 8) {
        *reinterpret_cast<bf16x8*>(dst) = bf16x8{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    } else if constexpr (CPI == 4) {
        *reinterpret_cast<bf16x4*>(dst) = bf16x4{v[0], v[1], v[2], v[3]};
    } else if constexpr (CPI == 2) {
        *reinterpret_cast<bf16x2*>(dst) = bf16x2{v[0], v[1]};
    } else {
        *reinterpret_cast<__bf16*>(dst) = v[0];
    }
}

template <int W, int MTW, int TPX, int RS>
struct DgradSmallCfg {
    static constexpr int PG = 4 / RS;                  // waves along the pixel axis
    static constexpr int MTT = MTW * RS;               // row tiles of the block
    static constexpr int RPT = 32 / W;                 // image rows per 32-pixel tile
    static constexpr int R = TPX * RPT;                // image rows per wave
    static constexpr int BPIX = PG * TPX * 32;         // body pixels per block
    static constexpr bool BAND = BPIX < W * W;         // a block is a band of rows of one frame (else whole frames)
    static constexpr int FPB = BAND ? 1 : BPIX / (W * W);  // frames per block
    static constexpr int PF = BPIX / FPB;              // body pixels per frame
    static constexpr int BR = PF / W;                  // body rows per frame
    static constexpr int IPOSF = (BR + 2) * W, IPOS = FPB * IPOSF;  // staged positions (halo rows included)
    static constexpr int IMG_BYTES = 2 * 2 * IPOS * 16;            // [plane][group][pos] x 16 B
    static constexpr int WFR = 3 * 2 * MTT;                         // 1-KB weight fragments per chunk: [dy][plane][mt]
    static constexpr int WGT_BYTES = WFR * 1024;
    static constexpr int CPI = BPIX / 64;              // channels per body staging item (x 4 pixels): 256 items per chunk
    static constexpr int NQ = BPIX / 4;                // pixel quads of the body
    static constexpr int NLD = CPI + (BAND ? 1 : 0);   // dwordx4 loads per thread and chunk
    static constexpr int NFI = R + 2 - (RPT - 1);      // distinct input fragment rows per wave: i = -1 .. R - RPT + 1
    static constexpr int ESTR = 36;                    // floats per row of the epilogue's E[row][pixel]
    static constexpr int EPI_BYTES = PG * MTT * 32 * ESTR * 4;
    static constexpr int LOOP_BYTES = 2 * IMG_BYTES + 2 * WGT_BYTES;
    static constexpr int LDS_BYTES = LOOP_BYTES > EPI_BYTES ? LOOP_BYTES : EPI_BYTES;
    static_assert(RS == 1 || RS == 2, "row groups");
    static_assert(CPI == 1 || CPI == 2 || CPI == 4 || CPI == 8, "body item shape");
    static_assert(!BAND || W == 32, "bands (halo rows to load) only at W = 32: 2 rows x 16 channels x 8 quads = 256 items");
    static_assert(PF % (TPX * 32) == 0, "a wave's tiles lie in one frame");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

template <int W, int MTW, int TPX, int RS>
__global__ __launch_bounds__(256) void dgrad_small_kernel(const DgradSmallParams p) {
    using C = DgradSmallCfg<W, MTW, TPX, RS>;
    constexpr int PG = C::PG, MTT = C::MTT, RPT = C::RPT, BPIX = C::BPIX, FPB = C::FPB, PF = C::PF, BR = C::BR;
    constexpr int IPOSF = C::IPOSF, IPOS = C::IPOS, IMG_BYTES = C::IMG_BYTES, WFR = C::WFR, WGT_BYTES = C::WGT_BYTES;
    constexpr int CPI = C::CPI, NQ = C::NQ, NLD = C::NLD, NFI = C::NFI, ESTR = C::ESTR;
    constexpr bool BAND = C::BAND;
    constexpr int NJ = (WFR + 3) / 4;  // weight fragments per wave and chunk
    constexpr unsigned MASKED = 0xFFFFFF00u;
    (void)BPIX; (void)PG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // lds: image[2] | weights[2]; the epilogue reuses all of it
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = wave / RS, rs = wave - pg * RS;
    const int l31 = lane & 31, kk = lane >> 5;
    const int HW = p.H * W;
    int n0, rb;  // first frame and first image row of the block
    if (BAND) {
        const int bands = p.H / BR;
        n0 = blockIdx.x / bands;
        rb = (blockIdx.x - n0 * bands) * BR;
    } else {
        n0 = blockIdx.x * FPB;
        rb = 0;
    }
    const int nchunks = p.Cin >> 4;
    // bounds-checked buffer over the whole input (descriptor from kernel arguments only: wave-uniform by construction);
    // masked lanes point past the end and read zeros.  The host guarantees N * in_ns * 4 < 0xFFFFFF00.
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0,
                                                         (unsigned)((long)p.N * p.in_ns * 4), 0x00020000);

    // ---- staging items of this thread.  Body: CPI channels x 4 pixels arrive as CPI dwordx4 loads and leave as 4 (hi, lo)
    // pairs of CPI x 2 bytes.  Halo (bands only): one channel x 4 pixels of the row above / below the band.
    unsigned b_off, h_off = MASKED;  // byte offsets inside the input of chunk 0 (MASKED: reads zeros)
    int b_dst, h_dst = 0;            // LDS byte offsets inside an image buffer (hi plane) of the first pixel
    {
        const int cg = tid / NQ, pq = tid - cg * NQ;
        const int f = (pq * 4) / PF, pin = pq * 4 - f * PF;
        const int cl = cg * CPI;
        const bool ok = n0 + f < p.N;
        b_off = ok ? (unsigned)((long)(n0 + f) * p.in_ns * 4) + (unsigned)((cl * HW + rb * W + pin) * 4) : MASKED;
        b_dst = ((cl >> 3) * IPOS + f * IPOSF + W + pin) * 16 + (cl & 7) * 2;
        if (BAND) {
            const int ch = tid >> 4, hr = (tid >> 3) & 1, q = tid & 7;
            const int gy = hr ? rb + BR : rb - 1;
            h_off = (gy >= 0 && gy < p.H) ? (unsigned)((long)n0 * p.in_ns * 4) + (unsigned)((ch * HW + gy * W + 4 * q) * 4)
                                          : MASKED;
            h_dst = ((ch >> 3) * IPOS + (hr ? (BR + 1) * W : 0) + 4 * q) * 16 + (ch & 7) * 2;
        }
    }
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
    // load j of chunk c: channel j of the body item, j == CPI: the halo item
    auto img_load1 = [&](f32x4 (&raw)[NLD], const int c, const int j) {
        const unsigned base = j < CPI ? b_off : h_off;
        const unsigned off = base == MASKED ? MASKED : base + (unsigned)((c * 16 + (j < CPI ? j : 0)) * HW * 4);
        const u32x4_ v = __builtin_amdgcn_raw_buffer_load_b128(rs_in, off, 0, 0);
        raw[j] = __builtin_bit_cast(f32x4, v);
    };
    // pixel e of this thread's items: split into bf16 hi / lo
    auto img_store1 = [&](const f32x4 (&raw)[NLD], const int buf, const int e) {
        unsigned char* img = lds + buf * IMG_BYTES + e * 16;
        __bf16 hi[CPI], lo[CPI];
#pragma unroll
        for (int j = 0; j < CPI; ++j) {
            const float v = raw[j][e];
            hi[j] = (__bf16)v;
            lo[j] = (__bf16)(v - (float)hi[j]);
        }
        ds_store_bf16<CPI>(img + b_dst, hi);
        ds_store_bf16<CPI>(img + b_dst + 2 * IPOS * 16, lo);
        if (BAND) {
            const float v = raw[NLD - 1][e];
            const __bf16 h = (__bf16)v;
            *reinterpret_cast<__bf16*>(img + h_dst) = h;
            *reinterpret_cast<__bf16*>(img + h_dst + 2 * IPOS * 16) = (__bf16)(v - (float)h);
        }
    };
    // weights of chunk c -> LDS buffer `buf`: fragment f = (dy*2 + plane)*MTT + mt holds rows mt*32 .. +31 of the stacked
    // (dx, co) rows; lane (row, kk) reads the pack unit (((c*9 + dy*3 + dx)*2 + plane)*2 + kk)*CoutP + co.  Wave w moves
    // the fragments w, w + 4, ...: their lane offsets inside a chunk are fixed.  Every wave issues NJ pieces (past the end
    // the last fragment once more, same bytes to the same place): no wave-dependent branch around a DMA piece.
    unsigned w_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = min(wave + 4 * j, WFR - 1);
        const int tp = f / MTT, mt = f - tp * MTT;  // tp = dy*2 + plane
        const int dy = tp >> 1, pl = tp & 1;
        const int row = mt * 32 + l31;
        int dx = (row >= p.CP4) + (row >= 2 * p.CP4);
        int co = row - dx * p.CP4;
        if (co >= p.Cout) {  // padding row: a zero row of the pack
            dx = 0;
            co = p.Cout;
        }
        w_off[j] = (unsigned)((((dy * 3 + dx) * 2 + pl) * 2 + kk) * p.CoutP + co) * 16u;
    }
    const unsigned w_cstride = 36u * (unsigned)p.CoutP * 16u;
    auto wgt_dma = [&](const int c, const int buf) {
        unsigned char* dst0 = lds + 2 * IMG_BYTES + buf * WGT_BYTES;
        const unsigned char* src0 = p.wpk + (size_t)c * w_cstride;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int f = min(wave + 4 * j, WFR - 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src0 + w_off[j]),
                                             (__attribute__((address_space(3))) void*)(dst0 + f * 1024), 16, 0, 0);
        }
    };
    {   // zero both image buffers once (whole frames: the rows above / below the frame stay zero)
        f32x4* z4 = reinterpret_cast<f32x4*>(lds);
        for (int i = tid; i < 2 * IMG_BYTES / 16; i += 256) z4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
    }

    f32x16 acc[TPX][MTW];
#pragma unroll
    for (int t = 0; t < TPX; ++t)
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][m][r] = 0.f;

    // this lane's position of input fragment row i = -1 inside the staged image: pixel l31 of the wave's first tile, one
    // image row up (staged row 0 of a frame is its halo row)
    const int wp0 = pg * TPX * 32;  // the wave's first body pixel
    const int wf = wp0 / PF;        // its frame inside the block
    const int pos0 = wf * IPOSF + (wp0 - wf * PF) + l31;

    // ---- three-stage pipeline over the 16-channel chunks: while the MFMAs of chunk c run, the registers loaded during
    // chunk c-1 (chunk c+1's image) are split and written to the other LDS buffer, and chunk c+2 is being loaded.
    f32x4 rawA[NLD], rawB[NLD];
    wgt_dma(0, 0);
#pragma unroll
    for (int j = 0; j < NLD; ++j) img_load1(rawA, 0, j);
#pragma unroll
    for (int j = 0; j < NLD; ++j) img_load1(rawB, 1, j);
#pragma unroll
    for (int e = 0; e < 4; ++e) img_store1(rawA, 0, e);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();

    // one chunk: rawC holds chunk c+1 (to be stored into the other buffer), rawN receives chunk c+2
    auto chunk = [&](auto st_, auto ld_, const int c, f32x4 (&rawC)[NLD], f32x4 (&rawN)[NLD]) {
        constexpr bool st = decltype(st_)::value, ld = decltype(ld_)::value;  // is there a chunk c+1 / c+2
        const int buf = c & 1;
        const bf16x8* img = reinterpret_cast<const bf16x8*>(lds + buf * IMG_BYTES) + kk * IPOS + pos0;
        const bf16x8* wl = reinterpret_cast<const bf16x8*>(lds + 2 * IMG_BYTES + buf * WGT_BYTES) + rs * MTW * 64 + lane;
        bf16x8 A[3][MTW][2];  // [dy][mt][plane]
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) A[dy][m][pl] = wl[((dy * 2 + pl) * MTT + m) * 64];
        bf16x8 B[2][2];
        B[0][0] = img[0];
        B[0][1] = img[2 * IPOS];
#pragma unroll
        for (int fi = 0; fi < NFI; ++fi) {  // input fragment first row i = fi - 1 (relative to the wave's rows)
            const int cur = fi & 1;
            if (fi + 1 < NFI) {
                B[cur ^ 1][0] = img[(fi + 1) * W];
                B[cur ^ 1][1] = img[2 * IPOS + (fi + 1) * W];
            }
            __builtin_amdgcn_sched_barrier(0);
            // the (up to) 3 x MTW accumulators this fragment feeds take turns: no back-to-back dependent MFMAs
#pragma unroll
            for (int combo = 0; combo < 3; ++combo) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int ro = (fi - 1) - (dy - 1);  // output tile's first row
                    if (ro >= 0 && ro <= (TPX - 1) * RPT && ro % RPT == 0) {
#pragma unroll
                        for (int m = 0; m < MTW; ++m) {
                            if (combo == 0) DS_MFMA(acc[ro / RPT][m], A[dy][m][1], B[cur][0]);
                            if (combo == 1) DS_MFMA(acc[ro / RPT][m], A[dy][m][0], B[cur][1]);
                            if (combo == 2) DS_MFMA(acc[ro / RPT][m], A[dy][m][0], B[cur][0]);
                        }
                    }
                }
            }
            // staging in the shadow of those MFMAs, in the first steps of the chunk: FIRST the pixels of chunk c+1 (split
            // + LDS write), THEN the weight DMA of chunk c+1, THEN the loads of chunk c+2 (into the other register set).
            // hipcc puts an s_waitcnt vmcnt(0) in front of the first split; what it waits for are the loads that the
            // previous chunk's vmcnt(NLD) left outstanding, issued most of a chunk ago, and nothing younger.
            constexpr int SS = NFI / 3 > 0 ? NFI / 3 : 1;  // steps that store / steps that load
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (st && (k * SS) / 4 == fi) img_store1(rawC, buf ^ 1, k);
            if (st && fi == SS) {
                // the DMA pieces in a scheduling region of their own: every one of them is issued before the first load
                // of chunk c+2, which is what the vmcnt(NLD) below counts on (without the fences hipcc interleaved them)
                __builtin_amdgcn_sched_barrier(0);
                wgt_dma(c + 1, buf ^ 1);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int k = 0; k < NLD; ++k)
                if (ld && SS + (k * SS) / NLD == fi) img_load1(rawN, c + 2, k);
            __builtin_amdgcn_sched_barrier(0);
        }
        // vector-memory operations complete in issue order: with at most the NLD loads of chunk c+2 in flight, every DMA
        // piece of chunk c+1 (issued before them, see above) has landed in LDS
        if (ld) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    {   // (nchunks is even: the host requires Cin % 32 == 0)
        using T_ = std::integral_constant<bool, true>;
        using F_ = std::integral_constant<bool, false>;
        int c = 0;
        for (; c + 3 < nchunks; c += 2) {
            chunk(T_{}, T_{}, c, rawB, rawA);
            chunk(T_{}, T_{}, c + 1, rawA, rawB);
        }
        chunk(T_{}, F_{}, c, rawB, rawA);
        chunk(F_{}, F_{}, c + 1, rawA, rawB);
    }

    // ---- epilogue.  D layout: col = lane & 31 (pixel), row = (r & 3) + 8 (r >> 2) + 4 kk.  Tile by tile the block's
    // accumulators go to E[pixel group][row][ESTR] in LDS; then the RS waves of a pixel group share its (channel, pixel
    // quad) items: out[co][x .. x+3] = E[co][x-1 .. x+2] + E[CP4 + co][x .. x+3] + E[2 CP4 + co][x+1 .. x+4], where the
    // elements left of x = 0 and right of x = W-1 (the neighbouring image row, frame or padding) count as zero.
    float* E = reinterpret_cast<float*>(lds) + pg * (MTT * 32 * ESTR);
#pragma unroll
    for (int t = 0; t < TPX; ++t) {
        if (t > 0) __syncthreads();  // the previous tile's reads are done (t = 0: the loop's last barrier)
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                E[((rs * MTW + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk) * ESTR + l31] = acc[t][m][r];
        __syncthreads();
        const int wp = wp0 + t * 32;
        const int n = n0 + wf;
        if (n < p.N) {
            const int pix0 = rb * W + (wp - wf * PF);
            for (int idx = rs * 64 + lane; idx < p.Cout * 8; idx += RS * 64) {
                const int co = idx >> 3, q = idx & 7;
                const int x0 = (4 * q) & (W - 1);
                const bool hasL = x0 != 0, hasR = x0 + 4 != W;
                const float* e0 = E + co * ESTR + 4 * q;
                const float* e1 = e0 + p.CP4 * ESTR;
                const float* e2 = e1 + p.CP4 * ESTR;
                const f32x4 a = *reinterpret_cast<const f32x4*>(e0);
                const f32x4 b = *reinterpret_cast<const f32x4*>(e1);
                const f32x4 cc = *reinterpret_cast<const f32x4*>(e2);
                float aL = e0[hasL ? -1 : 0], cR = e2[hasR ? 4 : 0];
                aL = hasL ? aL : 0.f;
                cR = hasR ? cR : 0.f;
                f32x4 o;
                o[0] = aL + b[0] + cc[1];
                o[1] = a[0] + b[1] + cc[2];
                o[2] = a[1] + b[2] + cc[3];
                o[3] = a[2] + b[3] + cR;
                const bool first = co < p.cout_split;
                float* dst = first ? p.out1 + n * p.out1_ns + (long)co * HW + pix0 + 4 * q
                                   : p.out2 + n * p.out2_ns + (long)(co - p.cout_split) * HW + pix0 + 4 * q;
                const bool accm = first ? p.acc1 : p.acc2;
                if (p.vec) {
                    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
                    if (accm) o += *d4;
                    *d4 = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[e] = accm ? o[e] + dst[e] : o[e];
                }
            }
        }
    }
}

template <int W, int MTW, int TPX, int RS>
static int launch_dgrad_small(const DgradSmallParams& p, hipStream_t st) {
    using C = DgradSmallCfg<W, MTW, TPX, RS>;
    constexpr size_t lds = C::LDS_BYTES;
    auto* k = dgrad_small_kernel<W, MTW, TPX, RS>;
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int blocks = C::BAND ? p.N * (p.H / C::BR) : (p.N + C::FPB - 1) / C::FPB;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, st, p);
    return 0;
}

// Cout <= 64 on 32x32 / 16x16 maps, Cout <= 96 on 8x8 maps (3 x Cout stacked rows x the block's pixel tiles must fit
// the register file), Cin % 32 == 0, square maps, the input inside the 32-bit buffer range.
extern "C" int rfn_dgrad_small_supported(int N, int Cin, int Cout, int H, int W) {
    if (N <= 0 || Cin <= 0 || (Cin & 31) || Cout <= 0 || H != W) return 0;
    if ((long)N * Cin * H * W * 4 >= 0xFFFFFF00L) return 0;  // 32-bit buffer offsets
    if (W == 32 || W == 16) return Cout <= 64;
    if (W == 8) return Cout <= 96;
    return 0;
}

// out[n, co, y, x] = sum_ci sum_tap in[n, ci, y+dy, x+dx] * w'[co][ci][tap] with w' the logical weight the pack buffer was
// built from (mode 1 of the pack kernel = data gradient of a forward weight); output channels [0, cout_split) go to out1,
// the rest to out2; acc1 / acc2: add into the existing values.
extern "C" int rfn_conv3x3_smallcout_bf16x3(const float* in, long in_ns, int Cin, const float* wpk, float* out1,
                                            long out1_ns, float* out2, long out2_ns, int Cout, int cout_split, int acc1,
                                            int acc2, int N, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(in && wpk && out1 && N >= 0, -1);
    RFN_CHECK_ARG(rfn_dgrad_small_supported(N > 0 ? N : 1, Cin, Cout, H, W), -2);
    RFN_CHECK_ARG(cout_split > 0 && cout_split <= Cout && (cout_split == Cout || out2), -3);
    RFN_CHECK_ARG(((uintptr_t)wpk & 15) == 0 && ((uintptr_t)in & 15) == 0 && (in_ns & 3) == 0, -4);
    RFN_CHECK_ARG((long)N * in_ns * 4 < 0xFFFFFF00L && in_ns >= (long)Cin * H * W, -5);
    if (N == 0) return 0;
    DgradSmallParams p;
    p.in = in; p.in_ns = in_ns; p.wpk = reinterpret_cast<const unsigned char*>(wpk);
    p.out1 = out1; p.out2 = out2; p.out1_ns = out1_ns; p.out2_ns = out2_ns;
    p.Cin = Cin; p.Cout = Cout; p.cout_split = cout_split; p.acc1 = acc1; p.acc2 = acc2;
    p.CoutP = ((Cout + 255) / 256) * 256;
    p.N = N; p.H = H;
    p.CP4 = (Cout + 3) & ~3;
    p.vec = ((uintptr_t)out1 & 15) == 0 && (out1_ns & 3) == 0 &&
            (cout_split == Cout || (((uintptr_t)out2 & 15) == 0 && (out2_ns & 3) == 0));
    hipStream_t st = (hipStream_t)stream;
    const int MTR = (3 * p.CP4 + 31) / 32;  // row tiles of the stacked (dx, co) rows
    if (W == 32) {         // bands of 16 rows (4 waves x 4 tiles) or, with two row groups, of 8 rows
        if (MTR <= 2) launch_dgrad_small<32, 2, 4, 1>(p, st);
        else if (MTR <= 4) launch_dgrad_small<32, 2, 4, 2>(p, st);
        else launch_dgrad_small<32, 3, 4, 2>(p, st);
    } else if (W == 16) {  // one frame per block
        if (MTR <= 2) launch_dgrad_small<16, 2, 2, 1>(p, st);
        else if (MTR <= 4) launch_dgrad_small<16, 4, 2, 1>(p, st);
        else launch_dgrad_small<16, 3, 4, 2>(p, st);
    } else {               // two frames per block, or one with two row groups
        if (MTR <= 4) launch_dgrad_small<8, 4, 1, 1>(p, st);
        else if (MTR <= 7 && N >= 512) launch_dgrad_small<8, 7, 1, 1>(p, st);
        else if (MTR <= 8) launch_dgrad_small<8, 4, 1, 2>(p, st);
        else launch_dgrad_small<8, 5, 1, 2>(p, st);
    }
    RFN_LAUNCH_CHECK();
    return 0;
}
