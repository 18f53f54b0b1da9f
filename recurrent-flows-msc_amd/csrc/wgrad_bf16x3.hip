// Weight gradients as one split-precision GEMM:  gw[m][n] += Σ_{frames, pixels} A[f][m][p] * B[f][n][p].
//
// Every split-precision weight gradient is brought to this 1x1 form; rfn_hip.ops.wgrad_plan names the forms:
//   * gemm      1x1 conv:               A = grad [M = Cout],       B = input [N = Cin]
//   * im2col    3x3 conv, Cin <= Cout:  A = grad,                  B = im2col3x3(input) [N = 9*Cin]   (rfn_im2col3x3_f32)
//   * scatter   3x3 conv, Cout <  Cin:  A = tap_scatter(grad) [M = 9*Cout] (rfn_tap_scatter_f32),     B = input
//   * implicit  3x3, Cin <= Cout, rows of a multiple of 8 pixels: no expansion in HBM, the kernel builds the shifted
//               planes of the input while staging (rfn_conv3x3_wgrad_implicit_bf16x3)
//   * mirrored  the same for the few-output conv, Cout < Cin: the gradient's planes, taps mirrored and roles swapped
//               (rfn_conv3x3_wgrad_mirrored_bf16x3)
//   * implicit_rows / mirrored_rows  the two on 4-pixel rows and 2 x 2 maps (rfn_conv3x3_wgrad_rows[_mirrored]_bf16x3)
//   * band      3x3 with few channels on BOTH sides, ungrouped: nothing expanded, nothing loaded per row -- bands of image rows of both operands
//               staged once, every tap an LDS address (wgrad_band_kernel, rfn_conv3x3_wgrad_band_bf16x3, further down)
// (its other two forms, f32 and scatter_f32, are the fp32 kernel of conv.hip).  The first three expand the SMALL operand
// in HBM, so the shifted-window reads of a 3x3 weight gradient never reach their kernel and the 8 consecutive k (pixels) an
// MFMA operand lane needs are 8 consecutive fp32 of one channel plane in NCHW: staged with 16-byte loads, split into
// bf16 hi/lo (see conv_bf16x3.hip) and stored as [row][k-group] 16-byte units with an odd row stride, so both fragment
// reads are conflict-free ds_read_b128.  K (all pixels of all frames) is split over gridDim.x; a workgroup sweeps its
// stages with register prefetch and emits float atomics once.
#include "conv_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct GemmWgradParams {
    const float* a;
    const float* b;
    long a_ns, b_ns;
    int M, N;
    float* gw;  // [M][N]
    int F, HW;  // frames, pixels per frame (HW % 4 == 0)
    long total; // F*HW
    int n_stages;
    // implicit 3x3 mode (IMPL = 1; WG_ROWS4 / WG_ROWS2 on rows shorter than 8 pixels): operand B row n = ci*9 + tap is
    // the input plane ci shifted by the tap, read straight from the convolution's (two-source) input -- b = in1,
    // b2 = in2 -- instead of from an im2col buffer in HBM
    const float* b2;
    long b2_ns;
    int C1, C2, H, W;
    // mirrored taps (implicit mode): row n = ci*9 + tap takes the plane shifted by the OPPOSITE tap, (1 - tap/3,
    // 1 - tap%3) -- the weight gradient of a convolution whose GRADIENT is the small operand B and whose input is A:
    // gw[co][ci][t] = sum_p g[co][p] in[ci][p + t] = sum_q in[ci][q] g[co][q - t], stored [Cin][Cout * 9]
    int mirror;
    // grouped launch (G > 0): G independent gradients of the SAME shape in one launch -- the K steps of a flow level, one
    // atomic tail instead of K.  gemm_wgrad_b3_kernel: blockIdx.z = grp * mtiles + mt, a K split per group; the ring
    // kernels: no grid dimension carries the group, the workgroups of a tile split the groups' flat stage range
    // (wg_split_part below).
    int G, mtiles;
    const float* ga[16];
    const float* gb[16];
    const float* gb2[16];
    float* ggw[16];
};

// operands of group `grp` of a grouped launch (or the single gradient's).  The group tables are read with
// COMPILE-TIME indices: a run-time index into the by-value parameter struct keeps the whole struct in scratch memory
// (632 bytes per lane, every field read through it -- what every kernel of this file did until round 3).
struct WgOperands { const float* a; const float* b; const float* b2; float* gw; };
__device__ __forceinline__ WgOperands wg_operands(const GemmWgradParams& p, const int grp) {
    WgOperands o = {p.a, p.b, p.b2, p.gw};
    if (p.G > 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i == grp) {
                o.a = p.ga[i];
                o.b = p.gb[i];
                o.b2 = p.gb2[i];
                o.gw = p.ggw[i];
            }
    }
    return o;
}
// The same for the ring kernels, which change group INSIDE their K loop (wg_split_part): there the compile-time select
// keeps all 64 table entries live in SGPRs across the stage loop (hundreds of spills).  They read the four pointers of
// the group from the kernel-argument segment itself instead -- p is the kernel's only argument, so the segment IS a
// GemmWgradParams -- with four scalar loads at a run-time offset; the by-value copy is still never indexed.  The
// launchers of the kernels that call this assert the kernel's signature (wg_sole_argument): a second kernel argument
// would move nothing (p stays first) but a wrapper that passes p differently must not compile.
__device__ __forceinline__ WgOperands wg_operands_kernarg(const int grp) {
    typedef const GemmWgradParams __attribute__((address_space(4))) KernargParams;
    KernargParams* kp = (KernargParams*)__builtin_amdgcn_kernarg_segment_ptr();
    WgOperands o = {kp->ga[grp], kp->gb[grp], kp->gb2[grp], kp->ggw[grp]};
    return o;
}
template <class Kern>
constexpr bool wg_sole_argument(Kern) { return std::is_same<Kern, void (*)(GemmWgradParams)>::value; }
// q, which points into the operand `from`, moved to the same place of the operand `to` (the next group's)
__device__ __forceinline__ const float* wg_rebase(const float* q, const float* from, const float* to) {
    return reinterpret_cast<const float*>((uintptr_t)q - (uintptr_t)from + (uintptr_t)to);
}

// K split of a grouped launch of the ring kernels: the unit of work is the flat stage space of ONE output tile,
// T = G * n_stages stages with group g owning [g * n_stages, (g + 1) * n_stages).  Workgroup w of the Wt of a tile owns
// the contiguous range [w T / Wt, (w + 1) T / Wt) -- two ranges differ by at most one stage, and every CU works
// whatever G is (a per-group split S = 256 / (tiles G) leaves 256 - S tiles G of them idle).  A range that crosses group
// boundaries is processed as parts, one per group it touches: (group, first stage of the group, count).
// wg_split_part hands out the parts of workgroup w in order: `pos` starts at wg_split_begin and is advanced; false when
// the range is used up (at once for an empty range, Wt > T).  The kernels and the launchers share it; the C ABI exports
// it as rfn_wgrad_split_parts.
struct WgPart { int grp, s0, cnt; };
__host__ __device__ inline long wg_split_begin(int G, int n_stages, int Wt, int w) {
    return (long)w * ((long)G * n_stages) / Wt;
}
__host__ __device__ inline bool wg_split_part(int G, int n_stages, int Wt, int w, long& pos, WgPart& part) {
    const long end = (long)(w + 1) * ((long)G * n_stages) / Wt;
    if (pos >= end) return false;
    const long g = pos / n_stages;
    part.grp = (int)g;
    part.s0 = (int)(pos - g * n_stages);
    const long left = end - pos, in_group = (long)n_stages - part.s0;
    part.cnt = (int)(left < in_group ? left : in_group);
    pos += part.cnt;
    return true;
}
// workgroups per output tile of a grouped ring launch: the chip's 256 CUs over the tiles, at least 8 stages each
// (`slots`: workgroups the chip holds at once -- 512 for the tiles of which two fit a CU)
__host__ __device__ inline int wg_split_workgroups(int tiles, int G, int n_stages, int slots = 256) {
    long Wt = slots / tiles, cap = (long)G * n_stages / 8;
    if (Wt > cap) Wt = cap;
    return Wt < 1 ? 1 : (int)Wt;
}

// ---- device pieces the three kernels below share
template <int N_>
__device__ __forceinline__ void wg_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }
template <int TM, int TN>
__device__ __forceinline__ void wg_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
// one k-step of a 32 x 32 tile: (ah + al)(bh + bl) without al bl, the small products first
__device__ __forceinline__ void wg_mfma3(f32x16& acc, const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}
// epilogue: acc of wave (wm, wn) added into gw [M][N], tile origin (m0, n0), with float atomics.
// D[i = m][j = n]: col = lane&31 = n (32 consecutive floats of a gw row = one 128-byte atomic segment)
template <int TM, int TN>
__device__ __forceinline__ void wg_add_tile(const f32x16 (&acc)[TM][TN], float* gw, const int M, const int N, const int m0,
                                            const int n0, const int wm, const int wn, const int l31, const int kk) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (m < M && n < N) atomicAdd(&gw[(long)m * N + n], acc[i][j][r]);
            }
        }
}
// The ring kernels pass wg_add_tile a tile origin made opaque per part: the offsets and bounds masks of the 16 TM TN
// atomics do not depend on the part, and hoisted out of the part loop they live, and spill, through the stage loop -- 256
// VGPRs + 92 spilled and 234 spilled SGPRs for the 256 x 256 tile without this, 240 and none with it, as before the part
// loop.  The empty asm computes nothing; if a compiler stops honouring it, tools/kernel_resources.py shows spills and a
// ScratchSize above 0 for the three ring kernels.
__device__ __forceinline__ void wg_opaque_origin(int& m0, int& n0) { asm volatile("" : "+s"(m0), "+s"(n0)); }

// The passes of a ring kernel's workgroup, each ending in an epilogue.  Ungrouped launch: ONE pass over the interleaved
// stages blockIdx.x, + gridDim.x, ...; grouped (G > 0): one pass per part of my range of the flat stage space
// (wg_split_part), over consecutive stages of the part's group.  The groups share shapes and strides, so a kernel
// computes its addresses once and on entering a part only moves their bases to the group's operands (wg_rebase).
struct WgParts {
    WgPart part;   // grouped: the part of the current pass
    long pos;      // where my range goes on
    int i;         // passes done
};
__device__ __forceinline__ WgParts wg_parts_begin(const GemmWgradParams& p) {
    WgParts ps;
    ps.pos = p.G > 0 ? wg_split_begin(p.G, p.n_stages, gridDim.x, blockIdx.x) : 0;
    ps.i = 0;
    return ps;
}
__device__ __forceinline__ bool wg_parts_next(const GemmWgradParams& p, WgParts& ps) {
    return p.G > 0 ? wg_split_part(p.G, p.n_stages, gridDim.x, blockIdx.x, ps.pos, ps.part) : ps.i == 0;
}
// entering part `part`: its stages and its group's operands (the caller rebases its pointers to them)
__device__ __forceinline__ WgOperands wg_part_enter(const WgPart& part, int& first, int& step, int& nmine) {
    first = part.s0;
    step = 1;
    nmine = part.cnt;
    return wg_operands_kernarg(part.grp);
}
// between two passes: the previous part's atomics have retired (they count in vmcnt like the DMA pieces the kernels'
// waits count), its fragment reads have returned, and nobody reads the slots and planes the next prologue is about to fill
__device__ __forceinline__ void wg_parts_drain() {
    wg_wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// Staging unit of the shifted operand of the implicit 3x3 forms: row n = ci*9 + tap of B (the output [Cout][9*Cin] IS
// the torch weight layout [Cout][Cin][3][3]) is plane ci of the two-source input (pb: the first C1 planes, pb2: the
// rest) shifted by the tap -- by the opposite tap for the mirrored form.  Rows beyond N take row 0 (the caller masks them).
// (gemm_wgrad_b3_kernel keeps the fields as plain per-unit arrays and gemm_wgrad_dma_impl_kernel as WgTap[]: what the
// staging lambdas capture decides the register allocation of every instantiation, the non-implicit ones included.)
struct WgTap {
    const float* plane;
    long ns;       // frame stride of the plane's source
    int dy, dx;
    bool first;    // the plane is of pb
};
__device__ __forceinline__ WgTap wg_tap(int row, const GemmWgradParams& p, const float* pb, const float* pb2) {
    if (row >= p.N) row = 0;
    const int ci = row / 9, tap = row - ci * 9;
    WgTap t;
    t.dy = p.mirror ? 1 - tap / 3 : tap / 3 - 1;
    t.dx = p.mirror ? 1 - tap % 3 : tap % 3 - 1;
    t.first = ci < p.C1;
    t.plane = t.first ? pb + (long)ci * p.HW : pb2 + (long)(ci - p.C1) * p.HW;
    t.ns = t.first ? p.b_ns : p.b2_ns;
    return t;
}
// the 8 pixels (y, x0 .. x0 + 7) of frame f lie in one image row (W % 8 == 0); shifted by dx they need one element beyond
// either end.  Unconditional loads: the row is clamped (rok: inside the image) and so is the edge element (eok)
struct WgTapRow {
    float4 v[2];
    float edge;
    bool rok, eok;
};
__device__ __forceinline__ WgTapRow wg_tap_load(const float* plane, const long ns, const int dy, const int dx,
                                                const unsigned f, const int y, const int x0, const int H, const int W) {
    WgTapRow r;
    const int yy = y + dy;
    r.rok = yy >= 0 && yy < H;
    const float* src = plane + (long)f * ns + (r.rok ? yy : y) * W + x0;
    r.v[0] = *reinterpret_cast<const float4*>(src);
    r.v[1] = *reinterpret_cast<const float4*>(src + 4);
    r.eok = dx < 0 ? x0 > 0 : x0 + 8 < W;  // the element beyond the end, inside the row?
    r.edge = src[r.eok ? (dx < 0 ? -1 : 8) : 0];
    return r;
}
// the loaded row shifted by dx, zeroed unless `ok`, split into bf16 (hi, lo)
__device__ __forceinline__ void wg_shift_split8(const float4 (&src)[2], const float edge, const int dx, const bool ok,
                                                const bool eok, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {src[0].x, src[0].y, src[0].z, src[0].w, src[1].x, src[1].y, src[1].z, src[1].w};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float left = c == 0 ? (eok ? edge : 0.f) : v[c > 0 ? c - 1 : 0];
        const float right = c == 7 ? (eok ? edge : 0.f) : v[c < 7 ? c + 1 : 7];
        float x = dx < 0 ? left : (dx > 0 ? right : v[c]);
        x = ok ? x : 0.f;
        const __bf16 h = (__bf16)x;
        hi[c] = h;
        lo[c] = (__bf16)(x - (float)h);
    }
}

// Rows shorter than a staging unit (IMPL = WG_ROWS4 / WG_ROWS2 of gemm_wgrad_b3_kernel): the 8 pixels of a unit are
//   * W == 4 (H even): the two image rows y0, y0 + 1 of one frame -- half h is row y0 + h + dy, one aligned 16-byte load,
//     clamped to row y0 + h for the load with its own row-ok bit; the x shift happens inside the float4, zero fill at
//     both ends, no edge element;
//   * H == W == 2: two consecutive frames, one 16-byte load each (the second clamped to the first when it is past the
//     last frame; the caller masks it); tap (dy, dx) is a fixed zero-filling permutation of the four pixels.
// Unconditional loads like wg_tap_load; all masking in wg_shift_split4.
constexpr int WG_ROWS4 = 2, WG_ROWS2 = 3;
__host__ __device__ inline bool wg_rows_covers(int H, int W) {
    return (W == 4 && H >= 2 && H % 2 == 0) || (H == 2 && W == 2);
}
constexpr int wg_rows_impl(int W) { return W == 4 ? WG_ROWS4 : WG_ROWS2; }
// half a unit (4 pixels), out[y][x] = in[y + dy][x + dx] where inside -- ROWS4: one image row, x shift only (the row
// shift was the load's); ROWS2: a 2 x 2 frame, both shifts -- zeroed unless `ok`, split into lanes c0 .. c0 + 3 of (hi, lo)
template <int ROWS>
__device__ __forceinline__ void wg_shift_split4(const float4 src, const int dy, const int dx, const bool ok, const int c0,
                                                bf16x8& hi, bf16x8& lo) {
    float v[4] = {src.x, src.y, src.z, src.w};
    if (ROWS == WG_ROWS4) {
        const float l[4] = {0.f, v[0], v[1], v[2]}, r[4] = {v[1], v[2], v[3], 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = dx < 0 ? l[c] : (dx > 0 ? r[c] : v[c]);
    } else {
        const float up[4] = {0.f, 0.f, v[0], v[1]}, dn[4] = {v[2], v[3], 0.f, 0.f};   // in[y - 1][x], in[y + 1][x]
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = dy < 0 ? up[c] : (dy > 0 ? dn[c] : v[c]);
        const float l[4] = {0.f, v[0], 0.f, v[2]}, r[4] = {v[1], 0.f, v[3], 0.f};      // in[y][x - 1], in[y][x + 1]
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = dx < 0 ? l[c] : (dx > 0 ? r[c] : v[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float x = ok ? v[c] : 0.f;
        const __bf16 h = (__bf16)x;
        hi[c0 + c] = h;
        lo[c0 + c] = (__bf16)(x - (float)h);
    }
}

// WM x WN waves (4 or 8) of TM x TN 32x32 tiles each.  The 8-wave 256-row configurations read both operands of the
// big level-0 / level-1 gradients exactly once (a 128 x 128 tiling of a 256 x 256 gradient reads each of them twice,
// and those launches sit on the HBM roof).
template <int WM, int WN, int TM, int TN, int KP, int IMPL = 0>
__global__ __launch_bounds__(64 * WM * WN) void gemm_wgrad_b3_kernel(const GemmWgradParams p) {
    constexpr int NT = 64 * WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int NU = KP / 8;        // 16-byte units (8 pixels) per row and stage
    constexpr int RS = NU + 1;        // odd-ish row stride in units -> conflict-free b128 fragment reads
    constexpr int AU = (BM * NU + NT - 1) / NT;  // units staged per thread (A)
    constexpr int BU = (BN * NU + NT - 1) / NT;
    constexpr bool AX = (BM * NU) % NT == 0, BX = (BN * NU) % NT == 0;  // exact: no tail guard
    static_assert(WM * WN == 4 || WM * WN == 8, "tile/stage shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16x8* Ah = reinterpret_cast<bf16x8*>(lds_raw);
    bf16x8* Al = Ah + BM * RS;
    bf16x8* Bh = Al + BM * RS;
    bf16x8* Bl = Bh + BN * RS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, kk = lane >> 5;
    const int grp = p.G > 0 ? (int)blockIdx.z / p.mtiles : 0;
    const int m0 = (p.G > 0 ? (int)blockIdx.z - grp * p.mtiles : (int)blockIdx.z) * BM, n0 = blockIdx.y * BN;
    const WgOperands ops_ = wg_operands(p, grp);
    const float* const pa_ = ops_.a;
    const float* const pb_ = ops_.b;
    const float* const pb2_ = ops_.b2;
    float* const pgw_ = ops_.gw;

    f32x16 acc[TM][TN];
    wg_zero(acc);

    // staging: unit e = tid + NT*u  ->  row = e / NU, k-group = e % NU   (consecutive threads = consecutive pixels)
    float4 ast[AU][2], bst[BU][2];
    // All units of a thread share the k-group (NT % NU == 0), so the (frame, pixel) split of a stage's two 4-pixel
    // groups is computed once per stage and thread -- the only divisions of the loop (32-bit: total < 2^31 is checked
    // on the host).  A group never straddles a frame because HW % 4 == 0.
    static_assert(NT % NU == 0, "k-group must be a per-thread constant");
    const int kg = tid % NU, r0 = tid / NU;   // unit u of this thread: row r0 + u*(NT/NU), k-group kg
    const unsigned uHW = (unsigned)p.HW;
    // The loads of the NEXT stage are issued ahead of the MFMAs of the current one and are not touched until the next
    // commit: unconditional (clamped rows / pixels, no select on a loaded value, no control flow) -- otherwise the
    // compiler waits for HBM right behind the loads and nothing overlaps.  Masks are applied in commit().
    bool okq[2] = {false, false};
    // implicit mode: per unit (fixed row n = ci*9 + tap) its tap (wg_tap); per stage the row's edge element and masks
    const float* uplane[IMPL ? BU : 1];
    long uns[IMPL ? BU : 1];
    int udy[IMPL ? BU : 1], udx[IMPL ? BU : 1];
    float bedge[IMPL ? BU : 1];
    unsigned rowmask = 0, edgemask = 0;
    if (IMPL) {
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const WgTap t = wg_tap(n0 + r0 + u * (NT / NU), p, pb_, pb2_);
            uplane[u] = t.plane;
            uns[u] = t.ns;
            udy[u] = t.dy;
            udx[u] = t.dx;
        }
    }
    auto prefetch = [&](int stage) {
        const unsigned q0 = (unsigned)stage * KP + 8u * kg;
        long offa[2], offb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned q = q0 + 4u * h;
            okq[h] = stage < p.n_stages && q < (unsigned)p.total;
            const unsigned qq = okq[h] ? q : 0u;
            const unsigned f = qq / uHW, px = qq - f * uHW;
            offa[h] = (long)f * p.a_ns + px;
            offb[h] = (long)f * p.b_ns + px;
        }
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int row = m0 + r0 + u * (NT / NU);
            const float* base = pa_ + (long)(row < p.M ? row : 0) * p.HW;
#pragma unroll
            for (int h = 0; h < 2; ++h) ast[u][h] = *reinterpret_cast<const float4*>(base + offa[h]);
        }
        if (IMPL >= WG_ROWS4) {
            // short rows: half h of the unit is an image row (rowmask / edgemask: row-ok of half 0 / 1) or a frame
            const unsigned qq = okq[0] ? q0 : 0u;
            const unsigned f = qq / uHW, pix = qq - f * uHW;
            const int y0 = (int)(pix >> 2);
            const unsigned f1 = okq[1] ? f + 1u : f;
            rowmask = IMPL == WG_ROWS4 ? 0u : ~0u;
            edgemask = rowmask;
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                if (IMPL == WG_ROWS4) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int yy = y0 + h + udy[u];
                        const bool rok = yy >= 0 && yy < p.H;
                        bst[u][h] = *reinterpret_cast<const float4*>(uplane[u] + (long)f * uns[u] + (rok ? yy : y0 + h) * 4);
                        (h ? edgemask : rowmask) |= (rok ? 1u : 0u) << u;
                    }
                } else {
                    bst[u][0] = *reinterpret_cast<const float4*>(uplane[u] + (long)f * uns[u]);
                    bst[u][1] = *reinterpret_cast<const float4*>(uplane[u] + (long)f1 * uns[u]);
                }
            }
        } else if (IMPL) {
            const unsigned qq = okq[0] ? q0 : 0u;
            const unsigned f = qq / uHW, pix = qq - f * uHW;
            const int y = (int)(pix / (unsigned)p.W), x0 = (int)(pix - (unsigned)y * (unsigned)p.W);
            rowmask = 0;
            edgemask = 0;
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const WgTapRow r = wg_tap_load(uplane[u], uns[u], udy[u], udx[u], f, y, x0, p.H, p.W);
                bst[u][0] = r.v[0];
                bst[u][1] = r.v[1];
                bedge[u] = r.edge;
                rowmask |= (r.rok ? 1u : 0u) << u;
                edgemask |= (r.eok ? 1u : 0u) << u;
            }
        } else {
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const int row = n0 + r0 + u * (NT / NU);
                const float* base = pb_ + (long)(row < p.N ? row : 0) * p.HW;
#pragma unroll
                for (int h = 0; h < 2; ++h) bst[u][h] = *reinterpret_cast<const float4*>(base + offb[h]);
            }
        }
    };
    auto split_store = [&](const float4 (&src)[2], bool okr, bf16x8* hi_p, bf16x8* lo_p) {
        const float v[8] = {src[0].x, src[0].y, src[0].z, src[0].w, src[1].x, src[1].y, src[1].z, src[1].w};
        bf16x8 hi, lo;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float x = (okr && okq[c >> 2]) ? v[c] : 0.f;
            const __bf16 h = (__bf16)x;
            hi[c] = h;
            lo[c] = (__bf16)(x - (float)h);
        }
        *hi_p = hi;
        *lo_p = lo;
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int o = (r0 + u * (NT / NU)) * RS + kg;
            if (AX || r0 + u * (NT / NU) < BM) split_store(ast[u], m0 + r0 + u * (NT / NU) < p.M, Ah + o, Al + o);
        }
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const int o = (r0 + u * (NT / NU)) * RS + kg;
            if (BX || r0 + u * (NT / NU) < BN) {
                const bool okr = n0 + r0 + u * (NT / NU) < p.N;
                if (IMPL >= WG_ROWS4) {
                    bf16x8 hi, lo;
                    wg_shift_split4<IMPL>(bst[u][0], udy[u], udx[u], okr && ((rowmask >> u) & 1u) && okq[0], 0, hi, lo);
                    wg_shift_split4<IMPL>(bst[u][1], udy[u], udx[u], okr && ((edgemask >> u) & 1u) && okq[1], 4, hi, lo);
                    Bh[o] = hi;
                    Bl[o] = lo;
                } else if (IMPL) {
                    bf16x8 hi, lo;
                    wg_shift_split8(bst[u], bedge[u], udx[u], okr && ((rowmask >> u) & 1u) && okq[0],
                                    (edgemask >> u) & 1u, hi, lo);
                    Bh[o] = hi;
                    Bl[o] = lo;
                } else
                    split_store(bst[u], okr, Bh + o, Bl + o);
            }
        }
    };

    const int arow = (wm * TM * 32 + l31) * RS + kk;  // + i*32*RS + 2*s
    const int brow = (wn * TN * 32 + l31) * RS + kk;
    int stage = blockIdx.x;
    prefetch(stage);
    for (; stage < p.n_stages; stage += gridDim.x) {
        __syncthreads();
        commit();
        __syncthreads();
        prefetch(stage + gridDim.x);        // always issued; past the end it re-reads pixel 0 and is never committed
        __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the MFMAs (the scheduler sinks them)
        // 8-wave tiles with 64-pixel stages: one k-step of fragments live at a time (register budget 256)
#pragma unroll WM * WN == 8 && KP > 32 ? 1 : KP / 16
        for (int s = 0; s < KP / 16; ++s) {
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = Ah[arow + i * 32 * RS + 2 * s];
                al[i] = Al[arow + i * 32 * RS + 2 * s];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[j] = Bh[brow + j * 32 * RS + 2 * s];
                bl[j] = Bl[brow + j * 32 * RS + 2 * s];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) wg_mfma3(acc[i][j], ah[i], al[i], bh[j], bl[j]);
        }
    }
    wg_add_tile(acc, pgw_, p.M, p.N, m0, n0, wm, wn, l31, kk);
}

// ------------------------------------------------------------------------------------------------ LDS-DMA variant
// The big gradients of the shallow flow levels (256 x 256 and 9C x 256 over 10^5 .. 10^6 pixels) read two 637 MB
// operands per launch and sit on the HBM roof -- if the loads are kept in flight.  The register-staged kernel above has
// ONE stage in flight per workgroup, and only while its MFMAs run: load -> convert -> LDS -> MFMA serialise into
// ~23 k cycles per 64-pixel stage against ~14 k of pure data movement.  Here the raw fp32 rows go HBM -> LDS by LDS-DMA
// (global_load_lds_dwordx4, no registers) into a ring of NST stages of KP pixels, two to three stages ahead of the
// MFMAs, and the fp32 -> bf16 (hi, lo) split moves to the fragment reads (each wave converts the fragments it consumes:
// 3x the conversions of a cooperative commit, issued in the shadow of the MFMAs).
//   * one DMA wave-instruction = 1 KB = 64 / UPR rows x UPR units of 16 B (UPR = KP / 4): coalesced row segments; LDS
//     image of a stage: [row][UPR units];
//   * the unit order inside a row is XOR-swizzled with (row / (16 / UPR)) & (UPR - 1) -- the LDS destination of a DMA
//     is linear in the lane, but WHICH global unit a lane fetches is free -- so the fragment reads (lane = row, two
//     ds_read_b128 per 8-pixel fragment) are conflict-free in the hardware's 16-lane groups (MI355X guide, LDS table);
//   * rows beyond M / N are clamped to the last valid row (their products are never written);
//   * ONE barrier per stage and one continuous software pipeline over all stages: the barrier at the top of stage t
//     certifies that everybody's pieces of stage t + 1 have landed (its first fragments are read during stage t) and
//     that everybody has left stage t - 1, whose slot the pieces of stage t + NST - 1 then fill -- issued one at a time
//     between the MFMAs.  Per unit (k-step, A tile): raw fragment of unit u + 2 read from LDS, TN x 3 MFMAs of unit u,
//     fragment of unit u + 1 split; the B fragments of the next k-step are read during its unit 0 and split, one tile
//     per unit, from unit 1 on.
// K split, epilogue atomics and operand roles are those of gemm_wgrad_b3_kernel (non-implicit, non-grouped).
__device__ __forceinline__ void wg_split8(const f32x4 lo4, const f32x4 hi4, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const __bf16 h = (__bf16)v[c];
        hi[c] = h;
        lo[c] = (__bf16)(v[c] - (float)h);
    }
}

template <int WM, int WN, int TM, int TN, int KP, int NST>
__global__ __launch_bounds__(64 * WM * WN) void gemm_wgrad_dma_kernel(const GemmWgradParams p) {
    constexpr int NW = WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int UPR = KP / 4, RPP = 64 / UPR, SWD = 16 / UPR;          // units per row, rows per piece, swizzle divisor
    constexpr int RB = KP * 4;                                            // bytes per row and stage
    constexpr int ROWS = BM + BN, PIECES = ROWS / RPP, PPW = PIECES / NW;  // 1-KB DMA pieces per stage / per wave
    constexpr int STAGE = ROWS * RB;                                      // bytes per ring slot
    constexpr int NK = KP / 16, NU_ = NK * TM;                            // k-steps / units per stage
    static_assert(KP == 16 || KP == 32, "stage width");
    static_assert(PIECES % NW == 0 && BM % 16 == 0 && NST >= 2, "pieces shared evenly; swizzle period divides BM");
    // NST >= 3: the software pipeline runs across stage boundaries (the first fragments of stage t + 1 are read during
    // stage t).  NST == 2 (the 256 x 256 tile: two 64-KB slots of 32 pixels; 16-pixel stages would fit four slots but
    // their 64-byte row segments stream at half the rate): stage t + 1 is in flight while stage t is consumed, the
    // pipeline drains and refills at every stage boundary.
    constexpr bool LOOK = NST >= 3;
    static_assert(TM % 2 == 0 && TM >= TN + 1, "pipeline parities");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, kk = lane >> 5;
    const int m0 = blockIdx.z * BM, n0 = blockIdx.y * BN;
    // the operands in hand: the single gradient's, or (grouped launch, G > 0) those of the group of the current part --
    // the groups share shapes and strides, so everything below is computed once and only the bases move (wg_rebase)
    const float* pa_ = p.a;
    const float* pb_ = p.b;
    float* pgw_ = p.gw;

    f32x16 acc[TM][TN];

    // this lane's share of a stage: PPW pieces; piece q = wave + j NW covers stacked rows RPP q .. (A rows, then B rows)
    const float* prow[PPW];   // row base + this lane's (swizzled) unit
    bool pisa[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int r = RPP * (wave + j * NW) + lane / UPR;               // stacked row
        const int u = (lane & (UPR - 1)) ^ ((r / SWD) & (UPR - 1));     // global unit that lands in LDS unit lane % UPR
        pisa[j] = r < BM;
        if (pisa[j]) {
            int row = m0 + r;
            row = row < p.M ? row : p.M - 1;
            prow[j] = pa_ + (long)row * p.HW + 4 * u;
        } else {
            int row = n0 + r - BM;
            row = row < p.N ? row : p.N - 1;
            prow[j] = pb_ + (long)row * p.HW + 4 * u;
        }
    }
    const unsigned uHW = (unsigned)p.HW;
    const int S = gridDim.x;
    // my stages: first, first + step, ... (nmine of them).  Ungrouped: blockIdx.x, + S, ...; grouped: the stages of one
    // part of my range of the flat stage space (wg_split_part), consecutive
    int first = blockIdx.x, step = S, nmine = (p.n_stages - (int)blockIdx.x + S - 1) / S;
    // frame / pixel offsets of my stage t (clamped to my last one: pieces past the end re-read it and are never used)
    long offa = 0, offb = 0;
    auto stage_offsets = [&](int t) {
        t = t < nmine ? t : nmine - 1;
        const unsigned q0 = (unsigned)(first + t * step) * KP;
        const unsigned f = q0 / uHW, px = q0 - f * uHW;          // a stage never straddles a frame (HW % KP == 0)
        offa = (long)f * p.a_ns + px;
        offb = (long)f * p.b_ns + px;
    };
    auto piece = [&](const int j, const int slot) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(prow[j] + (pisa[j] ? offa : offb)),
                                         (__attribute__((address_space(3))) void*)(lds_raw + slot * STAGE + (wave + j * NW) * 1024),
                                         16, 0, 0);
    };

    // fragment byte offsets inside a slot: row * RB + ((2 (2 s + kk) + h) ^ swz(row)) * 16
    int aoff[TM], boff[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = (wm * TM + i) * 32 + l31;
        aoff[i] = r * RB + (((2 * kk) ^ ((r / SWD) & (UPR - 1))) << 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int r = BM + (wn * TN + j) * 32 + l31;
        boff[j] = r * RB + (((2 * kk) ^ ((r / SWD) & (UPR - 1))) << 4);
    }
    auto raw = [&](const unsigned char* sb, const int off, const int s_, f32x4 (&r)[2]) {
        const int o = off ^ (s_ << 6);
        r[0] = *reinterpret_cast<const f32x4*>(sb + o);
        r[1] = *reinterpret_cast<const f32x4*>(sb + (o ^ 16));
    };

    f32x4 ra[2][2], rb[TN][2];
    bf16x8 ah[2], al[2], bh[2][TN], bl[2][TN];
    auto first_fragments = [&](const unsigned char* sb0) {
#pragma unroll
        for (int j = 0; j < TN; ++j) raw(sb0, boff[j], 0, rb[j]);
        raw(sb0, aoff[0], 0, ra[0]);
        raw(sb0, aoff[1], 0, ra[1]);
#pragma unroll
        for (int j = 0; j < TN; ++j) wg_split8(rb[j][0], rb[j][1], bh[0][j], bl[0][j]);
        wg_split8(ra[0][0], ra[0][1], ah[0], al[0]);
    };

    // one pass per part (WgParts)
    for (WgParts ps = wg_parts_begin(p); wg_parts_next(p, ps); ++ps.i) {
        if (p.G > 0) {
            const WgOperands o = wg_part_enter(ps.part, first, step, nmine);
#pragma unroll
            for (int j = 0; j < PPW; ++j) prow[j] = pisa[j] ? wg_rebase(prow[j], pa_, o.a) : wg_rebase(prow[j], pb_, o.b);
            pa_ = o.a;
            pb_ = o.b;
            pgw_ = o.gw;
        }
        if (ps.i > 0) wg_parts_drain();
        wg_zero(acc);

        // prologue: stages 0 .. NST-2 in flight; (LOOK) stage 0 landed, its first fragments read and split
#pragma unroll
        for (int t = 0; t < NST - 1; ++t) {
            stage_offsets(t);
#pragma unroll
            for (int j = 0; j < PPW; ++j) piece(j, t);
        }
        if (LOOK) {
            wg_wait_vm<(NST - 2) * PPW>();
            __builtin_amdgcn_s_barrier();
            first_fragments(lds_raw);
        }

        int slot = 0;
        for (int it = 0; it < nmine; ++it) {
            // top of stage `it`.  LOOK: my pieces of stage it + 1 have landed once only those of the stages issued after it
            // are outstanding; the barrier makes that everybody's pieces and frees the slot of stage it - 1.  Two slots: the
            // same for stage `it` itself (nothing younger is outstanding).
            wg_wait_vm<LOOK ? (NST - 3) * PPW : 0>();
            __builtin_amdgcn_s_barrier();
            const int nslot = slot + 1 == NST ? 0 : slot + 1;
            const int fslot = slot == 0 ? NST - 1 : slot - 1;          // slot of stage it - 1 = slot of stage it + NST - 1
            const unsigned char* sb = lds_raw + slot * STAGE;
            const unsigned char* sn = lds_raw + nslot * STAGE;
            stage_offsets(it + NST - 1);
            if (!LOOK) {
                // two slots: the next stage's pieces have exactly this stage to land -- issued before anything else
#pragma unroll
                for (int j = 0; j < PPW; ++j) piece(j, fslot);
                first_fragments(sb);
            }
#pragma unroll
            for (int u = 0; u < NU_; ++u) {
                const int s_ = u / TM, i = u % TM, cur = u & 1, kb = s_ & 1;
                // raw A fragment of unit u + 2 (this stage or the next one)
                if (u + 2 < NU_) raw(sb, aoff[(u + 2) % TM], (u + 2) / TM, ra[cur]);
                else if (LOOK) raw(sn, aoff[(u + 2) % TM], 0, ra[cur]);
                // raw B fragments of the next k-step
                if (i == 0) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if (s_ + 1 < NK) raw(sb, boff[j], s_ + 1, rb[j]);
                        else if (LOOK) raw(sn, boff[j], 0, rb[j]);
                    }
                }
                // the DMA pieces of the stage that will fill the freed slot (NST - 2 stages to land): one per MFMA gap of
                // the first unit(s)
                if (LOOK && u == 0) {
#pragma unroll
                    for (int j = 0; j < PPW; ++j) piece(j, fslot);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) wg_mfma3(acc[i][j], ah[cur], al[cur], bh[kb][j], bl[kb][j]);
                if (LOOK || u + 1 < NU_) wg_split8(ra[cur ^ 1][0], ra[cur ^ 1][1], ah[cur ^ 1], al[cur ^ 1]);
                if (i >= 1 && i <= TN && (LOOK || s_ + 1 < NK))
                    wg_split8(rb[i - 1][0], rb[i - 1][1], bh[kb ^ 1][i - 1], bl[kb ^ 1][i - 1]);
            }
            if (LOOK && (NK & 1)) {   // an odd number of k-steps per stage: the next stage starts on the other B buffer
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    bh[0][j] = bh[1][j];
                    bl[0][j] = bl[1][j];
                }
            }
            // the schedule of the stage, spelled out for the compiler (left alone it issues the conversions in long VALU
            // runs and the MFMAs back to back, i.e. one after the other): after every MFMA up to six VALU, one LDS read
            // and (first units) one DMA piece in its shadow
            if (!LOOK) {
                __builtin_amdgcn_sched_group_barrier(0x020, PPW, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * TN + 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 30 * (TN + 1), 0);
            }
#pragma unroll
            for (int g = 0; g < NU_ * TN * 3; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (LOOK && g < PPW) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
            slot = nslot;
        }
        wg_wait_vm<0>();   // (pieces past the end)
        int m0e = m0, n0e = n0;
        wg_opaque_origin(m0e, n0e);
        wg_add_tile(acc, pgw_, p.M, p.N, m0e, n0e, wm, wn, l31, kk);
    }   // parts
}

// ---- launchers: each sets p.n_stages for its stage width and decides its LDS size and K split S (gridDim.x);
// wg_launch is their common tail.  zgroups: groups carried by gridDim.z (gemm_wgrad_b3_kernel), 1 for the ring kernels.
static int wg_tiles(const GemmWgradParams& p, int BM, int BN) { return ceil_div(p.M, BM) * ceil_div(p.N, BN); }
template <class Kern>
static void wg_launch(Kern kern, GemmWgradParams& p, int BM, int BN, int NT, int S, int zgroups, size_t lds,
                      hipStream_t s) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    p.mtiles = ceil_div(p.M, BM);
    dim3 grid(S, ceil_div(p.N, BN), p.mtiles * zgroups);
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, s, p);
}

template <int WM, int WN, int TM, int TN, int KP, int NST>
static void launch_gemm_wgrad_dma(GemmWgradParams& p, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    p.n_stages = (int)(p.total / KP);
    // one 8-wave workgroup per CU (see launch_gemm_wgrad), at least 8 stages each; grouped: over the flat stage space
    // of the G groups (wg_split_part), so gridDim.x is the split of a TILE and no grid dimension carries the group
    const int S = wg_split_workgroups(wg_tiles(p, BM, BN), p.G > 0 ? p.G : 1, p.n_stages);
    auto kern = gemm_wgrad_dma_kernel<WM, WN, TM, TN, KP, NST>;
    static_assert(wg_sole_argument(decltype(kern){}), "wg_operands_kernarg reads p from the kernel-argument segment");
    wg_launch(kern, p, BM, BN, 64 * WM * WN, S, 1, (size_t)NST * (BM + BN) * KP * 4, s);
}

// Implicit 3x3 form of the ring kernel (conv1's weight gradient at the shallow levels: gw[256][ci*9 + tap], A = the
// 256-channel gradient image, B = the 18 / 36 input planes shifted by the tap).  The BIG operand A goes through the DMA
// ring (two slots of 256 rows x 32 pixels, split at the fragment reads) exactly as above; the SMALL operand keeps the
// cooperative register staging of gemm_wgrad_b3_kernel<..., IMPL = 1> -- its 9 Cin rows are built from L2-resident
// planes with the shift and the (hi, lo) split, into a double buffer of bf16 planes: the loads of stage t + 1 are issued
// at the top of stage t, committed at its end (which also certifies that the DMA pieces issued before them have landed:
// vector-memory operations complete in order), and the barrier at the top of stage t + 1 publishes both.
//
// Narrow column tiles (BN <= 64: the mirrored conv3 gradient of flow level 0, 36 columns) do a few hundred cycles of
// MFMAs per stage against some thousand of DMA, so one workgroup per CU -- one stage in flight -- is bound by latency.
// Two workgroups share a CU instead: 128 registers per lane (the second launch bound: 4 waves per SIMD) and 80 KB of
// LDS each, which the B planes reach without the pad unit -- their rows are 4 units (64 B) and the unit order inside a
// row is XOR-swizzled with (row / 4) & 3, conflict-free for the 16-lane groups of the fragment reads and 256 contiguous
// bytes per 16 lanes for the commit's stores.
constexpr int wg_impl_waves_per_simd(int NW, int BN) { return NW == 8 && BN <= 64 ? 4 : NW / 4; }
constexpr size_t wg_impl_lds(int BM, int BN) { return (size_t)2 * BM * 128 + (size_t)2 * 2 * BN * (BN <= 64 ? 4 : 5) * 16; }

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(64 * WM * WN, wg_impl_waves_per_simd(WM * WN, 32 * TN * WN))
void gemm_wgrad_dma_impl_kernel(const GemmWgradParams p) {
    constexpr int NW = WM * WN, NT = 64 * NW, KP = 32, NK = KP / 16;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int PIECES = BM / 8, PPW = PIECES / NW;   // 1-KB DMA pieces (8 rows x 128 B) of the A rows per stage / wave
    constexpr int ASLOT = BM * 128;
    constexpr bool SWZB = BN <= 64;                     // B planes without the pad unit, swizzled (see above)
    constexpr int NU = KP / 8, RS = SWZB ? NU : NU + 1; // B planes: 16-byte units per row, row stride (conflict-free)
    constexpr int BU = (BN * NU + NT - 1) / NT;         // B units staged per thread
    constexpr int BPLANE = BN * RS;                     // units per plane
    static_assert(PIECES % NW == 0 && NT % NU == 0 && TM % 2 == 0, "shares / parities");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16x8* const Bbase = reinterpret_cast<bf16x8*>(lds_raw + 2 * ASLOT);   // [buffer 2][plane 2][BN][RS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, kk = lane >> 5;
    const int m0 = blockIdx.z * BM, n0 = blockIdx.y * BN;
    // the operands in hand (see gemm_wgrad_dma_kernel): the single gradient's, or those of the current part's group
    const float* pa_ = p.a;
    const float* pb_ = p.b;
    const float* pb2_ = p.b2;
    float* pgw_ = p.gw;

    f32x16 acc[TM][TN];

    // ---- A: DMA pieces of this lane (rows 8 q .. 8 q + 7 of the tile, swizzled units: see gemm_wgrad_dma_kernel)
    const float* prow[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int r = 8 * (wave + j * NW) + (lane >> 3);
        const int u = (lane & 7) ^ ((r >> 1) & 7);
        int row = m0 + r;
        row = row < p.M ? row : p.M - 1;
        prow[j] = pa_ + (long)row * p.HW + 4 * u;
    }
    int aoff[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = (wm * TM + i) * 32 + l31;
        aoff[i] = r * 128 + (((2 * kk) ^ ((r >> 1) & 7)) << 4);
    }
    // ---- B: this thread's units (fixed row n = ci * 9 + tap, k-group kg): their taps (wg_tap)
    const int kg = tid % NU, r0 = tid / NU;
    WgTap tap[BU];
#pragma unroll
    for (int u = 0; u < BU; ++u) tap[u] = wg_tap(n0 + r0 + u * (NT / NU), p, pb_, pb2_);
    const unsigned uHW = (unsigned)p.HW;
    const int S = gridDim.x;
    // my stages: first, first + step, ... (ungrouped: blockIdx.x, + S, ...; grouped: one part of my range)
    int first = blockIdx.x, step = S, nmine = (p.n_stages - (int)blockIdx.x + S - 1) / S;
    float4 bst[BU][2];
    float bedge[BU];
    unsigned rowmask = 0, edgemask = 0;
    // loads of my stage t: DMA pieces of A into `slot`, B units into registers (clamped to my last stage)
    auto fetch = [&](int t, const int slot) {
        t = t < nmine ? t : nmine - 1;
        const unsigned q0 = (unsigned)(first + t * step) * KP;
        const unsigned f = q0 / uHW, px = q0 - f * uHW;
        const long offa = (long)f * p.a_ns + px;
#pragma unroll
        for (int j = 0; j < PPW; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(prow[j] + offa),
                                             (__attribute__((address_space(3))) void*)(lds_raw + slot * ASLOT + (wave + j * NW) * 1024),
                                             16, 0, 0);
        const unsigned pix = px + 8u * kg;
        const int y = (int)(pix / (unsigned)p.W), x0 = (int)(pix - (unsigned)y * (unsigned)p.W);
        rowmask = 0;
        edgemask = 0;
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const WgTapRow r = wg_tap_load(tap[u].plane, tap[u].ns, tap[u].dy, tap[u].dx, f, y, x0, p.H, p.W);
            bst[u][0] = r.v[0];
            bst[u][1] = r.v[1];
            bedge[u] = r.edge;
            rowmask |= (r.rok ? 1u : 0u) << u;
            edgemask |= (r.eok ? 1u : 0u) << u;
        }
    };
    auto commit = [&](const int buf) {
        bf16x8* Bh = Bbase + buf * 2 * BPLANE;
        bf16x8* Bl = Bh + BPLANE;
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const int row = r0 + u * (NT / NU);
            if (row < BN) {
                bf16x8 hi, lo;
                wg_shift_split8(bst[u], bedge[u], tap[u].dx, n0 + row < p.N && ((rowmask >> u) & 1u), (edgemask >> u) & 1u,
                                hi, lo);
                const int o = row * RS + (SWZB ? kg ^ ((row >> 2) & 3) : kg);
                Bh[o] = hi;
                Bl[o] = lo;
            }
        }
    };
    auto rawA = [&](const unsigned char* sb, const int i, const int s_, f32x4 (&r)[2]) {
        const int o = aoff[i] ^ (s_ << 6);
        r[0] = *reinterpret_cast<const f32x4*>(sb + o);
        r[1] = *reinterpret_cast<const f32x4*>(sb + (o ^ 16));
    };
    const int brow = (wn * TN * 32 + l31) * RS + (SWZB ? kk ^ ((l31 >> 2) & 3) : kk);   // unit kk + 2 s = kk ^ 2 s

    // one pass per part (WgParts)
    for (WgParts ps = wg_parts_begin(p); wg_parts_next(p, ps); ++ps.i) {
        if (p.G > 0) {
            const WgOperands o = wg_part_enter(ps.part, first, step, nmine);
#pragma unroll
            for (int j = 0; j < PPW; ++j) prow[j] = wg_rebase(prow[j], pa_, o.a);
#pragma unroll
            for (int u = 0; u < BU; ++u)
                tap[u].plane = tap[u].first ? wg_rebase(tap[u].plane, pb_, o.b) : wg_rebase(tap[u].plane, pb2_, o.b2);
            pa_ = o.a;
            pb_ = o.b;
            pb2_ = o.b2;
            pgw_ = o.gw;
        }
        if (ps.i > 0) wg_parts_drain();
        wg_zero(acc);

        // prologue: stage 0 loaded and committed
        fetch(0, 0);
        commit(0);
        int slot = 0;
        for (int it = 0; it < nmine; ++it) {
            wg_wait_vm<0>();                    // (my pieces of this stage: older than the B loads just committed)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();       // everybody's pieces and planes of stage `it`; the other slot / buffer is free
            fetch(it + 1, slot ^ 1);
            const unsigned char* sb = lds_raw + slot * ASLOT;
            const bf16x8* Bh = Bbase + slot * 2 * BPLANE;
            const bf16x8* Bl = Bh + BPLANE;
            f32x4 ra[2][TM][2];
            bf16x8 ah[2][TM], al[2][TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) rawA(sb, i, 0, ra[0][i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) wg_split8(ra[0][i][0], ra[0][i][1], ah[0][i], al[0][i]);
#pragma unroll
            for (int s_ = 0; s_ < NK; ++s_) {
                const int cur = s_ & 1;
                if (s_ + 1 < NK) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) rawA(sb, i, s_ + 1, ra[cur ^ 1][i]);
                }
                bf16x8 bh[TN], bl[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int o = SWZB ? (brow + j * 32 * RS) ^ (2 * s_) : brow + j * 32 * RS + 2 * s_;
                    bh[j] = Bh[o];
                    bl[j] = Bl[o];
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) wg_mfma3(acc[i][j], ah[cur][i], al[cur][i], bh[j], bl[j]);
                if (s_ + 1 < NK) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) wg_split8(ra[cur ^ 1][i][0], ra[cur ^ 1][i][1], ah[cur ^ 1][i], al[cur ^ 1][i]);
                }
            }
            commit(slot ^ 1);   // B planes of stage it + 1 (nobody reads that buffer before the next barrier)
            slot ^= 1;
        }
        wg_wait_vm<0>();
        int m0e = m0, n0e = n0;
        wg_opaque_origin(m0e, n0e);
        wg_add_tile(acc, pgw_, p.M, p.N, m0e, n0e, wm, wn, l31, kk);
    }   // parts
}

template <int WM, int WN, int TM, int TN>
static void launch_gemm_wgrad_dma_impl(GemmWgradParams& p, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    p.n_stages = (int)(p.total / 32);
    const size_t lds = wg_impl_lds(BM, BN);
    // (see launch_gemm_wgrad_dma); the narrow tiles, of which two fit a CU, at two workgroups per CU
    const int per_cu = 2 * lds <= 160 * 1024 ? 2 : 1;
    const int S = wg_split_workgroups(wg_tiles(p, BM, BN), p.G > 0 ? p.G : 1, p.n_stages, 256 * per_cu);
    auto kern = gemm_wgrad_dma_impl_kernel<WM, WN, TM, TN>;
    static_assert(wg_sole_argument(decltype(kern){}), "wg_operands_kernarg reads p from the kernel-argument segment");
    wg_launch(kern, p, BM, BN, 64 * WM * WN, S, 1, lds, s);
}

template <int WM, int WN, int TM, int TN, int KP, int IMPL = 0>
static void launch_gemm_wgrad(GemmWgradParams& p, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    p.n_stages = (int)((p.total + KP - 1) / KP);
    // K split: every workgroup ends with BM x BN float atomics into the SAME gw tile, and the chip retires only ~1.3 TB/s
    // of atomic bytes -- 1024 workgroups x 64 KB is 50 us of atomics on a problem whose GEMM takes 10.  So: as many
    // workgroups as the CUs can hold at once (8-wave tiles: one per CU, 4-wave: two), and at least 4 stages each.
    const int G = p.G > 0 ? p.G : 1;
    int S = (WM * WN == 8 ? 256 : 512) / (wg_tiles(p, BM, BN) * G);
    if (S > p.n_stages / 4) S = p.n_stages / 4;
    if (S < 1) S = 1;
    wg_launch(gemm_wgrad_b3_kernel<WM, WN, TM, TN, KP, IMPL>, p, BM, BN, 64 * WM * WN, S, G,
              (size_t)2 * (BM + BN) * (KP / 8 + 1) * 16, s);
}

// ---- kernel choice: choose_gemm_wgrad / choose_wgrad_implicit map a shape to a route (and launch nothing),
// launch_wgrad_route is the only place a route is mapped to a launch, the label queries of the C ABI read the same table.
// Instantiations: gemm_wgrad_dma_kernel<WM,WN,TM,TN,KP,NST>, gemm_wgrad_b3_kernel<WM,WN,TM,TN,KP[,IMPL]>.
enum WgradB3Route { DMA_256x256, DMA_64x256, R_256x192, R_256x256, R_64x256, R_256x64, R_128x128, IMPL_DMA_256x192,
                    IMPL_256x192, IMPL_32x256, IMPL_128x128, IMPL_DMA_256x64, IMPL_DMA_256x128, ROWS4_128x128,
                    ROWS2_128x128 };
static const char* const kWgradB3Labels[] = {
    "gemm_wgrad_dma_kernel<2,4,4,2,32,2>",   // 256 x 256, two slots of 64 KB
    "gemm_wgrad_dma_kernel<1,8,2,1,32,3>",   // 64 x 256, ring of 3 x 40 KB
    "gemm_wgrad_b3_kernel<4,2,2,3,64>",      // 256 x 192, 8 waves, 64-pixel stages
    "gemm_wgrad_b3_kernel<2,4,4,2,64>",      // 256 x 256, 8 waves, 64-pixel stages
    "gemm_wgrad_b3_kernel<1,4,2,2,32>",      // 64 x 256
    "gemm_wgrad_b3_kernel<4,1,2,2,32>",      // 256 x 64
    "gemm_wgrad_b3_kernel<2,2,2,2,64>",      // 128 x 128
    "gemm_wgrad_dma_impl_kernel<4,2,2,3>",   // implicit 3x3: 256 x 192, 8 waves, A through the DMA ring
    "gemm_wgrad_b3_kernel<4,2,2,3,64,1>",    // 256 x 192, 8 waves
    "gemm_wgrad_b3_kernel<1,4,1,2,32,1>",    // 32 x 256
    "gemm_wgrad_b3_kernel<2,2,2,2,64,1>",    // 128 x 128
    "gemm_wgrad_dma_impl_kernel<4,2,2,1>",   // implicit 3x3, narrow: 256 x 64, two workgroups per CU (mirrored conv3, C = 4)
    "gemm_wgrad_dma_impl_kernel<4,2,2,2>",   // 256 x 128 (mirrored conv3, C = 8)
    "gemm_wgrad_b3_kernel<2,2,2,2,64,2>",    // short rows, W == 4: 128 x 128 (both orientations)
    "gemm_wgrad_b3_kernel<2,2,2,2,64,3>",    // short rows, 2 x 2 maps
};
static_assert(sizeof(kWgradB3Labels) / sizeof(kWgradB3Labels[0]) == ROWS2_128x128 + 1, "one label per route");
static bool wgrad_dma_off() {
    static const int off = getenv("RFN_WGRAD_DMA") ? atoi(getenv("RFN_WGRAD_DMA")) == 0 : 0;
    return off;
}
// the shape fields of p both choices read: M, N, a_ns, b_ns, G (0: ungrouped), total, HW
static GemmWgradParams wgrad_shape(int M, int Nc, long a_ns, long b_ns, int G, int F, int HW) {
    GemmWgradParams p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = Nc; p.a_ns = a_ns; p.b_ns = b_ns; p.G = G; p.F = F; p.HW = HW; p.total = (long)F * HW;
    return p;
}

static WgradB3Route choose_gemm_wgrad(const GemmWgradParams& p) {
    const int M = p.M, Nc = p.N;
    // the LDS-DMA kernels take a plain (1x1-form) gradient -- or a group of them: the K gradients of a level together are
    // the problem size -- over whole 32-pixel stages
    if (!wgrad_dma_off() && p.HW % 32 == 0 && p.total * (p.G > 0 ? p.G : 1) >= 100000 && p.total >= 2048 &&
        p.a_ns % 4 == 0 && p.b_ns % 4 == 0 && Nc > 128 && Nc % 256 == 0) {
        if (M >= 192) return DMA_256x256;
        if (M <= 64) return DMA_64x256;
    }
    if (M > 128 && Nc > 128 && p.total >= 100000)
        return ceil_div(Nc, 192) * 192 < ceil_div(Nc, 256) * 256 ? R_256x192 : R_256x256;
    return M <= 64 ? R_64x256 : (Nc <= 64 ? R_256x64 : R_128x128);
}
extern "C" const char* rfn_gemm_wgrad_kernel_label_bf16x3(int M, int Nc, long a_ns, long b_ns, int G, int F, int HW) {
    return kWgradB3Labels[choose_gemm_wgrad(wgrad_shape(M, Nc, a_ns, b_ns, G, F, HW))];
}

// 3x3 weight gradient without the im2col buffer (rfn_conv3x3_wgrad_implicit_bf16x3 below): M = Cout, a = the gradient
static WgradB3Route choose_wgrad_implicit(const GemmWgradParams& p) {
    // (grouped: the K gradients of a level together are the problem size)
    if (p.M > 128 && p.total * (p.G > 0 ? p.G : 1) >= 100000 && p.total >= 2048 && !wgrad_dma_off() && p.HW % 32 == 0 &&
        p.a_ns % 4 == 0)
        return IMPL_DMA_256x192;
    if (p.M > 128 && p.total >= 100000) return IMPL_256x192;
    // few output channels (the 16- / 32-channel blocks of the extractor / upscaler on 64x64 and 32x32 maps): one 32-row
    // tile instead of 128 rows of which 16 are real (the clamped rows were 8x the loads and MFMAs of the gradient)
    return p.M <= 32 && p.G == 0 ? IMPL_32x256 : IMPL_128x128;
}
extern "C" const char* rfn_conv3x3_wgrad_implicit_kernel_label_bf16x3(int Cout, long g_ns, int G, int F, int H, int W) {
    return kWgradB3Labels[choose_wgrad_implicit(wgrad_shape(Cout, 0, g_ns, 0, G, F, H * W))];
}

// Mirrored form (rfn_conv3x3_wgrad_mirrored_bf16x3 below): the weight gradient of a 3x3 conv with FEW outputs (the last
// conv of a coupling net, 256 -> C): M = Cin rows of the conv's input h through the ring, the C gradient planes as the
// shifted operand, 9 C columns.  false: the shape has no mirrored route (rows of the map that are no multiple of 8
// pixels) and the caller expands the gradient in HBM as before.
static bool choose_wgrad_implicit_mirrored(const GemmWgradParams& p, WgradB3Route& r) {
    if (p.W % 8 != 0) return false;
    if (p.M > 128 && p.total * (p.G > 0 ? p.G : 1) >= 100000 && p.total >= 2048 && !wgrad_dma_off() && p.HW % 32 == 0 &&
        p.a_ns % 4 == 0) {
        // a column tile that fits 9 C: 36 -> 64, 72 -> 128 (8 waves; a 4-wave 256 x 96 tile was 5 % slower), 144 -> 192
        r = p.N <= 64 ? IMPL_DMA_256x64 : (p.N <= 128 ? IMPL_DMA_256x128 : IMPL_DMA_256x192);
        return true;
    }
    r = p.M > 128 && p.total >= 100000 ? IMPL_256x192 : IMPL_128x128;
    return true;
}
extern "C" const char* rfn_conv3x3_wgrad_mirrored_kernel_label_bf16x3(int Cin, long h_ns, int C, int G, int F, int H,
                                                                      int W) {
    GemmWgradParams p = wgrad_shape(Cin, 9 * C, h_ns, 0, G, F, H * W);
    p.H = H; p.W = W;
    WgradB3Route r;
    return choose_wgrad_implicit_mirrored(p, r) ? kWgradB3Labels[r] : "";
}

// Short-row forms (rfn_conv3x3_wgrad_rows[_mirrored]_bf16x3 below): 4-pixel rows and 2 x 2 maps, which the entry points
// above refuse -- the 128 x 128 tile these shapes took as plain GEMMs, the shifted operand built from halves of a unit
// (wg_shift_split4).  One route per staging form, both orientations; "": the staging does not cover the map.
static bool choose_wgrad_rows(const GemmWgradParams& p, WgradB3Route& r) {
    if (!wg_rows_covers(p.H, p.W)) return false;
    r = wg_rows_impl(p.W) == WG_ROWS4 ? ROWS4_128x128 : ROWS2_128x128;
    return true;
}
static const char* wgrad_rows_label(int H, int W) {
    GemmWgradParams p = wgrad_shape(0, 0, 0, 0, 0, 0, H * W);
    p.H = H; p.W = W;
    WgradB3Route r;
    return choose_wgrad_rows(p, r) ? kWgradB3Labels[r] : "";
}
extern "C" const char* rfn_conv3x3_wgrad_rows_kernel_label_bf16x3(int Cout, long g_ns, int G, int F, int H, int W) {
    return wgrad_rows_label(H, W);
}
extern "C" const char* rfn_conv3x3_wgrad_rows_mirrored_kernel_label_bf16x3(int Cin, long h_ns, int C, int G, int F, int H,
                                                                           int W) {
    return wgrad_rows_label(H, W);
}

// K split of the grouped ring launches, as queries that launch nothing: the workgroups per output tile the launchers
// start, and the parts (group, first stage, count) of workgroup w of Wt -- the very functions the kernels run
extern "C" int rfn_wgrad_split_workgroups(int tiles, int G, int n_stages) {
    RFN_CHECK_ARG(tiles >= 1 && G >= 1 && G <= 16 && n_stages >= 1, -1);
    return wg_split_workgroups(tiles, G, n_stages);
}
extern "C" int rfn_wgrad_split_parts(int G, int n_stages, int Wt, int w, long long* parts, int max_parts) {
    RFN_CHECK_ARG(G >= 1 && G <= 16 && n_stages >= 1 && Wt >= 1 && w >= 0 && w < Wt && (parts || max_parts == 0), -1);
    int n = 0;
    WgPart part;
    for (long pos = wg_split_begin(G, n_stages, Wt, w); wg_split_part(G, n_stages, Wt, w, pos, part); ++n)
        if (n < max_parts) {
            parts[3 * n] = part.grp;
            parts[3 * n + 1] = part.s0;
            parts[3 * n + 2] = part.cnt;
        }
    return n;
}

static void launch_wgrad_route(GemmWgradParams& p, WgradB3Route r, hipStream_t s) {
    switch (r) {
        case DMA_256x256:      return launch_gemm_wgrad_dma<2, 4, 4, 2, 32, 2>(p, s);
        case DMA_64x256:       return launch_gemm_wgrad_dma<1, 8, 2, 1, 32, 3>(p, s);
        case R_256x192:        return launch_gemm_wgrad<4, 2, 2, 3, 64>(p, s);
        case R_256x256:        return launch_gemm_wgrad<2, 4, 4, 2, 64>(p, s);
        case R_64x256:         return launch_gemm_wgrad<1, 4, 2, 2, 32>(p, s);
        case R_256x64:         return launch_gemm_wgrad<4, 1, 2, 2, 32>(p, s);
        case R_128x128:        return launch_gemm_wgrad<2, 2, 2, 2, 64>(p, s);
        case IMPL_DMA_256x192: return launch_gemm_wgrad_dma_impl<4, 2, 2, 3>(p, s);
        case IMPL_256x192:     return launch_gemm_wgrad<4, 2, 2, 3, 64, 1>(p, s);
        case IMPL_32x256:      return launch_gemm_wgrad<1, 4, 1, 2, 32, 1>(p, s);
        case IMPL_128x128:     return launch_gemm_wgrad<2, 2, 2, 2, 64, 1>(p, s);
        case IMPL_DMA_256x64:  return launch_gemm_wgrad_dma_impl<4, 2, 2, 1>(p, s);
        case IMPL_DMA_256x128: return launch_gemm_wgrad_dma_impl<4, 2, 2, 2>(p, s);
        case ROWS4_128x128:    return launch_gemm_wgrad<2, 2, 2, 2, 64, WG_ROWS4>(p, s);
        case ROWS2_128x128:    return launch_gemm_wgrad<2, 2, 2, 2, 64, WG_ROWS2>(p, s);
    }
}

// The parameter block of every entry point below: wgrad_shape plus the operands of the max(G, 1) gradients, as the group
// tables and their group-0 mirrors p.a / p.b / p.b2 / p.gw -- which are all a kernel reads when G == 0 (the single forms
// pass the address of their one pointer).  b2: second source of an implicit B operand; nullptr = b (the GEMM kernels
// never read it).  The implicit forms add b2_ns, C1, C2, H, W and `mirror` themselves.
static GemmWgradParams wgrad_params(int G, const float* const* a, long a_ns, int M, const float* const* b, long b_ns,
                                    const float* const* b2, int Nc, float* const* gw, int F, int HW) {
    GemmWgradParams p = wgrad_shape(M, Nc, a_ns, b_ns, G, F, HW);
    for (int g = 0; g < (G > 0 ? G : 1); ++g) {
        p.ga[g] = a[g]; p.gb[g] = b[g]; p.gb2[g] = b2 ? b2[g] : b[g]; p.ggw[g] = gw[g];
    }
    p.a = p.ga[0]; p.b = p.gb[0]; p.b2 = p.gb2[0]; p.gw = p.ggw[0];
    return p;
}

// ---- entry points.  Each single / grouped pair shares one body: the single form passes G = 0 and the address of its
// one pointer per operand, after the null check of those pointers (-1; a group's null pointer is a -3 of the grouped
// form, which checks G itself).  The body's checks run in the order of the codes: -1 sizes and tables, -2 pixel counts
// and strides the 16-byte loads cannot take, -3 the operands of every group (non-null, inputs 16-byte aligned), -4 the
// 32-bit pixel index; then F == 0 returns 0 -- all before the kernel choice and the launch.
static bool wg_aligned16(const float* x, const float* y, const float* z = nullptr) {
    return (((uintptr_t)x | (uintptr_t)y | (uintptr_t)z) & 15) == 0;
}

static int rfn_gemm_wgrad_bf16x3_body(int G, const float* const* a, long a_ns, int M, const float* const* b, long b_ns,
                                      int Nc, float* const* gw, int F, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(a && b && gw && M > 0 && Nc > 0 && F >= 0 && HW > 0, -1);
    RFN_CHECK_ARG(HW % 4 == 0 && a_ns % 4 == 0 && b_ns % 4 == 0, -2);
    for (int g = 0; g < (G > 0 ? G : 1); ++g) RFN_CHECK_ARG(a[g] && b[g] && gw[g] && wg_aligned16(a[g], b[g]), -3);
    RFN_CHECK_ARG((long)F * HW < (1L << 31) - 4096, -4);
    if (F == 0) return 0;
    GemmWgradParams p = wgrad_params(G, a, a_ns, M, b, b_ns, nullptr, Nc, gw, F, HW);
    launch_wgrad_route(p, choose_gemm_wgrad(p), (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_gemm_wgrad_bf16x3(const float* a, long a_ns, int M, const float* b, long b_ns, int Nc, float* gw,
                                     int F, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(a && b && gw, -1);
    return rfn_gemm_wgrad_bf16x3_body(0, &a, a_ns, M, &b, b_ns, Nc, &gw, F, HW, stream);
}
// G (<= 16) weight gradients of one shape in ONE launch: gw[g][M][Nc] += sum a[g] b[g]^T (same strides, F, HW for all).
extern "C" int rfn_gemm_wgrad_grouped_bf16x3(const float* const* a, long a_ns, int M, const float* const* b, long b_ns,
                                             int Nc, float* const* gw, int G, int F, int HW, rfn_stream_t stream) {
    RFN_CHECK_ARG(G >= 1 && G <= 16, -1);
    return rfn_gemm_wgrad_bf16x3_body(G, a, a_ns, M, b, b_ns, Nc, gw, F, HW, stream);
}

// 3x3 weight gradient without the im2col buffer: gw[co][ci][tap] = sum_{frames,pixels} g[co][px] * in[ci][px + tap]
// (pad 1), the shifted planes built while staging (rows of one image row, W % 8 == 0).  The output is the torch weight
// layout [Cout][Cin][3][3] (the GEMM on rfn_im2col3x3_f32's buffer gives [Cout][tap][Cin] instead).  Per group: g, in1,
// in2 (ignored when C2 == 0), gw.  (H <= 0 or W <= 0 alone is a -1 of the single and a -2 of the grouped form.)
static int rfn_conv3x3_wgrad_implicit_bf16x3_body(int G, const float* const* g, long g_ns, int Cout,
                                                  const float* const* in1, long in1_ns, int C1, const float* const* in2,
                                                  long in2_ns, int C2, float* const* gw, int F, int H, int W,
                                                  rfn_stream_t stream, bool rows = false) {
    RFN_CHECK_ARG(g && in1 && gw && Cout > 0 && C1 > 0 && C2 >= 0 && (C2 == 0 || in2) && F >= 0, -1);
    RFN_CHECK_ARG(H > 0 && W > 0, G > 0 ? -2 : -1);
    RFN_CHECK_ARG((rows ? wg_rows_covers(H, W) : W % 8 == 0) && g_ns % 4 == 0 && in1_ns % 4 == 0 &&
                      (C2 == 0 || in2_ns % 4 == 0), -2);
    for (int i = 0; i < (G > 0 ? G : 1); ++i)
        RFN_CHECK_ARG(g[i] && in1[i] && gw[i] && (C2 == 0 || in2[i]) && wg_aligned16(g[i], in1[i], C2 ? in2[i] : in1[i]),
                      -3);
    RFN_CHECK_ARG((long)F * H * W < (1L << 31) - 4096, -4);
    if (F == 0) return 0;
    GemmWgradParams p = wgrad_params(G, g, g_ns, Cout, in1, in1_ns, C2 ? in2 : nullptr, 9 * (C1 + C2), gw, F, H * W);
    p.b2_ns = C2 ? in2_ns : in1_ns; p.C1 = C1; p.C2 = C2; p.H = H; p.W = W;
    WgradB3Route r = rows ? ROWS4_128x128 : choose_wgrad_implicit(p);
    if (rows) choose_wgrad_rows(p, r);
    launch_wgrad_route(p, r, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_conv3x3_wgrad_implicit_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                                 const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                                 rfn_stream_t stream) {
    RFN_CHECK_ARG(g && in1 && gw && (C2 <= 0 || in2), -1);
    return rfn_conv3x3_wgrad_implicit_bf16x3_body(0, &g, g_ns, Cout, &in1, in1_ns, C1, &in2, in2_ns, C2, &gw, F, H, W,
                                                  stream);
}
extern "C" int rfn_conv3x3_wgrad_implicit_grouped_bf16x3(const float* const* g, long g_ns, int Cout,
                                                         const float* const* in1, long in1_ns, int C1,
                                                         const float* const* in2, long in2_ns, int C2, float* const* gw,
                                                         int G, int F, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(G >= 1 && G <= 16, -1);
    return rfn_conv3x3_wgrad_implicit_bf16x3_body(G, g, g_ns, Cout, in1, in1_ns, C1, in2, in2_ns, C2, gw, F, H, W, stream);
}

// 3x3 weight gradient of a conv with few outputs, without the tap-scattered gradient buffer: the roles of the implicit
// form swapped and the taps mirrored (GemmWgradParams::mirror).  gwT[ci][co][tap] = sum_{frames,pixels} h[ci][q] *
// g[co][q - tap] = gw[co][ci][tap]: the TRANSPOSE of the torch layout, [Cin][C][3][3].  Per group: h, g, gwT.  Every
// shape that passes the checks has a mirrored route (choose_wgrad_implicit_mirrored refuses only W % 8 != 0).
static int rfn_conv3x3_wgrad_mirrored_bf16x3_body(int G, const float* const* h, long h_ns, int Cin,
                                                  const float* const* g, long g_ns, int C, float* const* gwT, int F, int H,
                                                  int W, rfn_stream_t stream, bool rows = false) {
    RFN_CHECK_ARG(h && g && gwT && Cin > 0 && C > 0 && F >= 0, -1);
    RFN_CHECK_ARG(H > 0 && W > 0, G > 0 ? -2 : -1);
    RFN_CHECK_ARG((rows ? wg_rows_covers(H, W) : W % 8 == 0) && h_ns % 4 == 0 && g_ns % 4 == 0, -2);
    for (int i = 0; i < (G > 0 ? G : 1); ++i) RFN_CHECK_ARG(h[i] && g[i] && gwT[i] && wg_aligned16(h[i], g[i]), -3);
    RFN_CHECK_ARG((long)F * H * W < (1L << 31) - 4096, -4);
    if (F == 0) return 0;
    GemmWgradParams p = wgrad_params(G, h, h_ns, Cin, g, g_ns, nullptr, 9 * C, gwT, F, H * W);
    p.b2_ns = g_ns; p.C1 = C; p.H = H; p.W = W; p.mirror = 1;
    WgradB3Route r = IMPL_128x128;
    if (rows) choose_wgrad_rows(p, r);
    else choose_wgrad_implicit_mirrored(p, r);
    launch_wgrad_route(p, r, (hipStream_t)stream);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_conv3x3_wgrad_mirrored_bf16x3(const float* h, long h_ns, int Cin, const float* g, long g_ns, int C,
                                                 float* gwT, int F, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(h && g && gwT, -1);
    return rfn_conv3x3_wgrad_mirrored_bf16x3_body(0, &h, h_ns, Cin, &g, g_ns, C, &gwT, F, H, W, stream);
}
extern "C" int rfn_conv3x3_wgrad_mirrored_grouped_bf16x3(const float* const* h, long h_ns, int Cin, const float* const* g,
                                                         long g_ns, int C, float* const* gwT, int G, int F, int H, int W,
                                                         rfn_stream_t stream) {
    RFN_CHECK_ARG(G >= 1 && G <= 16, -1);
    return rfn_conv3x3_wgrad_mirrored_bf16x3_body(G, h, h_ns, Cin, g, g_ns, C, gwT, F, H, W, stream);
}

// The two forms above on maps with rows shorter than a staging unit: 4-pixel rows (H even) and 2 x 2 maps, the shifted
// operand built from halves of a unit (gemm_wgrad_b3_kernel<..., WG_ROWS4 / WG_ROWS2>).  Same arguments, checks and
// output layouts; -2 for every other map.
extern "C" int rfn_conv3x3_wgrad_rows_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                             const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                             rfn_stream_t stream) {
    RFN_CHECK_ARG(g && in1 && gw && (C2 <= 0 || in2), -1);
    return rfn_conv3x3_wgrad_implicit_bf16x3_body(0, &g, g_ns, Cout, &in1, in1_ns, C1, &in2, in2_ns, C2, &gw, F, H, W,
                                                  stream, true);
}
extern "C" int rfn_conv3x3_wgrad_rows_grouped_bf16x3(const float* const* g, long g_ns, int Cout, const float* const* in1,
                                                     long in1_ns, int C1, const float* const* in2, long in2_ns, int C2,
                                                     float* const* gw, int G, int F, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(G >= 1 && G <= 16, -1);
    return rfn_conv3x3_wgrad_implicit_bf16x3_body(G, g, g_ns, Cout, in1, in1_ns, C1, in2, in2_ns, C2, gw, F, H, W, stream,
                                                  true);
}
extern "C" int rfn_conv3x3_wgrad_rows_mirrored_bf16x3(const float* h, long h_ns, int Cin, const float* g, long g_ns, int C,
                                                      float* gwT, int F, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(h && g && gwT, -1);
    return rfn_conv3x3_wgrad_mirrored_bf16x3_body(0, &h, h_ns, Cin, &g, g_ns, C, &gwT, F, H, W, stream, true);
}
extern "C" int rfn_conv3x3_wgrad_rows_mirrored_grouped_bf16x3(const float* const* h, long h_ns, int Cin,
                                                              const float* const* g, long g_ns, int C, float* const* gwT,
                                                              int G, int F, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(G >= 1 && G <= 16, -1);
    return rfn_conv3x3_wgrad_mirrored_bf16x3_body(G, h, h_ns, Cin, g, g_ns, C, gwT, F, H, W, stream, true);
}

// ------------------------------------------------------------------------------------------------ band kernel
// 3x3 weight gradients whose BOTH channel counts are small (the extractor / upscaler blocks, 16 .. 128 channels on
// 64 x 64 .. 8 x 8 maps): gemm_wgrad_b3_kernel<..., IMPL = 1> fetches every input pixel nine times, once per row
// (ci, tap) of its B operand, and the Cin > Cout layers expand the gradient ninefold in HBM first.  Here the unit of work
// is a BAND, R consecutive image rows of one frame (R | H, R W % 16 == 0): a workgroup stages the band of g (its Cout
// planes) and the band of the input with one halo row above and below (zero beyond the frame) ONCE, split to bf16
// (hi, lo) on the way into LDS, and every shifted operand is LDS addressing:
//   * a dy shift is a row offset;
//   * the three dx shifts are three staged copies of the input band, zero beyond the row ends, so a B fragment of column
//     n = ci*9 + tap is ONE aligned 16-byte read of 8 consecutive pixels: copy tap % 3, plane ci, row y + tap / 3;
//   * strides (16-byte units): rows RSU = W/8 | 1, planes PS = 9a, copies CS = a (mod 16) with a = 11 RSU (3a = RSU):
//     column n reads unit a n + const (mod 16), a odd, so the 16 lanes of a ds_read_b128 group (16 consecutive n mod 16)
//     hit 16 different 16-byte slots of the 256-byte bank row.  The gradient's rows have an odd stride for the same reason.
// K = the band's pixels: the four waves of a workgroup take the 16-pixel k-steps of a band in turn and each keeps ALL
// MT x NTC accumulator tiles (every fragment is read from LDS by exactly one wave).  Workgroups are persistent, two per
// CU (one stages while the other multiplies): each walks a contiguous range of the (frame, band) units with its
// accumulators in registers, then the four waves' tiles are summed through LDS and flushed with float atomics once.
// PF: the loads of the next band's first staging round are issued ahead of the MFMAs of the current band and committed
// after them (one row tile: 0.164 -> 0.128 ms for 16 x 144 on 640 frames of 64 x 64); with two row tiles the 160
// accumulator registers leave no room for the round (it spilled), and the second workgroup of the CU is the only overlap.
// Columns are split by whole input channels over blockIdx.y (CPB channels, 9 CPB <= 32 NTC columns: a block stages only
// its planes), rows of more than 32 MT output channels over blockIdx.z.  Both orientations (Cin <= Cout, Cin > Cout)
// are the same problem; the output is the torch layout [Cout][Cin][3][3].
struct WgBandGeom {
    int R, CPB;                  // rows per band, input channels per column block
    int WU, RSU, PS, CS, AS;     // 16-byte units: per image row, strides of staged rows / planes / copies, of a g row
    int Arows;                   // gradient rows a block stages
    size_t lds;
};
struct WgBandParams {
    const float* g; const float* in1; const float* in2;
    float* gw;
    long g_ns, in1_ns, in2_ns;
    int Cout, C1, C2, F, H, W;
    int nbands, units;           // bands per frame, F * nbands
    WgBandGeom q;
};
constexpr int WG_BAND_NTC = 5, WG_BAND_CPB = 32 * WG_BAND_NTC / 9;   // 16 channels = 144 of 160 columns
constexpr size_t WG_BAND_LDS_MAX = 79 * 1024;                         // two workgroups per CU
constexpr size_t WG_BAND_RED = 4 * 16 * 64 * sizeof(float);           // the flush's scratch: one tile of four waves
constexpr int wg_band_pad16(int x, int r) { return x + ((r - x % 16) + 16) % 16; }   // smallest y >= x, y % 16 == r
// LDS image of a block: a constexpr function of (channels per column block, gradient rows, W, R)
constexpr WgBandGeom wg_band_geom(int cpb, int arows, int W, int R) {
    WgBandGeom q{};
    q.R = R; q.CPB = cpb; q.Arows = arows;
    q.WU = W / 8;
    q.RSU = q.WU | 1;
    const int a = 11 * q.RSU % 16;
    q.PS = wg_band_pad16((R + 2) * q.RSU, 9 * a % 16);
    q.CS = wg_band_pad16(cpb * q.PS, a);
    q.AS = (R * q.WU) | 1;
    q.lds = (size_t)16 * (2 * arows * q.AS + 6 * q.CS);
    if (q.lds < WG_BAND_RED) q.lds = WG_BAND_RED;
    return q;
}
static_assert(wg_band_geom(16, 16, 64, 2).lds <= WG_BAND_LDS_MAX, "16 channels of a 64-pixel-wide map: two rows per band");
// row tiles per block (MT), and the geometry: the most channels per column block (at most WG_BAND_CPB, evenly over the
// blocks), then the tallest band whose image fits two workgroups per CU.  false: no band fits, or W % 8 != 0.
static bool wg_band_choose(int Cout, int Cin, int H, int W, int& mt, WgBandGeom& q) {
    if (Cout < 1 || Cin < 1 || Cout > 128 || Cin > 128 || H < 1 || W < 8 || W % 8 != 0) return false;
    mt = Cout <= 32 ? 1 : 2;
    const int arows = Cout < 32 * mt ? Cout : 32 * mt;
    for (int cap = Cin < WG_BAND_CPB ? Cin : WG_BAND_CPB; cap >= 1; cap /= 2) {
        const int cpb = ceil_div(Cin, ceil_div(Cin, cap));
        for (int R = H; R >= 1; --R) {
            if (H % R != 0 || (R * W) % 16 != 0) continue;
            q = wg_band_geom(cpb, arows, W, R);
            if (q.lds <= WG_BAND_LDS_MAX) return true;
        }
    }
    return false;
}

template <int MT, int NTC, bool PF>
__global__ __launch_bounds__(256, 2) void wgrad_band_kernel(const WgBandParams p) {
    constexpr int NT = 256, U = 2;   // U: units of each operand a thread has in flight per staging round
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const WgBandGeom& q = p.q;
    bf16x8* Ah = reinterpret_cast<bf16x8*>(lds_raw);
    bf16x8* Al = Ah + q.Arows * q.AS;
    bf16x8* Bh = Al + q.Arows * q.AS;
    bf16x8* Bl = Bh + 3 * q.CS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int Cin = p.C1 + p.C2, HW = p.H * p.W;
    const int c0 = blockIdx.y * q.CPB, nch = Cin - c0 < q.CPB ? Cin - c0 : q.CPB;
    const int m0 = blockIdx.z * 32 * MT, mrows = p.Cout - m0 < 32 * MT ? p.Cout - m0 : 32 * MT;
    // my units: a contiguous range (neighbouring bands share their halo rows in L2); none left for the last workgroups
    // when the units do not divide
    const int per = (p.units + (int)gridDim.x - 1) / (int)gridDim.x;
    const int u0 = blockIdx.x * per, u1 = u0 + per < p.units ? u0 + per : p.units;
    if (u0 >= u1) return;

    f32x16 acc[MT][NTC];
    wg_zero(acc);
    // fragment bases: gradient row m (rows beyond the block's take row 0, columns beyond 9 nch column 0; never flushed)
    int aoff[MT], boff[NTC];
#pragma unroll
    for (int i = 0; i < MT; ++i) aoff[i] = (i * 32 + l31 < mrows ? i * 32 + l31 : 0) * q.AS;
#pragma unroll
    for (int j = 0; j < NTC; ++j) {
        const int n = j * 32 + l31 < 9 * nch ? j * 32 + l31 : 0;
        const int ci = n / 9, tap = n - ci * 9;
        boff[j] = (tap % 3) * q.CS + ci * q.PS + (tap / 3) * q.RSU;
    }
    const int PU = q.R * q.WU, nA = mrows * PU;                    // units of the gradient band
    const int perch = (q.R + 2) * q.WU, nB = nch * perch;          // units of the input band with its halo rows
    const int nmax = nA > nB ? nA : nB;

    // One staging round: U units of each operand per thread, unit e = base + k NT.  The loads are unconditional (clamped;
    // the masks apply at the stores) and are not touched before store_round, so a round issued ahead of the MFMAs of the
    // band before stays in flight behind them.
    float4 av[U][2], bv[U][2];
    float bl_[U], br_[U];
    int ao[U], bo[U];
    bool aok[U], bok[U], rok[U];
    auto load_round = [&](const int u, const int base) {
        const int f = u / p.nbands, y0 = (u - f * p.nbands) * q.R;
        const float* gsrc = p.g + (long)f * p.g_ns + (long)m0 * HW + y0 * p.W;
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int e = base + k * NT;
            aok[k] = e < nA;
            const int ee = aok[k] ? e : 0;
            const int co = ee / PU, pu = ee - co * PU;
            const float* src = gsrc + (long)co * HW + pu * 8;
            av[k][0] = *reinterpret_cast<const float4*>(src);
            av[k][1] = *reinterpret_cast<const float4*>(src + 4);
            ao[k] = co * q.AS + pu;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int e = base + k * NT;
            bok[k] = e < nB;
            const int ee = bok[k] ? e : 0;
            const int ci = ee / perch, r = ee - ci * perch;
            const int rr = r / q.WU, xg = r - rr * q.WU;
            const int yy = y0 - 1 + rr, cg = c0 + ci;
            rok[k] = yy >= 0 && yy < p.H;
            const float* plane = cg < p.C1 ? p.in1 + (long)f * p.in1_ns + (long)cg * HW
                                           : p.in2 + (long)f * p.in2_ns + (long)(cg - p.C1) * HW;
            const float* src = plane + (rok[k] ? yy : y0) * p.W + xg * 8;
            bv[k][0] = *reinterpret_cast<const float4*>(src);
            bv[k][1] = *reinterpret_cast<const float4*>(src + 4);
            // the elements beyond the 8, clamped into them where the image row ends (rok then also clears them)
            bl_[k] = src[xg > 0 ? -1 : 0];
            br_[k] = src[xg + 1 < q.WU ? 8 : 7];
            bo[k] = (ci * q.PS + rr * q.RSU + xg) | (xg > 0 ? 0 : 1 << 30) | (xg + 1 < q.WU ? 0 : 1 << 29);
        }
    };
    auto store_round = [&]() {
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (aok[k]) {
                bf16x8 hi, lo;
                wg_split8(f32x4{av[k][0].x, av[k][0].y, av[k][0].z, av[k][0].w},
                          f32x4{av[k][1].x, av[k][1].y, av[k][1].z, av[k][1].w}, hi, lo);
                Ah[ao[k]] = hi;
                Al[ao[k]] = lo;
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (bok[k]) {
                // the 10 pixels x - 1 .. x + 8 split once; copy d holds pixels d .. d + 7 of them: in[x + d - 1]
                const int o = bo[k] & 0xFFFFFF;
                const float v[10] = {(bo[k] >> 30) & 1 ? 0.f : bl_[k], bv[k][0].x, bv[k][0].y, bv[k][0].z, bv[k][0].w,
                                     bv[k][1].x, bv[k][1].y, bv[k][1].z, bv[k][1].w, (bo[k] >> 29) & 1 ? 0.f : br_[k]};
                __bf16 h[10], l[10];
#pragma unroll
                for (int c = 0; c < 10; ++c) {
                    const float x = rok[k] ? v[c] : 0.f;
                    h[c] = (__bf16)x;
                    l[c] = (__bf16)(x - (float)h[c]);
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    bf16x8 hi, lo;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        hi[c] = h[c + d];
                        lo[c] = l[c + d];
                    }
                    Bh[d * q.CS + o] = hi;
                    Bl[d * q.CS + o] = lo;
                }
            }
        }
    };

    if (PF) load_round(u0, tid);
    for (int u = u0; u < u1; ++u) {
        __syncthreads();   // everybody has left the previous band's fragments
        if (PF) store_round();
        for (int b0 = PF ? NT * U : 0; b0 < nmax; b0 += NT * U) {   // (PF: the rounds after the first, not ahead)
            load_round(u, b0 + tid);
            store_round();
        }
        __syncthreads();
        if (PF) {   // the next band's first round, in flight behind this band's MFMAs (past the end: this band again, unused)
            load_round(u + 1 < u1 ? u + 1 : u, tid);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the band's k-steps of 16 pixels, wave w the steps w, w + 4, ...: lane (l31, kk) reads pixel group 2 s + kk
        for (int s = wave; 2 * s < PU; s += 4) {
            const int pg = 2 * s + kk;
            const int yl = pg / q.WU, xg = pg - yl * q.WU;
            const int ko = yl * q.RSU + xg;
            bf16x8 ah[MT], al[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ah[i] = Ah[aoff[i] + pg];
                al[i] = Al[aoff[i] + pg];
            }
#pragma unroll
            for (int j = 0; j < NTC; ++j) {
                const bf16x8 bh = Bh[boff[j] + ko], bl = Bl[boff[j] + ko];
#pragma unroll
                for (int i = 0; i < MT; ++i) wg_mfma3(acc[i][j], ah[i], al[i], bh, bl);
            }
        }
    }

    // flush: per tile, the four waves' copies through LDS -- wave w adds registers 4w .. 4w + 3 of all four -- and one
    // float atomic per real output
    float* red = reinterpret_cast<float*>(lds_raw);   // [wave][register][lane]
    const int Nc = 9 * Cin;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTC; ++j) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[i][j][r];
            __syncthreads();
            const int n = j * 32 + l31;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int r = wave * 4 + t;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) sum += red[(w * 16 + r) * 64 + lane];
                const int m = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (m < mrows && n < 9 * nch) atomicAdd(&p.gw[(long)(m0 + m) * Nc + 9 * c0 + n], sum);
            }
        }
}

static const char* const kWgradBandLabels[2] = {"wgrad_band_kernel<1,5,1>", "wgrad_band_kernel<2,5,0>"};
extern "C" int rfn_conv3x3_wgrad_band_supported(int Cout, int Cin, int H, int W) {
    int mt;
    WgBandGeom q;
    return wg_band_choose(Cout, Cin, H, W, mt, q) ? 1 : 0;
}
extern "C" const char* rfn_conv3x3_wgrad_band_kernel_label_bf16x3(int Cout, int Cin, int F, int H, int W) {
    int mt;
    WgBandGeom q;
    return wg_band_choose(Cout, Cin, H, W, mt, q) ? kWgradBandLabels[mt - 1] : "";
}
// the launch geometry, for the tests and the benchmark: {R, CPB, grid x, y, z, LDS bytes}; 0, or -2 as the entry point
extern "C" int rfn_conv3x3_wgrad_band_geometry(int Cout, int Cin, int F, int H, int W, long long* out6) {
    int mt;
    WgBandGeom q;
    RFN_CHECK_ARG(out6 && F >= 1, -1);
    RFN_CHECK_ARG(wg_band_choose(Cout, Cin, H, W, mt, q), -2);
    const int gy = ceil_div(Cin, q.CPB), gz = ceil_div(Cout, 32 * mt);
    const long units = (long)F * (H / q.R), slots = 512 / (gy * gz) > 1 ? 512 / (gy * gz) : 1;
    out6[0] = q.R; out6[1] = q.CPB; out6[2] = (int)(units < slots ? units : slots); out6[3] = gy; out6[4] = gz;
    out6[5] = (int)q.lds;
    return 0;
}
// The contract of rfn_conv3x3_wgrad_implicit_bf16x3 (two-source input, frame strides, accumulates into the caller's
// zeroed gw, no memset), for every shape rfn_conv3x3_wgrad_band_supported names, however small.
extern "C" int rfn_conv3x3_wgrad_band_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                             const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                             rfn_stream_t stream) {
    RFN_CHECK_ARG(g && in1 && gw && Cout > 0 && C1 > 0 && C2 >= 0 && (C2 == 0 || in2) && F >= 0 && H > 0 && W > 0, -1);
    int mt;
    WgBandParams p{};
    RFN_CHECK_ARG(wg_band_choose(Cout, C1 + C2, H, W, mt, p.q) && g_ns % 4 == 0 && in1_ns % 4 == 0 &&
                      (C2 == 0 || in2_ns % 4 == 0), -2);
    RFN_CHECK_ARG(wg_aligned16(g, in1, C2 ? in2 : in1), -3);
    RFN_CHECK_ARG((long)F * H * W < (1L << 31) - 4096, -4);
    if (F == 0) return 0;
    p.g = g; p.in1 = in1; p.in2 = C2 ? in2 : in1; p.gw = gw;
    p.g_ns = g_ns; p.in1_ns = in1_ns; p.in2_ns = C2 ? in2_ns : in1_ns;
    p.Cout = Cout; p.C1 = C1; p.C2 = C2; p.F = F; p.H = H; p.W = W;
    p.nbands = H / p.q.R;
    p.units = F * p.nbands;
    const int gy = ceil_div(C1 + C2, p.q.CPB), gz = ceil_div(Cout, 32 * mt);
    const int slots = 512 / (gy * gz) > 1 ? 512 / (gy * gz) : 1;   // two workgroups on each of the 256 CUs
    const dim3 grid(p.units < slots ? p.units : slots, gy, gz);
    auto kern = mt == 1 ? wgrad_band_kernel<1, WG_BAND_NTC, true> : wgrad_band_kernel<2, WG_BAND_NTC, false>;
    if (p.q.lds > 65536)
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.q.lds);
    hipLaunchKernelGGL(kern, grid, dim3(256), p.q.lds, (hipStream_t)stream, p);
    RFN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ im2col (3x3, pad 1)
// X9[n][tap*Cin + ci][y][x] = in[n][ci][y+dy-1][x+dx-1] (0 outside), two-source input like the convolutions.
__global__ void im2col3x3_kernel(const float* __restrict__ in1, long in1_ns, int C1, const float* __restrict__ in2,
                                 long in2_ns, int C2, float* __restrict__ out, int N, int H, int W) {
    const int Cin = C1 + C2;
    const long HW = (long)H * W, total = (long)N * 9 * Cin * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        long r = idx / W;
        const int y = (int)(r % H);
        r /= H;
        const int tc = (int)(r % (9 * Cin));
        const long n = r / (9 * Cin);
        const int t = tc / Cin, ci = tc - t * Cin;
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
            v = ci < C1 ? in1[n * in1_ns + (long)ci * HW + (long)yy * W + xx]
                        : in2[n * in2_ns + (long)(ci - C1) * HW + (long)yy * W + xx];
        out[idx] = v;
    }
}
// W % 4 == 0: one thread = 4 consecutive pixels of one (frame, tap*Cin+ci, y) row -> one 16-byte store, the index
// divisions amortised over 4 elements (the element-wise kernel above spends its time in them).
__global__ void im2col3x3_v4_kernel(const float* __restrict__ in1, long in1_ns, int C1, const float* __restrict__ in2,
                                    long in2_ns, int C2, float* __restrict__ out, int N, int H, int W) {
    const int Cin = C1 + C2, HW4 = H * W / 4, W4 = W / 4;
    const long HW = (long)H * W, total = (long)N * 9 * Cin * HW4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int q = (int)(idx % HW4);
        const long r = idx / HW4;
        const int tc = (int)(r % (9 * Cin));
        const long n = r / (9 * Cin);
        const int t = tc / Cin, ci = tc - t * Cin;
        const int y = q / W4, x0 = (q - y * W4) * 4;
        const int yy = y + t / 3 - 1, dx = t % 3 - 1;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < H) {
            const float* src = (ci < C1 ? in1 + n * in1_ns + (long)ci * HW : in2 + n * in2_ns + (long)(ci - C1) * HW) +
                               (long)yy * W;
            if (dx == 0) {
                v = *reinterpret_cast<const float4*>(src + x0);
            } else {
                const float4 c = *reinterpret_cast<const float4*>(src + x0);
                if (dx < 0) {
                    v.x = x0 > 0 ? src[x0 - 1] : 0.f;
                    v.y = c.x; v.z = c.y; v.w = c.z;
                } else {
                    v.x = c.y; v.y = c.z; v.z = c.w;
                    v.w = x0 + 4 < W ? src[x0 + 4] : 0.f;
                }
            }
        }
        *reinterpret_cast<float4*>(out + idx * 4) = v;
    }
}
extern "C" int rfn_im2col3x3_f32(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                                 float* out, int N, int H, int W, rfn_stream_t stream) {
    RFN_CHECK_ARG(in1 && out && C1 > 0 && C2 >= 0 && (C2 == 0 || in2) && N >= 0 && H > 0 && W > 0, -1);
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long HWl = (long)H * W;
    if (W % 4 == 0 && in1_ns % 4 == 0 && (C2 == 0 || in2_ns % 4 == 0) && HWl % 4 == 0 &&
        (((uintptr_t)in1 | (uintptr_t)out | (uintptr_t)(C2 ? in2 : in1)) & 15) == 0) {
        long tot4 = (long)N * 9 * (C1 + C2) * (HWl / 4);
        int grid4 = (int)((tot4 + 255) / 256 < 16384 ? (tot4 + 255) / 256 : 16384);
        hipLaunchKernelGGL(im2col3x3_v4_kernel, dim3(grid4), dim3(256), 0, s, in1, in1_ns, C1, in2, in2_ns, C2, out, N, H, W);
        RFN_LAUNCH_CHECK();
        return 0;
    }
    long tot = (long)N * 9 * (C1 + C2) * H * W;
    int grid = (int)((tot + 255) / 256 < 8192 ? (tot + 255) / 256 : 8192);
    hipLaunchKernelGGL(im2col3x3_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in1, in1_ns, C1, in2, in2_ns, C2,
                       out, N, H, W);
    RFN_LAUNCH_CHECK();
    return 0;
}
