// The two pieces of glue of RFN's importance-weighted bound (RFN.iw_log_weights; DESIGN.md section 24 is the contract).
//
// rfn_latent_iw_f32 -- one latent step of a chain: from the raw outputs [rows, 2*ZHW] of the encoder / prior parameter
// convs (loc half | raw-scale half, rfn_latent_step_fwd_f32's layout) and the posterior eps to the posterior sample and
// the row's log-ratio of prior and posterior density AT that sample:
//   ps = softplus(pri_raw), es = softplus(enc_raw), pm = pri_loc, em = enc_loc (+ pm with res_q)   (nothing added)
//   zxt = em + es*eps                                             (rfn_latent_step_fwd_f32's expression: the same bits)
//   logr[row] = sum_j  -((zxt - pm)/ps)^2 / 2 - log ps + eps^2 / 2 + log es                  (the 2 pi terms cancel)
// Each element's term is evaluated in fp64 on the fp32 values zxt, pm, ps, es, eps and rounded to fp32 once; the sum is
// fp32.  One wavefront per row, RFN_IW_ROWS rows per workgroup, as gauss_heads.hip: lane l takes the elements l, l + 64, ... of
// its row and adds its terms in index order; the 64 lane sums are combined by the xor butterfly of wave_sum (offsets 32,
// 16, ..., 1).  No atomics, no LDS memory: a row's bits depend on that row alone.
//
// rfn_keyed_uniform_f32 -- addressed uniforms (the dequantisation noise of every step of a pass in one launch): out
// [n_steps, rows, numel]; row i of every step-block is draw first_draw + i / B of sequence first_seq + i % B (draw-major,
// as csrc/keyed_normal.hip), step-block s uses step first_step + s.
//   block q of a row = Philox4x64-10(key = (seed, (step << 32) | slot), counter = (q, 0, seq, draw)), words w0..w3
//   (csrc/philox.h); word w_i gives element 8q + 2i from its high half and 8q + 2i + 1 from its low half:
//     value = (half >> 8) * 2^-24 * scale      in [0, scale): the first product is exact, the second rounds once
//   slot >= 8: keyed_normal owns the slots 0..7 of the same key space (mol owns 16 and 17; the callers keep apart).
// One lane per Philox block, eight results per lane: two 16-byte stores where numel % 8 == 0 and the base is 16-byte
// aligned (then every row of every step-block is), single stores for a tail block and for an unaligned base.  A pure
// store stream: no atomics, no LDS.
#include "common.h"
#include "philox.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int RFN_IW_ROWS = 4;  // waves (= rows) per workgroup of 256 threads
constexpr int KU_THREADS = 256;

__global__ void __launch_bounds__(64 * RFN_IW_ROWS)
latent_iw_kernel(const float* __restrict__ enc, const float* __restrict__ pri, const float* __restrict__ eps_q,
                 float* __restrict__ zxt, float* __restrict__ logr, int rows, int ZHW, int res_q) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * RFN_IW_ROWS + (threadIdx.x >> 6);
    if (b >= rows) return;  // whole waves leave: no shuffle below is divergent
    const long in = b * 2 * ZHW, out = b * ZHW;
    float s = 0.f;
    for (int e = lane; e < ZHW; e += 64) {
        const float pm = pri[in + e], ps = softplusf_(pri[in + ZHW + e]);
        const float es = softplusf_(enc[in + ZHW + e]);
        const float em = enc[in + e] + (res_q ? pm : 0.f);
        const float eq = eps_q[out + e];
        const float z = em + es * eq;
        zxt[out + e] = z;
        // the element's term in fp64 on the fp32 quantities above, rounded once: its four parts nearly cancel where the
        // posterior is close to the prior, and fp32 parts would leave an error of the size of the parts, not of the term
        const double d = ((double)z - (double)pm) / (double)ps;
        s += (float)(0.5 * ((double)eq * (double)eq - d * d) + log((double)es / (double)ps));
    }
    s = wave_sum(s);
    if (lane == 0) logr[b] = s;
}

struct KeyedUniformParams {
    float* out;
    int numel, rows, B;
    int vec;                // the 16-byte stores
    long blocks_per_step;   // Philox blocks of one step-block: rows * ceil(numel / 8)
    long items;             // n_steps * blocks_per_step
    float scale;
    uint64_t seed, first_seq, first_draw;
    uint32_t first_step, slot;
};

__device__ __forceinline__ float ku_value(uint32_t half, float scale) {
    return (float)(half >> 8) * 0x1p-24f * scale;   // the integer is below 2^24: exact before the last product
}

__global__ __launch_bounds__(KU_THREADS) void keyed_uniform_kernel(const KeyedUniformParams p) {
    const long idx = (long)blockIdx.x * KU_THREADS + threadIdx.x;
    if (idx >= p.items) return;
    const long nblk = ((long)p.numel + 7) >> 3;
    const long s = idx / p.blocks_per_step;
    const long rem = idx - s * p.blocks_per_step;
    const long row = rem / nblk;
    const long q = rem - row * nblk;
    const uint64_t draw = p.first_draw + (uint64_t)(row / p.B);
    const uint64_t seq = p.first_seq + (uint64_t)(row % p.B);
    const uint64_t step = (uint64_t)p.first_step + (uint64_t)s;
    const Philox4x64 w = philox4x64_10((uint64_t)q, 0, seq, draw, p.seed, (step << 32) | (uint64_t)p.slot);
    float v[8];
    v[0] = ku_value((uint32_t)(w.w0 >> 32), p.scale);
    v[1] = ku_value((uint32_t)w.w0, p.scale);
    v[2] = ku_value((uint32_t)(w.w1 >> 32), p.scale);
    v[3] = ku_value((uint32_t)w.w1, p.scale);
    v[4] = ku_value((uint32_t)(w.w2 >> 32), p.scale);
    v[5] = ku_value((uint32_t)w.w2, p.scale);
    v[6] = ku_value((uint32_t)(w.w3 >> 32), p.scale);
    v[7] = ku_value((uint32_t)w.w3, p.scale);
    float* dst = p.out + (s * p.rows + row) * (long)p.numel + 8 * q;
    if (p.vec) {   // numel % 8 == 0: no tail block
        reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        const int left = p.numel - (int)(8 * q);   // >= 1
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < left) dst[e] = v[e];
    }
}

}  // namespace

extern "C" int rfn_latent_iw_f32(const float* enc, const float* pri, const float* eps_q, float* zxt, float* logr,
                                 int rows, int ZHW, int res_q, rfn_stream_t stream) {
    RFN_CHECK_ARG(rows >= 1 && ZHW >= 1, -1);
    RFN_CHECK_ARG(enc && pri && eps_q && zxt && logr, -1);
    hipLaunchKernelGGL(latent_iw_kernel, dim3((unsigned)ceil_div(rows, RFN_IW_ROWS)), dim3(64 * RFN_IW_ROWS), 0,
                       (hipStream_t)stream, enc, pri, eps_q, zxt, logr, rows, ZHW, res_q);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_keyed_uniform_f32(float* out, int n_steps, int rows, int B, int numel, float scale, long seed,
                                     int first_step, int slot, long first_seq, long first_draw, rfn_stream_t stream) {
    RFN_CHECK_ARG(n_steps >= 0 && numel >= 0, -1);
    RFN_CHECK_ARG(rows >= 0 && B >= 1 && rows % B == 0, -3);
    RFN_CHECK_ARG(seed >= 0 && first_seq >= 0 && first_draw >= 0 && first_step >= 0, -4);
    RFN_CHECK_ARG((long)first_step + n_steps <= 0x80000000L, -4);   // every step is a 32-bit word of the key
    RFN_CHECK_ARG(slot >= 8, -5);                                   // 0..7 are keyed_normal's
    RFN_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, -9);             // finite (NaN fails the first comparison)
    const long blocks_per_step = (((long)numel + 7) >> 3) * rows;
    if (blocks_per_step == 0 || n_steps == 0) return 0;
    RFN_CHECK_ARG(out && ((uintptr_t)out & 3) == 0, -6);
    RFN_CHECK_ARG(blocks_per_step <= 0x7fffffffL * KU_THREADS / n_steps, -7);
    KeyedUniformParams p;
    memset(&p, 0, sizeof(p));
    p.out = out;
    p.numel = numel;
    p.rows = rows;
    p.B = B;
    p.vec = (numel % 8 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    p.blocks_per_step = blocks_per_step;
    p.items = blocks_per_step * n_steps;
    p.scale = scale;
    p.seed = (uint64_t)seed;
    p.first_seq = (uint64_t)first_seq;
    p.first_draw = (uint64_t)first_draw;
    p.first_step = (uint32_t)first_step;
    p.slot = (uint32_t)slot;
    const long blocks = (p.items + KU_THREADS - 1) / KU_THREADS;   // <= 0x7fffffff by the check above
    hipLaunchKernelGGL(keyed_uniform_kernel, dim3((unsigned)blocks), dim3(KU_THREADS), 0, (hipStream_t)stream, p);
    RFN_LAUNCH_CHECK();
    return 0;
}
