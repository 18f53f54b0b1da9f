// Addressed normal noise for generation (RFN.predict_draws, the Evaluator's best-of-N): every N(0,1) value has an
// address and depends on nothing else -- not on the grid, the batch composition or how the draws are split into launches.
//
// One launch fills up to 8 tensors ("slots") [rows, numel_j], fp32 contiguous.  Row i of a launch stands for
// (draw, sequence): draw = first_draw + i / B, seq = first_seq + i % B (draw-major: i = r_local * B + b).
//   block q of slot j at step t = Philox4x64-10(key = (seed, (t << 32) | j), counter = (q, 0, seq, draw)), words w0..w3
//   (csrc/philox.h);
//   word w_i gives elements 8q + 2i and 8q + 2i + 1 of the row (flattened C*H*W):
//     a = w >> 32, b = w & 0xffffffff
//     u1 = ((a >> 8) + 1) * 2^-24   in (0, 1]
//     u2 = (b >> 8) * 2^-24         in [0, 1)
//     rad = sqrtf(-2 * logf(u1))
//     values rad * cospif(2 * u2), rad * sinpif(2 * u2)
//   with the accurate fp32 functions; 2 * u2 is exact, so no rounded 2 pi enters; |value| <= sqrt(48 ln 2) ~ 5.77.
//
// One lane per Philox block, eight results per lane: two 16-byte stores where numel_j % 8 == 0 and the slot's base is
// 16-byte aligned (then every row base is), single stores for a tail block and for unaligned slots.  The slot is
// blockIdx.z; its pointer and length are selected from the by-value tables with compile-time indices (a run-time index
// would put the whole struct in scratch memory).  A pure store stream: no atomics, no LDS.
//
// Tiled launches (rfn_keyed_normal_tiled_f32, a temperature sweep's common random numbers): the tensors hold `tiles`
// copies of the rows*numel_j block one after the other.  A lane computes its eight values once and stores them `tiles`
// times, numel_j * rows floats apart: the grid, the Philox blocks and the transcendental work are those of the untiled
// launch, only the stores multiply.  (A step's launch takes ~17 us from 0.55 MB to 4.4 MB -- it is bound by launch
// latency, not by ALU work or stores -- so recomputing would buy nothing and cost tiles x the arithmetic.)
#include "common.h"
#include "philox.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int KN_THREADS = 256;
constexpr int KN_MAX_SLOTS = 8;

struct KeyedNormalParams {
    float* out[KN_MAX_SLOTS];
    int numel[KN_MAX_SLOTS];
    unsigned vec_mask;   // bit j: slot j takes the 16-byte stores
    int rows, B;
    int tiles;           // copies of the [rows, numel] block per tensor, >= 1
    uint64_t seed, first_seq, first_draw;
    uint32_t step;
};

__device__ __forceinline__ void kn_pair(uint64_t w, float& x, float& y) {
    const uint32_t a = (uint32_t)(w >> 32), b = (uint32_t)w;
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;   // (0, 1]; the integer is at most 2^24: exact
    const float v2 = (float)(b >> 8) * 0x1p-23f;          // 2 * u2 in [0, 2): exact
    const float rad = sqrtf(-2.0f * logf(u1));
    x = rad * cospif(v2);
    y = rad * sinpif(v2);
}

__global__ __launch_bounds__(KN_THREADS) void keyed_normal_kernel(const KeyedNormalParams p) {
    const int j = (int)blockIdx.z;
    float* base = nullptr;
    int numel = 0;
#pragma unroll
    for (int i = 0; i < KN_MAX_SLOTS; ++i)
        if (i == j) {
            base = p.out[i];
            numel = p.numel[i];
        }
    if (numel <= 0) return;   // a slot this step does not use
    const long nblk = ((long)numel + 7) >> 3;
    const long idx = (long)blockIdx.x * KN_THREADS + threadIdx.x;
    if (idx >= nblk * p.rows) return;
    const long row = idx / nblk;
    const long q = idx - row * nblk;
    const uint64_t draw = p.first_draw + (uint64_t)(row / p.B);
    const uint64_t seq = p.first_seq + (uint64_t)(row % p.B);
    const Philox4x64 w = philox4x64_10((uint64_t)q, 0, seq, draw, p.seed, ((uint64_t)p.step << 32) | (uint64_t)j);
    float v[8];
    kn_pair(w.w0, v[0], v[1]);
    kn_pair(w.w1, v[2], v[3]);
    kn_pair(w.w2, v[4], v[5]);
    kn_pair(w.w3, v[6], v[7]);
    float* dst = base + row * (long)numel + 8 * q;
    const long tile_step = (long)p.rows * numel;   // a multiple of 8 floats where the slot takes 16-byte stores
    if ((p.vec_mask >> j) & 1u) {   // numel % 8 == 0: no tail block
        for (int k = 0; k < p.tiles; ++k, dst += tile_step) {
            reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
            reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
    } else {
        const int left = numel - (int)(8 * q);   // >= 1
        for (int k = 0; k < p.tiles; ++k, dst += tile_step) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < left) dst[e] = v[e];
        }
    }
}

}  // namespace

static int keyed_normal_launch(float* const* outs, const int* numels, int n_slots, int rows, int B, int tiles,
                               long seed, int step, long first_seq, long first_draw, rfn_stream_t stream) {
    RFN_CHECK_ARG(n_slots >= 1 && n_slots <= KN_MAX_SLOTS, -1);
    RFN_CHECK_ARG(outs && numels, -2);
    RFN_CHECK_ARG(rows >= 0 && B >= 1 && rows % B == 0, -3);
    RFN_CHECK_ARG(seed >= 0 && first_seq >= 0 && first_draw >= 0 && step >= 0, -4);
    RFN_CHECK_ARG(tiles >= 1 && (long)tiles * rows <= 0x7fffffffL, -8);
    KeyedNormalParams p;
    memset(&p, 0, sizeof(p));
    long most = 0;
    for (int j = 0; j < n_slots; ++j) {
        RFN_CHECK_ARG(numels[j] >= 0, -5);
        if (numels[j] == 0) continue;
        RFN_CHECK_ARG(outs[j] && ((uintptr_t)outs[j] & 3) == 0, -6);
        p.out[j] = outs[j];
        p.numel[j] = numels[j];
        if (numels[j] % 8 == 0 && ((uintptr_t)outs[j] & 15) == 0) p.vec_mask |= 1u << j;
        const long items = (((long)numels[j] + 7) >> 3) * rows;
        if (items > most) most = items;
    }
    if (most == 0) return 0;
    const long blocks = (most + KN_THREADS - 1) / KN_THREADS;
    RFN_CHECK_ARG(blocks <= 0x7fffffffL, -7);
    p.rows = rows;
    p.B = B;
    p.tiles = tiles;
    p.seed = (uint64_t)seed;
    p.first_seq = (uint64_t)first_seq;
    p.first_draw = (uint64_t)first_draw;
    p.step = (uint32_t)step;
    hipLaunchKernelGGL(keyed_normal_kernel, dim3((unsigned)blocks, 1, (unsigned)n_slots), dim3(KN_THREADS), 0,
                       (hipStream_t)stream, p);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_keyed_normal_f32(float* const* outs, const int* numels, int n_slots, int rows, int B, long seed,
                                    int step, long first_seq, long first_draw, rfn_stream_t stream) {
    return keyed_normal_launch(outs, numels, n_slots, rows, B, 1, seed, step, first_seq, first_draw, stream);
}

extern "C" int rfn_keyed_normal_tiled_f32(float* const* outs, const int* numels, int n_slots, int rows, int B,
                                          int tiles, long seed, int step, long first_seq, long first_draw,
                                          rfn_stream_t stream) {
    return keyed_normal_launch(outs, numels, n_slots, rows, B, tiles, seed, step, first_seq, first_draw, stream);
}
