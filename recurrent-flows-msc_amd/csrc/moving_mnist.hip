// Stochastic Moving MNIST rendered on the GPU (data_generators/stochasticMovingMnist.py:48-127 of the reference,
// MovingMNIST.__getitem__ with normalize=False, make_target=False, set_starting_position=False, digit_size 28).
//
// Walk of digit n of one sequence (the reference's, draw for draw):
//   idx = randint(N); sx = randint(S-D); sy = randint(S-D); dx = randint(-L, L+1); dy = randint(-L, L+1)
//   for t in 0..T-1:
//     y-bounce (sy < 0 -> sy = 0, sy >= S-D -> sy = S-D-1), then x-bounce (same for sx).  Deterministic variant: the
//       velocity component is negated.  Stochastic variant: a y-bounce redraws dy (randint(1, L+1) at the top wall,
//       randint(-L, 0) at the bottom), then dx = randint(-L, L+1); an x-bounce redraws dx the same way, then dy.
//     frame t gets the digit at (sy, sx); then sy += dy, sx += dx.
// Pixels: a digit byte k is float32(k) / float32(255) correctly rounded (torchvision ToTensor); the digits are summed in
// float32 in digit order, then x[x > 1] = 1; the C output channels are copies.
//
// Random draws (replacing numpy's global RNG): every draw has an address.
//   block     = Philox4x64-10(key = (seed, split), counter = (draw number, retry, sequence id, digit n)), word 0 used;
//   draw j of digit n is the j-th randint call of the walk above (0 = idx, 1 = sx, 2 = sy, 3 = dx, 4 = dy, then the
//   bounce redraws in order); retry starts at 0.
//   randint(lo, hi) = lo + Lemire(x, r = hi - lo): m = x * r (128 bit); if low64(m) < (2^64 - r) mod r the draw is
//   rejected and repeated with retry + 1 (exactly uniform; a rejection has probability below r / 2^64, i.e. < 2^-48
//   for r <= 70000), else the result is high64(m).
// Same (seed, split, sequence id) -> same bytes, on any grid, any batch composition and any number of ranks.
//
// Synchronized variant (MovingMNIST_synchronized, stochasticMovingMnist.py:131-248; rfn_moving_mnist_sync_render_f32):
// all sequences share one trajectory per digit, only the digit identities differ.
//   idx = randint(N); sx = randint(S-D); sy = randint(S-D); dx = dy = 3 (a constant whatever L is, as the reference has
//   it); then the frame loop above with L and the deterministic flag.
//   idx is draw 0 at the plain counter (0, retry, sequence id, n); every other draw uses the shared counter
//   (j, retry, 2^64-1, n): j = 1 for sx, 2 for sy, 3, 4, ... for the bounce redraws in walk order.  Sequence ids are
//   non-negative (< 2^63), so the shared address collides with none of them.  Same key, same bounded draw.
//   hit[b, t] = the largest n + 1 over the digits that either bounce branch clamped on frame t, 0 if none (the
//   reference's hit_boundary, which it overwrites in digit order); every row b holds the same values.
//
// One workgroup per (sequence, frame): lanes 0..num_digits-1 replay their digit's walk up to the frame (at most
// 4 draws per step; T is tens of steps) and publish (idx, y, x) in LDS; the workgroup stages the digits as float32 in
// LDS and writes the frame with 16-byte stores (scalar stores when S*S is not a multiple of 4), every output pixel
// summing only the digits whose 28x28 window covers it.
#include "common.h"
#include "../../include/rfn_hip.h"

namespace {

constexpr int MM_THREADS = 256;
constexpr int MM_D = 28;
constexpr int MM_DD = MM_D * MM_D;
constexpr int MM_MAX_DIGITS = 8;

struct Draws {
    uint64_t k0, k1;   // key = (seed, split)
    uint64_t seq;      // counter word 2
    uint64_t n;        // counter word 3
    uint64_t j;        // counter word 0: draws made so far
};

__device__ __forceinline__ uint64_t philox4x64_10_w0(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0,
                                                     uint64_t k1) {
    const uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    const uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t lo0 = M0 * c0, hi0 = __umul64hi(M0, c0);
        const uint64_t lo1 = M1 * c2, hi1 = __umul64hi(M1, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return c0;
}

// uniform integer in [0, r), r >= 1
__device__ __forceinline__ int draw_below(Draws& d, uint64_t r) {
    for (uint64_t retry = 0;; ++retry) {
        const uint64_t x = philox4x64_10_w0(d.j, retry, d.seq, d.n, d.k0, d.k1);
        const uint64_t lo = x * r;
        if (lo < r && lo < (0ull - r) % r) continue;   // rejected: same draw number, next retry
        d.j += 1;
        return (int)__umul64hi(x, r);
    }
}

// one frame's wall handling of the walk above: y-bounce, then x-bounce; true if either clamped the digit
__device__ __forceinline__ bool bounce(int& sy, int& sx, int& dy, int& dx, Draws& d, int R, int L, uint64_t span,
                                       int det) {
    bool clamped = false;
    if (sy < 0) {
        sy = 0;
        clamped = true;
        if (det) {
            dy = -dy;
        } else {
            dy = 1 + draw_below(d, (uint64_t)L);
            dx = draw_below(d, span) - L;
        }
    } else if (sy >= R) {
        sy = R - 1;
        clamped = true;
        if (det) {
            dy = -dy;
        } else {
            dy = draw_below(d, (uint64_t)L) - L;
            dx = draw_below(d, span) - L;
        }
    }
    if (sx < 0) {
        sx = 0;
        clamped = true;
        if (det) {
            dx = -dx;
        } else {
            dx = 1 + draw_below(d, (uint64_t)L);
            dy = draw_below(d, span) - L;
        }
    } else if (sx >= R) {
        sx = R - 1;
        clamped = true;
        if (det) {
            dx = -dx;
        } else {
            dx = draw_below(d, (uint64_t)L) - L;
            dy = draw_below(d, span) - L;
        }
    }
    return clamped;
}

// SYNC: the synchronized dataset (every sequence shares the trajectories; `hit` as the file header states)
template <bool SYNC>
__global__ __launch_bounds__(MM_THREADS) void moving_mnist_kernel(const uint8_t* __restrict__ digits, int N,
                                                                  float* __restrict__ out, long long* __restrict__ traj,
                                                                  int* __restrict__ hit, int T, int C, int S, int nd,
                                                                  int L, int det, uint64_t seed, uint64_t split,
                                                                  uint64_t first_id, int vec) {
    __shared__ float lut[256];
    __shared__ float glyph[MM_MAX_DIGITS][MM_DD];
    __shared__ int pos[MM_MAX_DIGITS][SYNC ? 4 : 3];

    const int t = (int)(blockIdx.x % (unsigned)T);
    const long b = (long)(blockIdx.x / (unsigned)T);
    const int tid = threadIdx.x;

    // ToTensor's k / 255 in float32, correctly rounded: the fp64 quotient is within 2^-53 (relative) of k / 255, which
    // is never that close to a float32 rounding boundary, so rounding it to float32 gives the correctly rounded value
    lut[tid] = (float)((double)tid / 255.0);

    if (tid < nd) {
        const int R = S - MM_D;   // start positions in [0, R), clamps to [0, R - 1]
        Draws d{seed, split, first_id + (uint64_t)b, (uint64_t)tid, 0};
        const int idx = draw_below(d, (uint64_t)N);
        if (SYNC) {   // every draw after idx comes from the address all sequences share, starting at draw 1
            d.seq = ~0ull;
            d.j = 1;
        }
        int sx = draw_below(d, (uint64_t)R);
        int sy = draw_below(d, (uint64_t)R);
        const uint64_t span = 2 * (uint64_t)L + 1;
        int dx = SYNC ? 3 : draw_below(d, span) - L;
        int dy = SYNC ? 3 : draw_below(d, span) - L;
        bool clamped = false;
        for (int s = 0;; ++s) {
            clamped = bounce(sy, sx, dy, dx, d, R, L, span, det);
            if (s == t) break;
            sy += dy;
            sx += dx;
        }
        pos[tid][0] = idx;
        pos[tid][1] = sy;
        pos[tid][2] = sx;
        if constexpr (SYNC) pos[tid][3] = clamped ? 1 : 0;
        if (traj) {
            long long* o = traj + (((long)b * nd + tid) * T + t) * 3;
            o[0] = idx;
            o[1] = sy;
            o[2] = sx;
        }
    }
    __syncthreads();

    if constexpr (SYNC) {
        if (hit && tid == 0) {   // the reference overwrites in digit order: the last clamped digit wins
            int h = 0;
            for (int n = 0; n < nd; ++n)
                if (pos[n][3]) h = n + 1;
            hit[(long)b * T + t] = h;
        }
    }

    for (int k = tid; k < nd * MM_DD; k += MM_THREADS) {
        const int n = k / MM_DD, e = k - n * MM_DD;
        glyph[n][e] = lut[digits[(long)pos[n][0] * MM_DD + e]];
    }
    __syncthreads();

    int py[MM_MAX_DIGITS], px[MM_MAX_DIGITS];
#pragma unroll
    for (int n = 0; n < MM_MAX_DIGITS; ++n) {
        py[n] = n < nd ? pos[n][1] : 0;
        px[n] = n < nd ? pos[n][2] : 0;
    }
    auto pixel = [&](int p) {
        const int y = p / S, x = p - y * S;
        float v = 0.0f;
#pragma unroll
        for (int n = 0; n < MM_MAX_DIGITS; ++n) {
            if (n >= nd) break;
            const int u = y - py[n], w = x - px[n];
            if ((unsigned)u < (unsigned)MM_D && (unsigned)w < (unsigned)MM_D) v += glyph[n][u * MM_D + w];
        }
        return v > 1.0f ? 1.0f : v;
    };

    const int SS = S * S;
    float* frame = out + ((long)b * T + t) * (long)C * SS;
    if (vec) {   // SS % 4 == 0 and a 16-byte aligned base: every channel plane starts 16-byte aligned
        for (int q = tid; q < SS / 4; q += MM_THREADS) {
            const float4 v = make_float4(pixel(4 * q), pixel(4 * q + 1), pixel(4 * q + 2), pixel(4 * q + 3));
            for (int c = 0; c < C; ++c) reinterpret_cast<float4*>(frame + (long)c * SS)[q] = v;
        }
    } else {
        for (int p = tid; p < SS; p += MM_THREADS) {
            const float v = pixel(p);
            for (int c = 0; c < C; ++c) frame[(long)c * SS + p] = v;
        }
    }
}

}  // namespace

static int mm_render(bool sync, const void* digits, int N, float* out, long long* traj, int* hit, int B, int T, int C,
                     int S, int num_digits, int step_length, int deterministic, long seed, long split, long first_id,
                     rfn_stream_t stream) {
    RFN_CHECK_ARG(B >= 0 && T >= 1 && C >= 1, -1);
    RFN_CHECK_ARG(S > MM_D && S <= 4096, -2);
    RFN_CHECK_ARG(num_digits >= 1 && num_digits <= MM_MAX_DIGITS, -3);
    RFN_CHECK_ARG(step_length >= 1 && step_length <= (1 << 20), -4);
    RFN_CHECK_ARG(N >= 1, -5);
    RFN_CHECK_ARG(seed >= 0 && split >= 0 && first_id >= 0, -6);
    RFN_CHECK_ARG((long)B * T <= 0x7fffffffL, -7);
    if (B == 0) return 0;
    RFN_CHECK_ARG(digits && out, -8);
    const int vec = (S * S) % 4 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(sync ? moving_mnist_kernel<true> : moving_mnist_kernel<false>, dim3((unsigned)(B * T)),
                       dim3(MM_THREADS), 0, (hipStream_t)stream, (const uint8_t*)digits, N, out, traj, hit, T, C, S,
                       num_digits, step_length, deterministic, (uint64_t)seed, (uint64_t)split, (uint64_t)first_id,
                       vec);
    RFN_LAUNCH_CHECK();
    return 0;
}

extern "C" int rfn_moving_mnist_render_f32(const void* digits, int N, float* out, long long* traj, int B, int T, int C,
                                           int S, int num_digits, int step_length, int deterministic, long seed,
                                           long split, long first_id, rfn_stream_t stream) {
    return mm_render(false, digits, N, out, traj, nullptr, B, T, C, S, num_digits, step_length, deterministic, seed,
                     split, first_id, stream);
}

extern "C" int rfn_moving_mnist_sync_render_f32(const void* digits, int N, float* out, long long* traj, long hit_addr,
                                                int B, int T, int C, int S, int num_digits, int step_length,
                                                int deterministic, long seed, long split, long first_id,
                                                rfn_stream_t stream) {
    RFN_CHECK_ARG((hit_addr & 3) == 0, -9);
    return mm_render(true, digits, N, out, traj, reinterpret_cast<int*>(hit_addr), B, T, C, S, num_digits, step_length,
                     deterministic, seed, split, first_id, stream);
}
