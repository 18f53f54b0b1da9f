// Philox4x64-10 (Salmon et al. 2011; the generator of numpy's np.random.Philox): one block of four 64-bit words from a
// 4-word counter under a 2-word key.  Round function and constants are those of csrc/moving_mnist.hip, which keeps its
// own word-0 copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct Philox4x64 { uint64_t w0, w1, w2, w3; };

__device__ __forceinline__ Philox4x64 philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0,
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
    return Philox4x64{c0, c1, c2, c3};
}
