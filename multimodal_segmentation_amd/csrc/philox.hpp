// Counter-based randomness and the blur boundary rule shared by the augmentation units (augment.hip: the elastic field; intensity.hip:
// the blur and the noise).  The host restates both in utils/augment.py.
#pragma once
#include "common.hpp"

// Philox4x32-10: 4 counter words, 2 key words -> the first two of the 4 output words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& o0, uint32_t& o1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0;
    o1 = c1;
}

// half-sample symmetric reflection, period 2n
__device__ __forceinline__ int el_reflect(int i, int n) {
    const int p = 2 * n;
    int t = i % p;
    if (t < 0) t += p;
    return t >= n ? p - 1 - t : t;
}
