// The counter-based random numbers of the training-time kernels (s3r_augment.hip, s3r_surface_points.hip): Philox4x32-10 and the map of
// a word to [0, 1).  include/s3r.h states both (s3r_augment_pair, "Random numbers"); tests/_augment64.py restates them.
#pragma once
#include <hip/hip_runtime.h>

namespace s3r {

struct Words { unsigned w[4]; };

__device__ __forceinline__ Words philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1;
        c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float aug_unit(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }      // 2^-24: exact

}  // namespace s3r
