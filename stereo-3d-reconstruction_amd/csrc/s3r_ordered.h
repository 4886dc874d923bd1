// The ordered-sum scheme of the backward kernels (s3r_head_bwd.hip, s3r_batchnorm.hip, s3r_conv_bwd.hip, s3r_stem_bwd.hip,
// s3r_linear_bwd.hip, s3r_voxel_loss.hip): the building blocks that make "fixed summation order, no atomics, the same bits on every run and
// at every 4-byte-aligned address" ONE rule instead of one per file.  tests/_linear64.g32 restates the activation rule and
// tests/_head64.chunk_sums32 / reduce32 the order of the sums; what changes here changes every layer's bits together.
//
// The contract.  Everything is fp32 and every operation is rounded on its own (#pragma clang fp contract(off): a product is rounded, then
// added — NOT fused).
//   - A row's S positions are cut into chunks of CHUNK = 512 consecutive positions (the last may be short; missing positions count as +0.0).
//   - A WAVE owns one chunk: lane L (0..63) owns the eight positions 256 j + 4 L + i (j = 0 .. Q - 1; i = 0..3) — Q = 2 16-byte accesses
//     per lane and tensor through a dword-aligned vector type (v4f_u), 1 KiB contiguous per wave instruction — and adds its terms in
//     ascending position to a partial that starts as +0.0.
//   - The 64 partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1 (wave_tree); v[0] is the
//     chunk's sum, stored to a row [B][nch] of chunk sums, nch = chunks(S).
//   - row_total, one wave per row: lane L adds the chunk sums of sample b0 + L in ascending chunk order into a partial that starts as chunk
//     0's sum (a function of S only); the per-sample partials are added into ONE accumulator in ascending b, starting from sample 0's.
// A pointer (or a row, when S is no multiple of 4) that is only 4-byte aligned runs the same instructions.  A chunk that crosses its row's
// end is read and written element by element in every lane (`full`, a wave-uniform choice — no per-lane branch in the streaming path):
// the same arithmetic, the same bits.  Terms of positions past the row's end are replaced by +0.0 AFTER they are computed (0 * NaN and
// 0 * inf would be NaN), which changes no bit: a partial that starts as +0.0 never holds -0.0, so partial + (+0.0) == partial.  Waves are
// independent: no LDS, no barrier.
#pragma once
#include "s3r_kernels.h"

namespace s3r {

constexpr int CHUNK = 512;           // positions per wave: 2 x (64 lanes x 16 bytes)
constexpr int Q = CHUNK / 256;       // 16-byte quads per lane

inline long long chunks(long long S) { return (S + CHUNK - 1) / CHUNK; }

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));       // dword-aligned 16-byte access

// positions i .. i + 3 of a row of n; `full` (wave-uniform: the wave's whole chunk lies inside the row) takes the 16-byte access
__device__ __forceinline__ v4f load4(const float* __restrict__ p, long long i, long long n, bool full) {
    if (full) return *reinterpret_cast<const v4f_u*>(p + i);
    v4f v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : 0.f;
    return v;
}

__device__ __forceinline__ void store4(float* __restrict__ p, long long i, long long n, v4f v, bool full) {
    if (full) { *reinterpret_cast<v4f_u*>(p + i) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) p[i + k] = v[k];
}

// the pre-activation gradient g of y = act(u) from (y, grad_y), nothing fused:
//   none: g = grad_y        ReLU: g = (y > 0.f) ? grad_y : 0.f  (a NaN y gives 0)        sigmoid: t = 1 - y; u = y * t; g = grad_y * u
__device__ __forceinline__ float act_grad(float y, float gy, int act) {
#pragma clang fp contract(off)
    if (act == 1) return (y > 0.f) ? gy : 0.f;
    if (act == 2) {
        const float t = 1.f - y;
        const float u = y * t;
        return gy * u;
    }
    return gy;
}

__device__ __forceinline__ float wave_tree(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
    return v;                                                            // (lane 0 holds the tree's root)
}

// the total of one row [B][nch] of chunk sums, in every lane of the one wave that calls it
__device__ __forceinline__ float row_total(const float* __restrict__ part, int B, long long nch, int lane) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        float p = 0.f;
        if (b < B) {
            const float* __restrict__ src = part + (size_t)b * nch;
            p = src[0];
            long long z = 1;
            for (; z + 16 <= nch; z += 16) {                             // sixteen loads in flight, then the adds in order
                float t[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = src[z + u];
#pragma unroll
                for (int u = 0; u < 16; ++u) p = p + t[u];
            }
            for (; z < nch; ++z) p = p + src[z];
        }
        const int n = B - b0 < 64 ? B - b0 : 64;
        for (int l = 0; l < n; ++l) {
            const float v = __shfl(p, l, 64);
            acc = (b0 + l == 0) ? v : acc + v;
        }
    }
    return acc;
}

}  // namespace s3r
