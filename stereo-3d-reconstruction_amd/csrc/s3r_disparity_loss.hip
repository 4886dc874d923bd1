// Masked smooth-L1 loss on disparity maps (s3r_disparity_loss_forward / s3r_disparity_loss_backward): pred, gt (B, P) fp32, a pixel
// valid exactly as s3r_disparity_metrics defines it (ground truth finite and >= 0), a per-sample fp32 sum in s3r_voxel_bce_forward's
// FIXED order — a function of P only —, the per-sample count of valid pixels, and the elementwise gradient.  Built like
// s3r_voxel_loss.hip: 16-byte accesses per lane through a dword-aligned vector type, so a pointer (or a sample row, when P is no
// multiple of 4) that is only 4-byte aligned runs the same instructions and gives the same bits; a quad that crosses the end of its
// tensor is read and written element by element.  No atomics, no scratch.
//
// Per valid element (contraction off, every operation rounded once), e = pred - gt, a = |e|:
//   a < beta:  h = 0.5f * e;  s = h * e;  l = s / beta          (IEEE division)
//   otherwise: l = a - 0.5f * beta                               (beta == 0: a - 0 = |e|, plain L1; a NaN e compares false: l is NaN)
// An invalid element is +0.0 by a SELECT: its pred and gt never enter arithmetic (0 * NaN would be NaN).
//
// loss_sum[b] (disparity_loss_kernel, one workgroup of 16 waves per sample): the order of voxel_bce_kernel —
//   - the sample's P losses are cut into chunks of 1024 consecutive elements (the last may be short: missing elements count as +0.0);
//   - one wave sums a chunk: lane L (0..63) owns the 16 elements 256 j + 4 L + i (j = 0..3, i = 0..3) and adds them in ascending
//     element order to a partial that starts as +0.0; the 64 partials are combined by the halving tree (wave_tree, s3r_ordered.h);
//   - the chunk sums are added in ascending chunk order into ONE accumulator that starts as chunk 0's sum.
// count[b]: the valid pixels, an exact integer (the order of an integer sum does not matter).
//
// grad_pred (disparity_loss_bwd_kernel, elementwise over the flat (B P) tensor), valid elements:
//   beta > 0:  v = e / beta;  c = (v < -1.f) ? -1.f : ((v > 1.f) ? 1.f : v);  grad_pred = grad_scale[b] * c     (a NaN passes the selects)
//   beta == 0: c = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : ((e == 0.f) ? 0.f : e));  grad_pred = grad_scale[b] * c
// invalid elements: exactly +0.0.
#include "s3r_ordered.h"

namespace s3r {

constexpr int DL_CHUNK = 1024;       // elements per chunk: 4 x (64 lanes x 16 bytes) — voxel_bce_kernel's
constexpr int DL_WAVES = 16;         // waves per workgroup = chunks per round

// elements i .. i + 3 of a tensor of n elements; `fill` where i + k >= n (never read)
__device__ __forceinline__ v4f dl_load4(const float* __restrict__ p, long long i, long long n, float fill) {
    if (i + 4 <= n) return *reinterpret_cast<const v4f_u*>(p + i);
    v4f v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : fill;
    return v;
}

__device__ __forceinline__ void dl_store4(float* __restrict__ p, long long i, long long n, v4f v) {
    if (i + 4 <= n) { *reinterpret_cast<v4f_u*>(p + i) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) p[i + k] = v[k];
}

__device__ __forceinline__ bool dl_valid(float t) { return (t >= 0.f) && (t < __builtin_inff()); }      // false for NaN as well

__device__ __forceinline__ float dl_elem(float p, float t, float beta) {
#pragma clang fp contract(off)
    if (!dl_valid(t)) return 0.f;
    const float e = p - t;
    const float a = fabsf(e);
    if (a < beta) {
        const float h = 0.5f * e;
        const float s = h * e;
        return s / beta;
    }
    return a - 0.5f * beta;
}

__device__ __forceinline__ float dl_grad(float p, float t, float gs, float beta) {
#pragma clang fp contract(off)
    if (!dl_valid(t)) return 0.f;
    const float e = p - t;
    float c;
    if (beta > 0.f) {
        const float v = e / beta;
        c = (v < -1.f) ? -1.f : ((v > 1.f) ? 1.f : v);
    } else {
        c = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : ((e == 0.f) ? 0.f : e));
    }
    return gs * c;
}

__global__ __launch_bounds__(64 * DL_WAVES) void disparity_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                      float beta, float* __restrict__ loss_sum,
                                                                      int* __restrict__ count, float* __restrict__ loss_elem,
                                                                      long long P) {
#pragma clang fp contract(off)
    __shared__ float csum[DL_WAVES];
    __shared__ unsigned ccnt[DL_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t row = (size_t)blockIdx.x * P;
    const float* __restrict__ p = pred + row;
    const float* __restrict__ t = gt + row;
    float* __restrict__ le = loss_elem ? loss_elem + row : nullptr;
    const long long nch = (P + DL_CHUNK - 1) / DL_CHUNK;
    float total = 0.f;
    unsigned valid = 0u;                                                 // this lane's valid pixels over all its chunks
    for (long long c0 = 0; c0 < nch; c0 += DL_WAVES) {
        const long long ch = c0 + wave;
        float s = 0.f;
        if (ch < nch) {                                                  // (wave-uniform)
            v4f pv[4], tv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                // all eight loads in flight before the first division
                const long long e = ch * DL_CHUNK + 256 * j + 4 * lane;
                pv[j] = dl_load4(p, e, P, 0.f);
                tv[j] = dl_load4(t, e, P, -1.f);                         // (past the end: invalid)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = ch * DL_CHUNK + 256 * j + 4 * lane;
                v4f l;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    l[i] = dl_elem(pv[j][i], tv[j][i], beta);
                    s = s + (e + i < P ? l[i] : 0.f);
                    valid += (e + i < P && dl_valid(tv[j][i])) ? 1u : 0u;
                }
                if (le) dl_store4(le, e, P, l);
            }
            s = wave_tree(s);
        }
        if (lane == 0) csum[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = nch - c0 < DL_WAVES ? (int)(nch - c0) : DL_WAVES;
            for (int i = 0; i < n; ++i) total = (c0 + i == 0) ? csum[i] : total + csum[i];
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_xor(valid, o, 64);
    if (lane == 0) ccnt[wave] = valid;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned n = 0u;
        for (int i = 0; i < DL_WAVES; ++i) n += ccnt[i];
        loss_sum[blockIdx.x] = total;
        count[blockIdx.x] = (int)n;
    }
}

// one thread per four consecutive elements of the flat (B P) tensor; the sample of each element picks its grad_scale
__global__ __launch_bounds__(256) void disparity_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const float* __restrict__ gscale, float beta,
                                                                 float* __restrict__ gpred, long long P, long long total) {
#pragma clang fp contract(off)
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    long long b = i0 / P, r = i0 - b * P;
    const v4f p = dl_load4(pred, i0, total, 0.f), t = dl_load4(gt, i0, total, -1.f);
    v4f g;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = 0.f;
        if (i0 + k < total) {
            g[k] = dl_grad(p[k], t[k], gscale[b], beta);
            if (++r == P) { r = 0; ++b; }
        }
    }
    dl_store4(gpred, i0, total, g);
}

hipError_t launch_disparity_loss(const float* pred, const float* gt, float beta, float* loss_sum, int* count, float* loss_elem, int B,
                                 int64_t P, hipStream_t s) {
    hipLaunchKernelGGL(disparity_loss_kernel, dim3((unsigned)B), dim3(64 * DL_WAVES), 0, s, pred, gt, beta, loss_sum, count, loss_elem,
                       (long long)P);
    return hipGetLastError();
}

hipError_t launch_disparity_loss_backward(const float* pred, const float* gt, const float* gscale, float beta, float* gpred, int B,
                                          int64_t P, hipStream_t s) {
    const long long total = (long long)B * P;
    hipLaunchKernelGGL(disparity_loss_bwd_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, pred, gt, gscale, beta, gpred,
                       (long long)P, total);
    return hipGetLastError();
}

}  // namespace s3r
