// Binary cross-entropy on occupancy grids (s3r_voxel_bce_forward / s3r_voxel_bce_backward): torch.nn.BCELoss's per-element rule
// on pred, target (B, V), a per-sample fp32 sum in a FIXED order that is a function of V only, and the elementwise gradient.  Both
// stream memory with 16-byte accesses per lane through a dword-aligned vector type, so a pointer (or a sample row, when V is no
// multiple of 4) that is only 4-byte aligned runs the same instructions and gives the same bits; a quad that crosses the end of its
// tensor is read and written element by element.  No atomics, no scratch.
//
// Per element (contraction off, every operation rounded once):
//   a = clamp(logf(p));  c = clamp(logf(1.f - p));  l = -(t * a + (1.f - t) * c);  clamp(v) = (v < -100.f) ? -100.f : v
// The clamp comes BEFORE the multiplication (p = 0, t = 0 is 0 * -100, not 0 * -inf) and is a compare-and-select, so a NaN passes
// through it (fmaxf would swallow it): a NaN or out-of-range p gives a NaN l.
//
// loss_sum[b] (voxel_bce_kernel, one workgroup of 16 waves per sample):
//   - the sample's V losses are cut into chunks of 1024 consecutive elements (the last one may be short: the missing elements count
//     as +0.0);
//   - one wave sums a chunk: lane L (0..63) owns the 16 elements 256 j + 4 L + i (j = 0..3, i = 0..3: four 16-byte loads per tensor)
//     and adds them in ascending element order to a partial that starts as +0.0; the 64 partials are combined by the halving tree
//     v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1;
//   - the chunk sums are added in ascending chunk order into ONE accumulator that starts as chunk 0's sum (waves 0..15 take chunks
//     c0 .. c0 + 15 of a round; thread 0 adds the round's sums in order).
// Nothing of this depends on B, on the device or on an address: sample b has the same bits in every batch split.
//
// grad_pred (voxel_bce_bwd_kernel, elementwise over the flat (B V) tensor):
//   n = grad_scale[b] * (p - t);  d = max((1.f - p) * p, 1e-12f);  grad_pred = n / d    (IEEE division)
#include "s3r_ordered.h"

namespace s3r {

constexpr int BCE_CHUNK = 1024;      // elements per chunk: 4 x (64 lanes x 16 bytes)
constexpr int BCE_WAVES = 16;        // waves per workgroup = chunks per round

// not s3r_ordered.h's load4 / store4: the choice is per quad, with a fill value, in chunks of 1024
// elements i .. i + 3 of a tensor of n elements; `fill` where i + k >= n (never read)
__device__ __forceinline__ v4f bce_load4(const float* __restrict__ p, long long i, long long n, float fill) {
    if (i + 4 <= n) return *reinterpret_cast<const v4f_u*>(p + i);
    v4f v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : fill;
    return v;
}

__device__ __forceinline__ void bce_store4(float* __restrict__ p, long long i, long long n, v4f v) {
    if (i + 4 <= n) { *reinterpret_cast<v4f_u*>(p + i) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) p[i + k] = v[k];
}

__device__ __forceinline__ float bce_clamp(float v) { return (v < -100.f) ? -100.f : v; }      // (a NaN compares false: it passes)

__device__ __forceinline__ float bce_elem(float p, float t) {
#pragma clang fp contract(off)
    const float a = bce_clamp(logf(p));
    const float c = bce_clamp(logf(1.f - p));
    return -(t * a + (1.f - t) * c);
}

__global__ __launch_bounds__(64 * BCE_WAVES) void voxel_bce_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  float* __restrict__ loss_sum, float* __restrict__ loss_elem,
                                                                  long long V) {
#pragma clang fp contract(off)
    __shared__ float csum[BCE_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t row = (size_t)blockIdx.x * V;
    const float* __restrict__ p = pred + row;
    const float* __restrict__ t = target + row;
    float* __restrict__ le = loss_elem ? loss_elem + row : nullptr;
    const long long nch = (V + BCE_CHUNK - 1) / BCE_CHUNK;
    float total = 0.f;
    for (long long c0 = 0; c0 < nch; c0 += BCE_WAVES) {
        const long long ch = c0 + wave;
        float s = 0.f;
        if (ch < nch) {                                                  // (wave-uniform)
            v4f pv[4], tv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                // all eight loads in flight before the first logf
                const long long e = ch * BCE_CHUNK + 256 * j + 4 * lane;
                pv[j] = bce_load4(p, e, V, 0.5f);
                tv[j] = bce_load4(t, e, V, 0.5f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = ch * BCE_CHUNK + 256 * j + 4 * lane;
                v4f l;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    l[i] = bce_elem(pv[j][i], tv[j][i]);
                    s = s + (e + i < V ? l[i] : 0.f);
                }
                if (le) bce_store4(le, e, V, l);
            }
            s = wave_tree(s);
        }
        if (lane == 0) csum[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = nch - c0 < BCE_WAVES ? (int)(nch - c0) : BCE_WAVES;
            for (int i = 0; i < n; ++i) total = (c0 + i == 0) ? csum[i] : total + csum[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss_sum) loss_sum[blockIdx.x] = total;
}

// one thread per four consecutive elements of the flat (B V) tensor; the sample of each element picks its grad_scale
__global__ __launch_bounds__(256) void voxel_bce_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            const float* __restrict__ gscale, float* __restrict__ gpred, long long V,
                                                            long long total) {
#pragma clang fp contract(off)
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    long long b = i0 / V, r = i0 - b * V;
    const v4f p = bce_load4(pred, i0, total, 0.5f), t = bce_load4(target, i0, total, 0.5f);
    v4f g;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = 0.f;
        if (i0 + k < total) {
            const float n = gscale[b] * (p[k] - t[k]);
            const float d = fmaxf((1.f - p[k]) * p[k], 1e-12f);
            g[k] = n / d;
            if (++r == V) { r = 0; ++b; }
        }
    }
    bce_store4(gpred, i0, total, g);
}

hipError_t launch_voxel_bce(const float* pred, const float* target, float* loss_sum, float* loss_elem, int B, int64_t V,
                            hipStream_t s) {
    hipLaunchKernelGGL(voxel_bce_kernel, dim3((unsigned)B), dim3(64 * BCE_WAVES), 0, s, pred, target, loss_sum, loss_elem, (long long)V);
    return hipGetLastError();
}

hipError_t launch_voxel_bce_backward(const float* pred, const float* target, const float* gscale, float* gpred, int B, int64_t V,
                                     hipStream_t s) {
    const long long total = (long long)B * V;
    hipLaunchKernelGGL(voxel_bce_bwd_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, pred, target, gscale, gpred,
                       (long long)V, total);
    return hipGetLastError();
}

}  // namespace s3r
