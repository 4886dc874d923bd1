// Train-mode BatchNorm with batch statistics (s3r_batchnorm_train_forward / s3r_batchnorm_train_backward): z (B,C,S) fp32 plain, S the
// product of the spatial extents (one entry serves 2D and 3D layers), gamma / beta (C), N = B S, nf = (float)N.  Everything is fp32, every
// operation is rounded on its own (#pragma clang fp contract(off): the product is rounded, then the add — NOT fused), and every sum has
// a FIXED order — no atomics, the same bits on every run, at every 4-byte-aligned address and with any scratch contents on entry.
//
// Forward, five launches:
//   1 bn_stat_kernel<false>   chunk sums of z                          -> scratch[c][b][chunk]
//   2 bn_finish_kernel        mean[c] = total / nf                     -> save_mean
//   3 bn_stat_kernel<true>    chunk sums of d * d, d = z - mean[c]     -> scratch[c][b][chunk]   (two-pass: no sum of z^2 anywhere)
//   4 bn_finish_kernel        var[c] = total / nf (biased); invstd[c] = 1.f / sqrtf(var[c] + eps)   -> save_var, save_invstd
//   5 bn_norm_kernel          xhat = (z - mean) * invstd; t = xhat * gamma; u = t + beta; y = act(u)
//                             (ReLU: u < 0.f ? 0.f : u, so a NaN stays a NaN; sigmoid: 1.f / (1.f + __expf(-u)), the forward kernels' own)
// Backward, three launches (two without grad_z):
//   1 bn_bwd_sums_kernel      g = act_grad(y, grad_y) (s3r_ordered.h); chunk sums of g and of g * xhat (xhat recomputed as in the
//                             forward; the product is rounded, then added)   -> scratch[0][c][b][chunk], scratch[1][c][b][chunk]
//   2 bn_finish_kernel        grad_beta[c], grad_gamma[c] (into scratch's tail when the caller passes NULL and grad_z needs them)
//   3 bn_bwd_gz_kernel        m1 = grad_beta / nf; m2 = grad_gamma / nf; a = gamma * invstd; p = xhat * m2; q = g - m1; r = q - p;
//                             grad_z = a * r
// A finish is NOT folded into its consumer: every wave of the consumer would have to re-add the channel's B * ceil(S / 512) chunk sums
// to stream 512 positions (at d3's geometry 2048 loads for 512), and a last-block-done hand-off needs an atomic counter.
//
// The order of every sum, which IS the contract, is s3r_ordered.h's, a row being the S positions of one (b, c): every streaming kernel
// gives a wave one chunk of one row, and bn_finish_kernel is one wave per channel (and sum) that takes row_total of the channel's chunk sums.
#include "s3r_ordered.h"

namespace s3r {

__device__ __forceinline__ float bn_act(float u, int act) {
#pragma clang fp contract(off)
    if (act == 1) return (u < 0.f) ? 0.f : u;
    if (act == 2) return 1.f / (1.f + __expf(-u));
    return u;
}

// what every streaming kernel starts with: the wave's row (b, c), its chunk k, the lane's first position, and whether the whole chunk
// lies inside the row (wave-uniform).  false: the wave has no chunk (the grid's tail)
struct BnWave { long long row, k, s0; int b, c, lane; bool full; };

__device__ __forceinline__ bool bn_wave(BnWave& w, int B, int C, long long S, long long nch) {
    w.lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= (long long)B * C * nch) return false;                     // (wave-uniform; the kernels have no barrier)
    w.row = wid / nch;
    w.k = wid - w.row * nch;
    w.b = (int)(w.row / C);
    w.c = (int)(w.row - (long long)w.b * C);
    w.s0 = w.k * CHUNK + 4 * w.lane;
    w.full = (w.k + 1) * CHUNK <= S;
    return true;
}

// VAR false: chunk sums of z; VAR true: of d * d with d = z - mean[c].  part: [C][B][nch]
template <bool VAR>
__global__ __launch_bounds__(256) void bn_stat_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                                                      float* __restrict__ part, int B, int C, long long S, long long nch) {
#pragma clang fp contract(off)
    BnWave w;
    if (!bn_wave(w, B, C, S, nch)) return;
    const float* __restrict__ zr = z + (size_t)w.row * S;
    v4f zv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) zv[j] = load4(zr, w.s0 + 256 * j, S, w.full);
    const float m = VAR ? mean[w.c] : 0.f;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = w.full || w.s0 + 256 * j + i < S;
            float t = zv[j][i];
            if (VAR) {
                const float d = t - m;
                t = d * d;
            }
            a = a + (in ? t : 0.f);
        }
    a = wave_tree(a);
    if (w.lane == 0) part[((size_t)w.c * B + w.b) * nch + w.k] = a;
}

// one wave per row of `part` ([rows][B][nch]).  mode 0: o0[c] = total / nf (the mean).  mode 1: o0[c] = v = total / nf (the biased
// variance), o1[c] = 1.f / sqrtf(v + eps).  mode 2: rows 0 .. C - 1 -> o0[c] (grad_beta), rows C .. 2 C - 1 -> o1[c] (grad_gamma), each
// when non-NULL
__global__ __launch_bounds__(64) void bn_finish_kernel(const float* __restrict__ part, float* __restrict__ o0, float* __restrict__ o1,
                                                       float nf, float eps, int B, int C, long long nch, int mode) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    if (mode == 2) {
        float* __restrict__ dst = r < C ? o0 : o1;
        if (!dst) return;
        const float acc = row_total(part + (size_t)r * B * nch, B, nch, lane);
        if (lane == 0) dst[r < C ? r : r - C] = acc;
        return;
    }
    const float acc = row_total(part + (size_t)r * B * nch, B, nch, lane);
    const float v = acc / nf;
    if (lane != 0) return;
    o0[r] = v;
    if (mode == 1) {
        const float e = v + eps;
        o1[r] = 1.f / sqrtf(e);
    }
}

__global__ __launch_bounds__(256) void bn_norm_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float* __restrict__ y, int B, int C, long long S,
                                                      long long nch, int act) {
#pragma clang fp contract(off)
    BnWave w;
    if (!bn_wave(w, B, C, S, nch)) return;
    const float* __restrict__ zr = z + (size_t)w.row * S;
    float* __restrict__ yr = y + (size_t)w.row * S;
    v4f zv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) zv[j] = load4(zr, w.s0 + 256 * j, S, w.full);
    const float m = mean[w.c], is = invstd[w.c], ga = gamma[w.c], be = beta[w.c];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        v4f o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = zv[j][i] - m;
            const float xh = d * is;
            const float t = xh * ga;
            const float u = t + be;
            o[i] = bn_act(u, act);
        }
        store4(yr, w.s0 + 256 * j, S, o, w.full);
    }
}

// part: [2][C][B][nch] chunk sums: of g, then (GG) of g * xhat.  GG false: z is not read
template <bool GG>
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                          const float* __restrict__ gy, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, float* __restrict__ part, int B, int C,
                                                          long long S, long long nch, int act) {
#pragma clang fp contract(off)
    BnWave w;
    if (!bn_wave(w, B, C, S, nch)) return;
    const size_t base = (size_t)w.row * S;
    v4f zv[Q], yv[Q], gv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        gv[j] = load4(gy + base, w.s0 + 256 * j, S, w.full);
        yv[j] = act ? load4(y + base, w.s0 + 256 * j, S, w.full) : v4f{0.f, 0.f, 0.f, 0.f};
        zv[j] = GG ? load4(z + base, w.s0 + 256 * j, S, w.full) : v4f{0.f, 0.f, 0.f, 0.f};
    }
    const float m = GG ? mean[w.c] : 0.f, is = GG ? invstd[w.c] : 0.f;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = w.full || w.s0 + 256 * j + i < S;
            const float g = act_grad(yv[j][i], gv[j][i], act);
            a1 = a1 + (in ? g : 0.f);
            if (GG) {
                const float d = zv[j][i] - m;
                const float xh = d * is;
                const float t = g * xh;
                a2 = a2 + (in ? t : 0.f);
            }
        }
    const size_t at = ((size_t)w.c * B + w.b) * nch + w.k;
    a1 = wave_tree(a1);
    if (w.lane == 0) part[at] = a1;
    if (GG) {
        a2 = wave_tree(a2);
        if (w.lane == 0) part[(size_t)C * B * nch + at] = a2;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_gz_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                        const float* __restrict__ gy, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gbeta, const float* __restrict__ ggamma,
                                                        float* __restrict__ gz, float nf, int B, int C, long long S, long long nch,
                                                        int act) {
#pragma clang fp contract(off)
    BnWave w;
    if (!bn_wave(w, B, C, S, nch)) return;
    const size_t base = (size_t)w.row * S;
    v4f zv[Q], yv[Q], gv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        gv[j] = load4(gy + base, w.s0 + 256 * j, S, w.full);
        yv[j] = act ? load4(y + base, w.s0 + 256 * j, S, w.full) : v4f{0.f, 0.f, 0.f, 0.f};
        zv[j] = load4(z + base, w.s0 + 256 * j, S, w.full);
    }
    const float m = mean[w.c], is = invstd[w.c];
    const float m1 = gbeta[w.c] / nf, m2 = ggamma[w.c] / nf;
    const float a = gamma[w.c] * is;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        v4f o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float g = act_grad(yv[j][i], gv[j][i], act);
            const float d = zv[j][i] - m;
            const float xh = d * is;
            const float p = xh * m2;
            const float q = g - m1;
            const float r = q - p;
            o[i] = a * r;
        }
        store4(gz + base, w.s0 + 256 * j, S, o, w.full);
    }
}

// forward: [C][B][ceil(S / 512)] chunk sums, used by both statistics passes in turn.  backward: two such blocks (g, g * xhat) and 2 C
// floats for the two sums when their outputs are NULL.  Functions of the shape only, monotone in B
int64_t batchnorm_forward_scratch_elems(int B, int C, int64_t S) { return (int64_t)C * B * chunks(S); }
int64_t batchnorm_backward_scratch_elems(int B, int C, int64_t S) { return 2 * (int64_t)C * B * chunks(S) + 2 * (int64_t)C; }

hipError_t launch_batchnorm_train_forward(const float* z, const float* gamma, const float* beta, float eps, int act, float* y,
                                          float* mean, float* var, float* invstd, int B, int C, int64_t S, float* scratch, hipStream_t s,
                                          int* launches) {
    const long long nch = chunks(S);
    const dim3 grid((unsigned)(((long long)B * C * nch + 3) / 4));
    const float nf = (float)((long long)B * S);
    hipLaunchKernelGGL((bn_stat_kernel<false>), grid, dim3(256), 0, s, z, (const float*)nullptr, scratch, B, C, (long long)S, nch);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)C), dim3(64), 0, s, scratch, mean, (float*)nullptr, nf, eps, B, C, nch, 0);
    hipLaunchKernelGGL((bn_stat_kernel<true>), grid, dim3(256), 0, s, z, mean, scratch, B, C, (long long)S, nch);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)C), dim3(64), 0, s, scratch, var, invstd, nf, eps, B, C, nch, 1);
    hipLaunchKernelGGL(bn_norm_kernel, grid, dim3(256), 0, s, z, gamma, beta, mean, invstd, y, B, C, (long long)S, nch, act);
    *launches = 5;
    return hipGetLastError();
}

hipError_t launch_batchnorm_train_backward(const float* z, const float* y, const float* gy, const float* gamma, const float* mean,
                                           const float* invstd, int act, float* gz, float* ggamma, float* gbeta, int B, int C, int64_t S,
                                           float* scratch, hipStream_t s, int* launches) {
    const long long nch = chunks(S);
    const dim3 grid((unsigned)(((long long)B * C * nch + 3) / 4));
    const float nf = (float)((long long)B * S);
    const bool gg = ggamma || gz;                                        // grad_z needs both sums
    float* tail = scratch + 2 * (size_t)C * B * nch;
    float* sb = gbeta ? gbeta : (gz ? tail : nullptr);
    float* sg = ggamma ? ggamma : (gz ? tail + C : nullptr);
    if (gg)
        hipLaunchKernelGGL((bn_bwd_sums_kernel<true>), grid, dim3(256), 0, s, z, y, gy, mean, invstd, scratch, B, C, (long long)S, nch, act);
    else
        hipLaunchKernelGGL((bn_bwd_sums_kernel<false>), grid, dim3(256), 0, s, z, y, gy, mean, invstd, scratch, B, C, (long long)S, nch, act);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)(gg ? 2 * C : C)), dim3(64), 0, s, scratch, sb, sg, nf, 0.f, B, C, nch, 2);
    *launches = 2;
    if (gz) {
        hipLaunchKernelGGL(bn_bwd_gz_kernel, grid, dim3(256), 0, s, z, y, gy, gamma, mean, invstd, sb, sg, gz, nf, B, C, (long long)S, nch, act);
        ++*launches;
    }
    return hipGetLastError();
}

}  // namespace s3r
