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
//   1 bn_bwd_sums_kernel      g = s3r_linear_backward's rule on (y, grad_y); chunk sums of g and of g * xhat (xhat recomputed as in the
//                             forward; the product is rounded, then added)   -> scratch[0][c][b][chunk], scratch[1][c][b][chunk]
//   2 bn_finish_kernel        grad_beta[c], grad_gamma[c] (into scratch's tail when the caller passes NULL and grad_z needs them)
//   3 bn_bwd_gz_kernel        m1 = grad_beta / nf; m2 = grad_gamma / nf; a = gamma * invstd; p = xhat * m2; q = g - m1; r = q - p;
//                             grad_z = a * r
// A finish is NOT folded into its consumer: every wave of the consumer would have to re-add the channel's B * ceil(S / 512) chunk sums
// to stream 512 positions (at d3's geometry 2048 loads for 512), and a last-block-done hand-off needs an atomic counter.
//
// The order of every sum, which IS the contract (head_bwd_kernel's, with a (b, c) row in place of a sample):
//   - a row's S positions are cut into chunks of 512 consecutive positions (the last may be short; missing positions count as +0.0);
//   - a WAVE owns one chunk: lane L (0..63) owns the 8 positions 256 j + 4 L + i (j = 0, 1; i = 0..3) — two 16-byte loads per lane and
//     tensor through a dword-aligned vector type — and adds its terms in ascending position to a partial that starts as +0.0; the 64
//     partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1; v[0] is the chunk's sum;
//   - bn_finish_kernel, one wave per channel (and sum): lane L adds the chunk sums of sample b0 + L in ascending chunk order into a partial
//     that starts as chunk 0's sum; the per-sample partials are added into ONE accumulator in ascending b, starting from sample 0's.
// A chunk that crosses its row's end is read and written element by element in every lane (a wave-uniform choice): the same arithmetic,
// the same bits.  Terms of positions past the row's end are replaced by +0.0 AFTER they are computed (0 * inf would be NaN), which
// changes no bit: a partial that starts as +0.0 never holds -0.0.  Waves are independent: no LDS, no barrier.
#include "s3r_kernels.h"

namespace s3r {

typedef float v4f_n __attribute__((ext_vector_type(4)));
typedef float v4f_nu __attribute__((ext_vector_type(4), aligned(4)));      // dword-aligned 16-byte access

constexpr int BN_CHUNK = 512;        // positions per wave: 2 x (64 lanes x 16 bytes)
constexpr int BN_Q = BN_CHUNK / 256; // 16-byte quads per lane

__device__ __forceinline__ v4f_n bn_load4(const float* __restrict__ p, long long i, long long n, bool full) {
    if (full) return *reinterpret_cast<const v4f_nu*>(p + i);
    v4f_n v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : 0.f;
    return v;
}

__device__ __forceinline__ void bn_store4(float* __restrict__ p, long long i, long long n, v4f_n v, bool full) {
    if (full) { *reinterpret_cast<v4f_nu*>(p + i) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) p[i + k] = v[k];
}

__device__ __forceinline__ float bn_g(float y, float gy, int act) {
#pragma clang fp contract(off)
    if (act == 1) return (y > 0.f) ? gy : 0.f;
    if (act == 2) {
        const float t = 1.f - y;
        const float u = y * t;
        return gy * u;
    }
    return gy;
}

__device__ __forceinline__ float bn_act(float u, int act) {
#pragma clang fp contract(off)
    if (act == 1) return (u < 0.f) ? 0.f : u;
    if (act == 2) return 1.f / (1.f + __expf(-u));
    return u;
}

__device__ __forceinline__ float bn_tree(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
    return v;                                                            // (lane 0 holds the tree's root)
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
    w.s0 = w.k * BN_CHUNK + 4 * w.lane;
    w.full = (w.k + 1) * BN_CHUNK <= S;
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
    v4f_n zv[BN_Q];
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) zv[j] = bn_load4(zr, w.s0 + 256 * j, S, w.full);
    const float m = VAR ? mean[w.c] : 0.f;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < BN_Q; ++j)
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
    a = bn_tree(a);
    if (w.lane == 0) part[((size_t)w.c * B + w.b) * nch + w.k] = a;
}

// the total of one row [B][nch] of chunk sums, in every lane: ascending chunk per sample starting from chunk 0's sum, then ascending b
// starting from sample 0's partial
__device__ __forceinline__ float bn_total(const float* __restrict__ part, int B, long long nch, int lane) {
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
        const float acc = bn_total(part + (size_t)r * B * nch, B, nch, lane);
        if (lane == 0) dst[r < C ? r : r - C] = acc;
        return;
    }
    const float acc = bn_total(part + (size_t)r * B * nch, B, nch, lane);
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
    v4f_n zv[BN_Q];
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) zv[j] = bn_load4(zr, w.s0 + 256 * j, S, w.full);
    const float m = mean[w.c], is = invstd[w.c], ga = gamma[w.c], be = beta[w.c];
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) {
        v4f_n o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = zv[j][i] - m;
            const float xh = d * is;
            const float t = xh * ga;
            const float u = t + be;
            o[i] = bn_act(u, act);
        }
        bn_store4(yr, w.s0 + 256 * j, S, o, w.full);
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
    v4f_n zv[BN_Q], yv[BN_Q], gv[BN_Q];
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) {
        gv[j] = bn_load4(gy + base, w.s0 + 256 * j, S, w.full);
        yv[j] = act ? bn_load4(y + base, w.s0 + 256 * j, S, w.full) : v4f_n{0.f, 0.f, 0.f, 0.f};
        zv[j] = GG ? bn_load4(z + base, w.s0 + 256 * j, S, w.full) : v4f_n{0.f, 0.f, 0.f, 0.f};
    }
    const float m = GG ? mean[w.c] : 0.f, is = GG ? invstd[w.c] : 0.f;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < BN_Q; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = w.full || w.s0 + 256 * j + i < S;
            const float g = bn_g(yv[j][i], gv[j][i], act);
            a1 = a1 + (in ? g : 0.f);
            if (GG) {
                const float d = zv[j][i] - m;
                const float xh = d * is;
                const float t = g * xh;
                a2 = a2 + (in ? t : 0.f);
            }
        }
    const size_t at = ((size_t)w.c * B + w.b) * nch + w.k;
    a1 = bn_tree(a1);
    if (w.lane == 0) part[at] = a1;
    if (GG) {
        a2 = bn_tree(a2);
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
    v4f_n zv[BN_Q], yv[BN_Q], gv[BN_Q];
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) {
        gv[j] = bn_load4(gy + base, w.s0 + 256 * j, S, w.full);
        yv[j] = act ? bn_load4(y + base, w.s0 + 256 * j, S, w.full) : v4f_n{0.f, 0.f, 0.f, 0.f};
        zv[j] = bn_load4(z + base, w.s0 + 256 * j, S, w.full);
    }
    const float m = mean[w.c], is = invstd[w.c];
    const float m1 = gbeta[w.c] / nf, m2 = ggamma[w.c] / nf;
    const float a = gamma[w.c] * is;
#pragma unroll
    for (int j = 0; j < BN_Q; ++j) {
        v4f_n o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float g = bn_g(yv[j][i], gv[j][i], act);
            const float d = zv[j][i] - m;
            const float xh = d * is;
            const float p = xh * m2;
            const float q = g - m1;
            const float r = q - p;
            o[i] = a * r;
        }
        bn_store4(gz + base, w.s0 + 256 * j, S, o, w.full);
    }
}

static long long bn_chunks(int64_t S) { return ((long long)S + BN_CHUNK - 1) / BN_CHUNK; }

// forward: [C][B][ceil(S / 512)] chunk sums, used by both statistics passes in turn.  backward: two such blocks (g, g * xhat) and 2 C
// floats for the two sums when their outputs are NULL.  Functions of the shape only, monotone in B
int64_t batchnorm_forward_scratch_elems(int B, int C, int64_t S) { return (int64_t)C * B * bn_chunks(S); }
int64_t batchnorm_backward_scratch_elems(int B, int C, int64_t S) { return 2 * (int64_t)C * B * bn_chunks(S) + 2 * (int64_t)C; }

hipError_t launch_batchnorm_train_forward(const float* z, const float* gamma, const float* beta, float eps, int act, float* y,
                                          float* mean, float* var, float* invstd, int B, int C, int64_t S, float* scratch, hipStream_t s,
                                          int* launches) {
    const long long nch = bn_chunks(S);
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
    const long long nch = bn_chunks(S);
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
