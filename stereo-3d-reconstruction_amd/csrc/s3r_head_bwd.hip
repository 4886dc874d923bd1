// Backward of the pointwise head  y[b][s] = act(fmaf(sum_c x[b][c][s] w[c], scale, shift))  (s3r_head_backward; the forward is
// head_kernel in s3r_pointwise.hip): x (B,C,S), w (C), scale one float or NULL, y and grad_y (B,S), act none / ReLU / sigmoid.  Three
// results, each optional, each with a FIXED order — no atomics, the same bits on every run and at every 4-byte-aligned address:
//
//   g (B,S), the pre-activation gradient, fp32, nothing fused: act_grad (s3r_ordered.h)
//   gs = g * scale, rounded once (g itself when scale is NULL)
//   grad_x[b][c][s] = gs[b][s] * w[c]            one multiplication
//   grad_w[c]       = sum_{b,s} gs[b][s] x[b][c][s]
//   grad_shift      = sum_{b,s} g[b][s]
//
// The order of every sum is s3r_ordered.h's, a row being one sample's S positions.  head_bwd_kernel streams the tensors once: a WAVE owns
// one chunk of one sample.  g and gs of the lane's eight positions are computed once and kept in registers; then the wave walks ALL C
// channels of its positions — one read of x serves every channel sum — four channels' loads (8 per lane) in flight at a time:
//   - grad_x: 16-byte stores of gs * w[c];
//   - grad_w: the lane's partial takes partial = partial + gs * x over its positions (the product is rounded, then the add: NOT fused — a
//     numpy restatement is then exact, and the kernel has VALU time to spare); the chunk sum goes to scratch[c][b][chunk];
//   - grad_shift: the same with plain adds of g, stored to scratch[C][b][chunk].
// Positions past S contribute +0.0 (gs and x are both replaced by 0: 0 * NaN would be NaN).  A wave holds no channel state between
// channels, so C is unbounded.
//
// head_bwd_finish_kernel: one wave per channel (and one for grad_shift): row_total's sum of its row of scratch, written out in the kernel.
//
// Templates: GW / GX switch the x loads and the grad_x stores off entirely — grad_x NULL does not cost its write, grad_w NULL does
// not cost the read of x; with neither, the channel loop is gone (grad_shift alone reads y and grad_y only).
#include "s3r_ordered.h"

namespace s3r {

constexpr int HB_UC = 4;             // channels whose loads are in flight together

// channels c0 .. c0 + N - 1 (all < C) of one wave's chunk: the N channels' loads first, then per channel the stores and the chunk sum
template <bool GW, bool GX, int N, bool FULL>
__device__ __forceinline__ void hb_channels(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ gx,
                                            float* __restrict__ part, const float (&gs)[Q][4], int B, int C, long long S,
                                            long long nch, long long b, long long k, long long s0, int c0, int lane) {
#pragma clang fp contract(off)
    v4f xv[N][Q];
    if (GW) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float* __restrict__ xr = x + ((size_t)b * C + c0 + u) * S;
#pragma unroll
            for (int j = 0; j < Q; ++j) xv[u][j] = load4(xr, s0 + 256 * j, S, FULL);
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int c = c0 + u;
        if (GX) {
            const float wc = w[c];
            float* __restrict__ gr = gx + ((size_t)b * C + c) * S;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                v4f o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = gs[j][i] * wc;
                store4(gr, s0 + 256 * j, S, o, FULL);
            }
        }
        if (GW) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < Q; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) a = a + gs[j][i] * xv[u][j][i];
            a = wave_tree(a);
            if (lane == 0) part[((size_t)c * B + b) * nch + k] = a;
        }
    }
}

// part: [C + 1][B][nch] chunk sums (row C: grad_shift); shift != 0: the grad_shift row is wanted
template <bool GW, bool GX>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ scale, const float* __restrict__ y,
                                                       const float* __restrict__ gy, float* __restrict__ gx, float* __restrict__ part,
                                                       int B, int C, long long S, long long nch, int act, int shift) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= (long long)B * nch) return;                               // (wave-uniform; the kernel has no barrier)
    const long long b = wid / nch, k = wid - b * nch;
    const long long s0 = k * CHUNK + 4 * lane;
    const bool full = (k + 1) * CHUNK <= S;                           // (wave-uniform)
    const float sc = scale ? scale[0] : 1.f;
    float g[Q][4], gs[Q][4];
    {
        v4f gv[Q], yv[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            gv[j] = load4(gy + (size_t)b * S, s0 + 256 * j, S, full);
            yv[j] = act ? load4(y + (size_t)b * S, s0 + 256 * j, S, full) : v4f{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < Q; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool in = s0 + 256 * j + i < S;
                const float v = act_grad(yv[j][i], gv[j][i], act);
                g[j][i] = in ? v : 0.f;
                gs[j][i] = in ? (scale ? v * sc : v) : 0.f;
            }
    }
    if (shift) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < Q; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) a = a + g[j][i];
        a = wave_tree(a);
        if (lane == 0) part[((size_t)C * B + b) * nch + k] = a;
    }
    if (!GW && !GX) return;
    int c0 = 0;
    if (full) {                                                          // (the streaming path: straight-line 16-byte accesses)
        for (; c0 + HB_UC <= C; c0 += HB_UC) hb_channels<GW, GX, HB_UC, true>(x, w, gx, part, gs, B, C, S, nch, b, k, s0, c0, lane);
        for (; c0 < C; ++c0) hb_channels<GW, GX, 1, true>(x, w, gx, part, gs, B, C, S, nch, b, k, s0, c0, lane);
    } else {                                                             // (a sample's last, short chunk)
        for (; c0 < C; ++c0) hb_channels<GW, GX, 1, false>(x, w, gx, part, gs, B, C, S, nch, b, k, s0, c0, lane);
    }
}

// one wave per row of `part`: rows 0 .. C - 1 -> grad_w (when asked for), row C -> grad_shift (when asked for)
__global__ __launch_bounds__(64) void head_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ gw,
                                                             float* __restrict__ gshift, int B, int C, long long nch) {
#pragma clang fp contract(off)
    const int c = blockIdx.x, lane = threadIdx.x;
    float* __restrict__ dst = c < C ? (gw ? gw + c : nullptr) : gshift;
    if (!dst) return;
    // row_total (s3r_ordered.h) with the row's base folded into each sample's address: the call itself measured 0.3 us slower (4.7 -> 5.0)
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        float p = 0.f;
        if (b < B) {
            const float* __restrict__ src = part + ((size_t)c * B + b) * nch;
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
    if (lane == 0) *dst = acc;
}

// [C + 1][B][ceil(S / 512)] chunk sums: the worst case over the outputs, a function of the shape only, monotone in B
int64_t head_backward_scratch_elems(int B, int C, int64_t S) { return ((int64_t)C + 1) * B * chunks(S); }

hipError_t launch_head_backward(const float* x, const float* w, const float* scale, const float* y, const float* gy, float* gx,
                                float* gw, float* gshift, int B, int C, int64_t S, int act, float* scratch, hipStream_t s,
                                int* launches) {
    const long long nch = chunks(S);
    const dim3 grid((unsigned)(((long long)B * nch + 3) / 4));
    const int shift = gshift != nullptr;
#define S3R_HB_LAUNCH(GW, GX) \
    hipLaunchKernelGGL((head_bwd_kernel<GW, GX>), grid, dim3(256), 0, s, x, w, scale, y, gy, gx, scratch, B, C, (long long)S, nch, act, shift)
    if (gw && gx) S3R_HB_LAUNCH(true, true);
    else if (gw) S3R_HB_LAUNCH(true, false);
    else if (gx) S3R_HB_LAUNCH(false, true);
    else S3R_HB_LAUNCH(false, false);
#undef S3R_HB_LAUNCH
    *launches = 1;
    if (gw || gshift) {
        hipLaunchKernelGGL(head_bwd_finish_kernel, dim3((unsigned)(C + 1)), dim3(64), 0, s, scratch, gw, gshift, B, C, nch);
        ++*launches;
    }
    return hipGetLastError();
}

}  // namespace s3r
