// Backward of the soft disparity read-out (s3r_disparity_soft_backward): the gradient of sum grad_disp_l disp_l + sum grad_disp_r disp_r
// with respect to the two feature maps, for the maps s3r_disparity_soft (s3r_disparity.hip) writes at the feature size or upsampled.
// Nothing is saved by the forward: costs, minimum, weights, Z, S and disp are recomputed here with the forward's operations in the
// forward's order (the costs are the forward's bit for bit; every operation below is rounded once, nothing is contracted).
//
// Per sample, direction X in {L, R} and feature pixel (h, w), fp32 (include/s3r.h has the contract):
//   G     the feature-size gradient: grad_disp_X[h,w] * disp_scale at the feature size, otherwise the adjoint of the forward's bilinear
//         blend, gathered over the output pixels that read (h, w): rows ascending, columns ascending within a row, ONE accumulator
//         that starts as +0.0:  acc = acc + ((g[oy,ox] * disp_scale) * wy) * wx,  wy = (i0 == h ? 1 - lam : 0) + (i1 == h ? lam : 0)
//   k = G / tau;  p_d = e_d / Z;  t_d = p_d * (disp - (float)d);  q_d = t_d * k             (= d loss / d c(d))
//   grad_left [c,h,w] = sum_{d < n_L(w)} sgn(L[c,h,w] - R[c,h,w-d]) (q^L_d(h,w) + q^R_d(h,w-d))
//   grad_right[c,h,w] = sum_{d < n_R(w)} sgn(R[c,h,w] - L[c,h,w+d]) (q^R_d(h,w) + q^L_d(h,w+d))
// the inner sum one add, the term that sum, its negation or 0; the accumulator starts AS the d = 0 term and takes the others one at a
// time in ascending d.  Every output is its own sequential sum: no atomics, no cross-lane reduction, no scratch.
//
// One launch, one workgroup of 256 per (sample, feature row):
//   1. the row pair is staged as fp32 [C][W] in LDS, as the forward stages it;
//   2. one thread per (direction, pixel) gathers G into LDS.  The output rows that read feature row h are those whose lower source
//      index i0 is h - 1 or h, and i0 is monotone in the output index: the rows — and likewise the columns of a pixel — form one
//      contiguous window, found by two binary searches over bilinear_src;
//   3. costs, then weights, then q in ONE LDS region of 2 W min(D, W) floats, each overwriting the last.  The region is laid out
//      [2][min(D, W)][W] — d-major, NOT the forward's [2][W][min(D, W)]: consecutive lanes hold consecutive w in the softmax (one
//      thread per pixel walks d) and in step 4, so every ds_read_b32 / ds_write_b32 of a 32-lane half touches 32 consecutive dwords:
//      no bank conflict (32 banks for these instructions), where the pixel-major layout puts the lanes min(D, W) = 28 dwords apart
//      (8 distinct banks, a 4-way conflict).  The cost pass walks w fastest as well, so its feature reads are consecutive too;
//   4. one thread per (tensor, c, w), w fastest, runs the ascending-d sum: consecutive lanes store consecutive w.
// LDS: 4 (2 C W + 2 W min(D, W) + 2 W) bytes, within the forward's rule 4 (2 C W + 2 W min(D, W) + 12 W): the limit is the forward's.
#include "s3r_kernels.h"

#include <cfloat>

namespace s3r {

// (the forward's rule, s3r_disparity.hip: evaluated in fp32 with nothing contracted, on the host and the device alike)
struct BilinSrcB {
    int i0, i1;
    float lam;
};

__device__ __forceinline__ BilinSrcB bilinear_src_b(int dst, int in, float scale) {
#pragma clang fp contract(off)
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    int i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    BilinSrcB r;
    r.i0 = i0;
    r.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    r.lam = s - (float)i0;
    return r;
}

// the first output index in [0, n_out] whose lower source index is >= t (i0 is monotone non-decreasing in the output index)
__device__ __forceinline__ int first_i0_at_least(int t, int n_out, int in, float scale) {
    int lo = 0, hi = n_out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bilinear_src_b(mid, in, scale).i0 >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the weight with which output index o reads source index i: both neighbours' weights where an edge clamp made them one
__device__ __forceinline__ float bilinear_weight(BilinSrcB r, int i) {
#pragma clang fp contract(off)
    const float a = r.i0 == i ? 1.f - r.lam : 0.f;
    const float b = r.i1 == i ? r.lam : 0.f;
    return a + b;
}

__global__ __launch_bounds__(256) void disparity_soft_bwd_kernel(const float* __restrict__ fl, const float* __restrict__ fr,
                                                                 const float* __restrict__ gdl, const float* __restrict__ gdr,
                                                                 float* __restrict__ gl, float* __restrict__ gr, int C, int D, int H,
                                                                 int W, float tau, int OH, int OW, float sh, float sw,
                                                                 float disp_scale) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float db_smem[];
    const int dm = D < W ? D : W;
    float* sl = db_smem;                      // [C][W] left feature row
    float* sr = sl + C * W;                   // [C][W] right feature row
    float* q = sr + C * W;                    // [2][dm][W]: costs, then weights, then q
    float* G = q + 2 * dm * W;                // [2][W] feature-size gradient
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const size_t plane = (size_t)H * W;
    const bool same = OH == H && OW == W;

    {   // 1. the row pair
        const float* __restrict__ pl = fl + (size_t)b * C * plane + (size_t)h * W;
        const float* __restrict__ pr = fr + (size_t)b * C * plane + (size_t)h * W;
        for (int i = threadIdx.x; i < C * W; i += 256) {
            const int c = i / W, w = i - c * W;
            sl[i] = pl[(size_t)c * plane + w];
            sr[i] = pr[(size_t)c * plane + w];
        }
    }
    // 2. G: one thread per (direction, pixel)
    int y0 = 0, y1 = -1;
    if (!same) {
        y0 = first_i0_at_least(h - 1, OH, H, sh);
        y1 = first_i0_at_least(h + 1, OH, H, sh) - 1;
    }
    for (int o = threadIdx.x; o < 2 * W; o += 256) {
        const bool right = o >= W;
        const int w = right ? o - W : o;
        const float* __restrict__ g = right ? gdr : gdl;
        float acc = 0.f;
        if (g) {
            g += (size_t)b * OH * OW;
            if (same) {
                acc = g[(size_t)h * OW + w] * disp_scale;
            } else {
                const int x0 = first_i0_at_least(w - 1, OW, W, sw), x1 = first_i0_at_least(w + 1, OW, W, sw) - 1;
                for (int oy = y0; oy <= y1; ++oy) {
                    const float wy = bilinear_weight(bilinear_src_b(oy, H, sh), h);
                    const float* __restrict__ grow = g + (size_t)oy * OW;
                    for (int ox = x0; ox <= x1; ++ox) {
                        const float wx = bilinear_weight(bilinear_src_b(ox, W, sw), w);
                        const float gs = grow[ox] * disp_scale;
                        acc = acc + (gs * wy) * wx;
                    }
                }
            }
        }
        G[o] = acc;
    }
    __syncthreads();
    // 3a. costs, the forward's bit for bit: one thread per (direction, d, pixel), w fastest
    for (int i = threadIdx.x; i < 2 * dm * W; i += 256) {
        const bool right = i >= dm * W;
        const int j = right ? i - dm * W : i;
        const int d = j / W, w = j - d * W;
        const int dmax = right ? (W - 1 - w) : w;
        if (d > dmax) continue;
        const float* a = right ? sr : sl;
        const float* m = right ? sl : sr;
        const int wm = right ? w + d : w - d;
        float c = 0.f;
#pragma unroll 8
        for (int k = 0; k < C; ++k) c = c + fabsf(a[k * W + w] - m[k * W + wm]);
        q[i] = c;
    }
    __syncthreads();
    // 3b. softmax and q: one thread per (direction, pixel), d ascending
    for (int o = threadIdx.x; o < 2 * W; o += 256) {
        const bool right = o >= W;
        const int w = right ? o - W : o;
        const int dmax = right ? (W - 1 - w) : w;
        const int n = (dmax < D - 1 ? dmax : D - 1) + 1;
        float* cc = q + (right ? dm * W : 0) + w;                    // element d at cc[d * W]
        float mn = cc[0];
        for (int d = 1; d < n; ++d) mn = fminf(mn, cc[d * W]);
        float z = 0.f, s = 0.f;
#pragma unroll 4
        for (int d = 0; d < n; ++d) {
            float e = expf((mn - cc[d * W]) / tau);
            if (e < FLT_MIN) e = 0.f;
            cc[d * W] = e;
            z = z + e;
            s = s + (float)d * e;
        }
        const float disp = s / z;
        const float k = G[o] / tau;
#pragma unroll 4
        for (int d = 0; d < n; ++d) {
            const float p = cc[d * W] / z;
            const float t = p * (disp - (float)d);
            cc[d * W] = t * k;
        }
    }
    __syncthreads();
    // 4. one thread per (tensor, c, w): its own sequential sum over ascending d
    const int cw = C * W;
    for (int i = threadIdx.x; i < 2 * cw; i += 256) {
        const bool right = i >= cw;
        float* __restrict__ out = right ? gr : gl;
        if (!out) continue;
        const int j = right ? i - cw : i;
        const int c = j / W, w = j - c * W;
        const int n = right ? (D < W - w ? D : W - w) : (D < w + 1 ? D : w + 1);
        const float* own = (right ? sr : sl) + c * W;
        const float* oth = (right ? sl : sr) + c * W;
        const float* qo = q + (right ? dm * W : 0);                  // the own direction's q
        const float* qx = q + (right ? 0 : dm * W);                  // the other direction's
        const float a = own[w];
        float acc = 0.f;
        for (int d = 0; d < n; ++d) {
            const int wm = right ? w + d : w - d;
            const float m = oth[wm];
            const float sum = qo[d * W + w] + qx[d * W + wm];
            const float term = (a > m) ? sum : ((a < m) ? -sum : 0.f);
            acc = d == 0 ? term : acc + term;
        }
        out[((size_t)b * C + c) * plane + (size_t)h * W + w] = acc;
    }
}

size_t disparity_soft_bwd_lds_bytes(int C, int D, int W) {
    const int dm = D < W ? D : W;
    return sizeof(float) * ((size_t)2 * C * W + (size_t)2 * W * dm + (size_t)2 * W);
}

hipError_t launch_disparity_soft_backward(const float* fl, const float* fr, const float* gdl, const float* gdr, float* gl, float* gr,
                                          int B, int C, int D, int H, int W, float tau, int OH, int OW, float disp_scale,
                                          hipStream_t s) {
    const size_t lds = disparity_soft_bwd_lds_bytes(C, D, W);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
    hipLaunchKernelGGL(disparity_soft_bwd_kernel, dim3((unsigned)((int64_t)B * H)), dim3(256), lds, s, fl, fr, gdl, gdr, gl, gr, C, D,
                       H, W, tau, OH, OW, sh, sw, disp_scale);
    return hipGetLastError();
}

}  // namespace s3r
