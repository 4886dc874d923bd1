// Sub-pixel disparity read-out at any output resolution, and the stereo error metrics.
//
// Soft read-out: a soft-argmin over the SAME shift-and-diff costs the winner-take-all read-out (disparity_wta_kernel,
// s3r_pointwise.hip) takes the argmin of, upsampled bilinearly to the caller's output size, with the probability of the best
// disparity as an optional confidence map.  Still a stand-in read-out: no learned head, the temperature is the caller's.
//   c(d)  = sum_{c=0..C-1} |A[c,h,w] - M[c,h,w -/+ d]|, d in [0, n-1], n = min(D-1, w)+1 (left) / min(D-1, W-1-w)+1 (right):
//           fp32, c ascending, |a-b| then add — bit for bit the WTA's costs
//   e_d   = expf((min_d c(d) - c(d)) / tau), IEEE expf; a weight that would be subnormal is taken as 0 (it is below 2^-126 of the
//           best disparity's weight 1, so it cannot move Z; it would only leave a subnormal residue in S when the best d is 0)
//   disp  = S / Z, conf = 1 / Z with Z = sum e_d, S = sum d e_d (d ascending); D = 1 gives exactly 0 and 1
// then, unless the output size is the feature size, bilinear with torch's align_corners=False convention; disp x disp_scale.
//
// One launch for both directions and all samples: one workgroup per (sample, band of R output rows).  The band's feature rows
// (at most kSoftMaxRows, the host picks R so) are processed one at a time: the row pair is staged in LDS as fp32 [C][W] (the bf16
// channels-last input widens exactly on the way in), the 2 W min(D, W) costs are spread over the workgroup's threads, one thread
// per (direction, pixel) runs the softmax over them, and the soft values stay in LDS for the band's interpolation.  A feature row
// shared by two bands is computed by both: that recomputation is cheaper than a round trip through HBM.
#include "s3r_kernels.h"

#include <cfloat>

namespace s3r {

typedef unsigned v4u_d __attribute__((ext_vector_type(4)));

constexpr int kSoftMaxRows = 3;          // feature rows one workgroup computes (s3r.h's LDS rule counts 4 kSoftMaxRows W floats)

struct BilinSrc {
    int i0, i1;
    float lam;
};

// torch's upsample_bilinear2d source index (align_corners=False): src = scale (dst + 0.5) - 0.5 clamped at 0, scale = in / out
// in fp32; the upper neighbour clamped at in - 1.  Evaluated on the host (band planning) and the device (interpolation): no
// contraction, so both see the same i0 / i1.
__host__ __device__ inline BilinSrc bilinear_src(int dst, int in, float scale) {
#pragma clang fp contract(off)
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    int i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    BilinSrc r;
    r.i0 = i0;
    r.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    r.lam = s - (float)i0;
    return r;
}

size_t disparity_soft_lds_bytes(int C, int D, int W) {
    const int dm = D < W ? D : W;
    return sizeof(float) * ((size_t)2 * C * W + (size_t)2 * W * dm + (size_t)4 * kSoftMaxRows * W);
}

__device__ __forceinline__ float bf16_lo(unsigned x) { return __uint_as_float(x << 16); }
__device__ __forceinline__ float bf16_hi(unsigned x) { return __uint_as_float(x & 0xffff0000u); }

template <bool BF16>
__global__ __launch_bounds__(256) void disparity_soft_kernel(const void* __restrict__ fl_, const void* __restrict__ fr_,
                                                             float* __restrict__ dl, float* __restrict__ dr,
                                                             float* __restrict__ cl, float* __restrict__ cr, int C, int D,
                                                             int H, int W, float tau, int OH, int OW, int R, int nbands,
                                                             float sh, float sw, float disp_scale) {
    extern __shared__ __attribute__((aligned(16))) float ds_smem[];
    const int dm = D < W ? D : W;
    float* sl = ds_smem;                      // [C][W] left feature row
    float* sr = sl + C * W;                   // [C][W] right feature row
    float* cost = sr + C * W;                 // [2][W][dm]
    float* soft = cost + 2 * W * dm;          // [kSoftMaxRows][4][W]: disp_l, disp_r, conf_l, conf_r
    const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
    const int oh0 = band * R, oh1 = min(OH, oh0 + R);
    const bool same = OH == H && OW == W;
    const int ha = same ? oh0 : bilinear_src(oh0, H, sh).i0;
    const int hb = same ? oh1 - 1 : bilinear_src(oh1 - 1, H, sh).i1;
    const int nrows = min(hb - ha + 1, kSoftMaxRows);
    const size_t plane = (size_t)H * W;

    for (int r = 0; r < nrows; ++r) {
        const int hh = ha + r;
        // stage the row pair as fp32 [C][W]; the previous row's costs were all read before its softmax barrier
        if (BF16) {
            const int cg = C >> 3;
            const size_t row = ((size_t)b * H + hh) * W * C;
            const v4u_d* __restrict__ pl = reinterpret_cast<const v4u_d*>(reinterpret_cast<const unsigned short*>(fl_) + row);
            const v4u_d* __restrict__ pr = reinterpret_cast<const v4u_d*>(reinterpret_cast<const unsigned short*>(fr_) + row);
            for (int i = threadIdx.x; i < W * cg; i += 256) {
                const int w = i / cg, c0 = (i - w * cg) * 8;
                const v4u_d a = pl[i], m = pr[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sl[(c0 + 2 * k) * W + w] = bf16_lo(a[k]);
                    sl[(c0 + 2 * k + 1) * W + w] = bf16_hi(a[k]);
                    sr[(c0 + 2 * k) * W + w] = bf16_lo(m[k]);
                    sr[(c0 + 2 * k + 1) * W + w] = bf16_hi(m[k]);
                }
            }
        } else {
            const float* __restrict__ pl = reinterpret_cast<const float*>(fl_) + (size_t)b * C * plane + (size_t)hh * W;
            const float* __restrict__ pr = reinterpret_cast<const float*>(fr_) + (size_t)b * C * plane + (size_t)hh * W;
            for (int i = threadIdx.x; i < C * W; i += 256) {
                const int c = i / W, w = i - c * W;
                sl[i] = pl[(size_t)c * plane + w];
                sr[i] = pr[(size_t)c * plane + w];
            }
        }
        __syncthreads();
        // costs: one thread per (direction, pixel, d); consecutive lanes walk d, so the matched view's reads are consecutive
        for (int i = threadIdx.x; i < 2 * W * dm; i += 256) {
            const bool right = i >= W * dm;
            const int j = right ? i - W * dm : i;
            const int w = j / dm, d = j - w * dm;
            const int dmax = right ? (W - 1 - w) : w;
            if (d > dmax) continue;                                  // (d < dm <= D already)
            const float* a = right ? sr : sl;
            const float* m = right ? sl : sr;
            const int wm = right ? w + d : w - d;
            float c = 0.f;
#pragma unroll 8
            for (int k = 0; k < C; ++k) c = c + fabsf(a[k * W + w] - m[k * W + wm]);   // (unrolled: the LDS reads issue ahead)
            cost[i] = c;
        }
        __syncthreads();
        // softmax: one thread per (direction, pixel), d ascending
        for (int o = threadIdx.x; o < 2 * W; o += 256) {
            const bool right = o >= W;
            const int w = right ? o - W : o;
            const int dmax = right ? (W - 1 - w) : w;
            const int n = (dmax < D - 1 ? dmax : D - 1) + 1;
            const float* cc = cost + (right ? W * dm : 0) + w * dm;
            float mn = cc[0];
            for (int d = 1; d < n; ++d) mn = fminf(mn, cc[d]);
            float z = 0.f, s = 0.f;
#pragma unroll 4
            for (int d = 0; d < n; ++d) {
                float e = expf((mn - cc[d]) / tau);
                if (e < FLT_MIN) e = 0.f;
                z = z + e;
                s = s + (float)d * e;
            }
            soft[(r * 4 + (right ? 1 : 0)) * W + w] = s / z;
            soft[(r * 4 + (right ? 3 : 2)) * W + w] = 1.f / z;
        }
        __syncthreads();
    }

    const int nout = (oh1 - oh0) * OW;
    for (int i = threadIdx.x; i < nout; i += 256) {
        const int oy = i / OW, ox = i - oy * OW;
        const int oh = oh0 + oy;
        float v[4];
        if (same) {
            const float* p = soft + (size_t)(oh - ha) * 4 * W + ox;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[k * W];
        } else {
            const BilinSrc ry = bilinear_src(oh, H, sh), rx = bilinear_src(ox, W, sw);
            const int s0 = min(max(ry.i0 - ha, 0), nrows - 1), s1 = min(max(ry.i1 - ha, 0), nrows - 1);
            const float h1l = ry.lam, h0l = 1.f - h1l, w1l = rx.lam, w0l = 1.f - w1l;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* p0 = soft + (s0 * 4 + k) * W;
                const float* p1 = soft + (s1 * 4 + k) * W;
                v[k] = h0l * (w0l * p0[rx.i0] + w1l * p0[rx.i1]) + h1l * (w0l * p1[rx.i0] + w1l * p1[rx.i1]);
            }
        }
        const size_t o = ((size_t)b * OH + oh) * OW + ox;
        if (dl) dl[o] = v[0] * disp_scale;
        if (dr) dr[o] = v[1] * disp_scale;
        if (cl) cl[o] = v[2];
        if (cr) cr[o] = v[3];
    }
}

// Output rows per workgroup: the largest R <= 8 whose every band needs at most kSoftMaxRows feature rows (R = 1 always does:
// two rows at most); one row per workgroup at the feature size, where bands share no feature row.
static int disparity_soft_rows(int H, int OH, float sh, bool same) {
    if (same) return 1;
    for (int R = 8; R > 1; --R) {
        bool ok = true;
        for (int oh0 = 0; oh0 < OH && ok; oh0 += R) {
            const int oh1 = OH < oh0 + R ? OH : oh0 + R;
            ok = bilinear_src(oh1 - 1, H, sh).i1 - bilinear_src(oh0, H, sh).i0 + 1 <= kSoftMaxRows;
        }
        if (ok) return R;
    }
    return 1;
}

hipError_t launch_disparity_soft(const void* fl, const void* fr, int bf16, float* dl, float* dr, float* cl, float* cr, int B,
                                 int C, int D, int H, int W, float tau, int OH, int OW, float disp_scale, hipStream_t s) {
    const size_t lds = disparity_soft_lds_bytes(C, D, W);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const bool same = OH == H && OW == W;
    const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
    const int R = disparity_soft_rows(H, OH, sh, same);
    const int nbands = (OH + R - 1) / R;
    const dim3 grid((unsigned)((int64_t)B * nbands));
    if (bf16)
        hipLaunchKernelGGL(disparity_soft_kernel<true>, grid, dim3(256), lds, s, fl, fr, dl, dr, cl, cr, C, D, H, W, tau, OH, OW,
                           R, nbands, sh, sw, disp_scale);
    else
        hipLaunchKernelGGL(disparity_soft_kernel<false>, grid, dim3(256), lds, s, fl, fr, dl, dr, cl, cr, C, D, H, W, tau, OH,
                           OW, R, nbands, sh, sw, disp_scale);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Stereo metrics per sample: the end-point error exactly as disparity_epe_kernel computes it (same loop, same fixed fp64 order:
// the same bits) and four integer counts over the valid pixels (ground truth finite and >= 0): valid, |err| > 1, |err| > 3,
// D1 (|err| > 3 and |err| > 0.05 gt, the product in fp64).  Comparisons are strict.  Integer counts pool exactly over samples
// and ranks.
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void disparity_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                float* __restrict__ epe, int* __restrict__ counts, long long S) {
    __shared__ double psum[4];
    __shared__ unsigned pcnt[4][4];
    const float* __restrict__ p = pred + (size_t)blockIdx.x * S;
    const float* __restrict__ g = gt + (size_t)blockIdx.x * S;
    double sum = 0.0;
    unsigned n[4] = {0u, 0u, 0u, 0u};
#pragma unroll 4
    for (long long i = threadIdx.x; i < S; i += 256) {         // (unrolled: loads issue ahead; the fp64 sum keeps its order)
        const float t = g[i];
        const bool ok = (t >= 0.f) && (t < __builtin_inff());       // false for NaN as well
        if (ok) {
            const float e = fabsf(p[i] - t);
            sum += (double)e;
            ++n[0];
            n[1] += e > 1.f;
            n[2] += e > 3.f;
            n[3] += (e > 3.f) && ((double)e > 0.05 * (double)t);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] = wave_sum_u(n[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        psum[wave] = sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) pcnt[k][wave] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const unsigned c4 = pcnt[k][0] + pcnt[k][1] + pcnt[k][2] + pcnt[k][3];
        counts[(size_t)blockIdx.x * 4 + k] = (int)c4;
        if (k == 0) {
            const double s4 = ((psum[0] + psum[1]) + psum[2]) + psum[3];
            epe[blockIdx.x] = c4 ? (float)(s4 / (double)c4) : 0.f;
        }
    }
}

hipError_t launch_disparity_metrics(const float* pred, const float* gt, float* epe, int* counts, int B, int64_t S,
                                    hipStream_t s) {
    hipLaunchKernelGGL(disparity_metrics_kernel, dim3(B), dim3(256), 0, s, pred, gt, epe, counts, (long long)S);
    return hipGetLastError();
}

}  // namespace s3r
