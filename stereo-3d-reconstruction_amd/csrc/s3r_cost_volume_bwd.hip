// Backward of the cost volume (s3r_cost_volume_backward).  The forward writes, per (b, c, d, h, w),
//   vol[b,   c, d, h, w] = L[b,c,h,w] - R[b,c,h,w-d]   (w >= d,    else the constant 0)
//   vol[b, C+c, d, h, w] = R[b,c,h,w] - L[b,c,h,w+d]   (w + d < W, else the constant 0)
// so with gv = grad_volume (B, 2C, D, H, W), n_L(w) = min(D, w + 1) and n_R(w) = min(D, W - w):
//   grad_left [b,c,h,w] = sum_{d < n_L(w)} ( gv[b,  c,d,h,w] - gv[b,C+c,d,h,w-d] )
//   grad_right[b,c,h,w] = sum_{d < n_R(w)} ( gv[b,C+c,d,h,w] - gv[b,  c,d,h,w+d] )
// Every position the two sums name is a LIVE position of its slab (left slab: w >= d; right slab: w + d < W): gv[b,c,d,h,w] with
// d < n_L(w) has w >= d, gv[b,C+c,d,h,w-d] has (w - d) + d = w < W, and likewise for the other sum.  The structural zeros of the
// forward — and every plane d >= W — are therefore never loaded at all.
//
// Order (the contract, include/s3r.h): per output element the difference t_d is one fp32 subtraction, the accumulator starts AS t_0 (not
// as +0.0: -0.0 + +0.0 would lose the sign) and t_1, t_2, ... are added one at a time in ascending d.  Contraction is off and there is
// no multiplication to fuse.  One thread owns one (b, c, h, w) and both of its outputs; nothing crosses lanes, no LDS, no atomics, no
// scratch: the bits are a function of the element's own terms only.
//
// Memory.  Consecutive threads own consecutive w, so every load instruction of a wave reads one contiguous 256-byte run (less a row
// wrap) of one plane: the aligned operand at the thread's own position, the shifted one d floats to the side in the same row.  A
// position of gv is read once as an aligned and once as a shifted operand, by neighbouring lanes of the same workgroup in the same
// iteration: the second read is served by the L1 / L2, and HBM sees each live line once.  The d loop runs to min(D, W) for every lane (a
// wave spans more than one row of the network's 28-float rows, so some lane needs nearly every d); a lane past its own count re-reads its
// last live plane (a clamped index: same address as the iteration before) and KEEPS its accumulator through a select — no branch, so
// the compiler batches the loads of four iterations.  All accesses are single dwords: a 4-byte-aligned pointer runs the same code.
#include "s3r_kernels.h"

namespace s3r {

template <bool DO_L, bool DO_R>
__global__ __launch_bounds__(256) void cost_volume_bwd_kernel(const float* __restrict__ gv, float* __restrict__ gl,
                                                              float* __restrict__ gr, int C, int D, int W, int HW, int Dn, int total,
                                                              FastDiv dHW, FastDiv dW, FastDiv dC) {
#pragma clang fp contract(off)
    const unsigned iu = blockIdx.x * 256u + threadIdx.x;
    if (iu >= (unsigned)total) return;
    const int i = (int)iu;
    const int bc = dHW.div(i), e = i - bc * HW;          // (b, c) plane and the position inside it
    const int h = dW.div(e), w = e - h * W;
    const int b = dC.div(bc), c = bc - b * C;
    const size_t slab = (size_t)D * HW;
    const float* __restrict__ L = gv + ((size_t)b * 2 * C + c) * slab + e;      // left slab of (b, c) at the own position, plane 0
    const float* __restrict__ R = L + (size_t)C * slab;                         // right slab
    const int nl = min(Dn, w + 1), nr = min(Dn, W - w);                         // >= 1 both
    float al = 0.f, ar = 0.f;
    {
        const float l0 = L[0], r0 = R[0];                                       // plane 0 is live everywhere in both slabs
        if (DO_L) al = l0 - r0;
        if (DO_R) ar = r0 - l0;
    }
#pragma unroll 4
    for (int d = 1; d < Dn; ++d) {
        if (DO_L) {
            const int k = min(d, nl - 1);                                       // past the own count: the last live plane again
            const float t = L[k * HW] - R[k * HW - k];
            al = d < nl ? al + t : al;                                          // a select: what is not summed cannot reach the sum
        }
        if (DO_R) {
            const int k = min(d, nr - 1);
            const float t = R[k * HW] - L[k * HW + k];
            ar = d < nr ? ar + t : ar;
        }
    }
    if (DO_L) gl[i] = al;
    if (DO_R) gr[i] = ar;
}

hipError_t launch_cost_volume_backward(const float* gv, float* gl, float* gr, int B, int C, int D, int H, int W, hipStream_t s) {
    const int HW = H * W;
    const int total = B * C * HW;                        // < 2^31: the caller checked the (larger) volume
    const int Dn = D < W ? D : W;                        // planes d >= W are structural zeros throughout
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const FastDiv dHW((unsigned)HW), dW((unsigned)W), dC((unsigned)C);
    if (gl && gr)
        hipLaunchKernelGGL((cost_volume_bwd_kernel<true, true>), grid, block, 0, s, gv, gl, gr, C, D, W, HW, Dn, total, dHW, dW, dC);
    else if (gl)
        hipLaunchKernelGGL((cost_volume_bwd_kernel<true, false>), grid, block, 0, s, gv, gl, gr, C, D, W, HW, Dn, total, dHW, dW, dC);
    else
        hipLaunchKernelGGL((cost_volume_bwd_kernel<false, true>), grid, block, 0, s, gv, gl, gr, C, D, W, HW, Dn, total, dHW, dW, dC);
    return hipGetLastError();
}

}  // namespace s3r
