// The operand passes of the one-axis Winograd forms (map and F(4,3) derivation: s3r_wino.h): the F(4,3) input and weight
// transforms of a convolution, and the difference tensors and weight sums of a transposed convolution's F(2,2) classes.  The
// class GEMM that reads them is s3r_wino_gemm.hip.
#include "s3r_wino.h"

namespace s3r {

// ---- input transform: one thread per (plane row of V, column); rows 0 .. R+1 of the group in the padded input plane
template <int R>
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, float* __restrict__ V, long long planes,
                                                         int Hp, int Wp, int Hq, long long cls_stride) {
    const long long total = planes * Hq * Wp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long row = i / Wp;                     // (plane, q)
        const int w = (int)(i - row * Wp);
        const long long pl = row / Hq;
        const int q = (int)(row - pl * Hq);
        const float* __restrict__ src = x + (pl * Hp + R * q) * Wp + w;
        float r[R + 2], v[R + 2];
#pragma unroll
        for (int k = 0; k < R + 2; ++k) r[k] = (R * q + k < Hp) ? src[(long long)k * Wp] : 0.f;   // (rows below the halo are zero)
        wino_rows_to_classes<R>(r, v);
#pragma unroll
        for (int k = 0; k < R + 2; ++k) V[i + k * cls_stride] = v[k];
    }
}

hipError_t launch_wino_input(const float* x, float* V, long long planes, int Hp, int Wp, int Hq, int R, hipStream_t s) {
    const long long total = planes * Hq * Wp;
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
    if (R != 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wino_input_kernel<4>, grid, dim3(256), 0, s, x, V, planes, Hp, Wp, Hq, total);
    return hipGetLastError();
}

// ---- weights: w[Cout][Cin][kd][3][kw] (torch layout, 2D: kd = 1) -> R + 2 class slabs in the conv kernel's packed K order
__global__ void pack_wino_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int CoutPad, int kd,
                                 int kw, int R) {
    const int T = kd * kw;
    const size_t per_cls = (size_t)T * Cin * CoutPad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)(R + 2) * per_cls; i += (size_t)gridDim.x * blockDim.x) {
        const int cls = (int)(i / per_cls);
        size_t r = i % per_cls;
        const int co = (int)(r % CoutPad);
        r /= CoutPad;
        const int c = (int)(r % WBK);
        r /= WBK;
        const int tap = (int)(r % T);
        const int cc = (int)(r / T);
        const int cin = cc * WBK + c;
        float v = 0.f;
        if (co < Cout) {
            const int td = tap / kw, tw = tap - td * kw;
            const float* g = w + (((size_t)co * Cin + cin) * kd + td) * 3 * kw + tw;       // g[kh * kw]
            const float g0 = g[0], g1 = g[kw], g2 = g[2 * kw];
            const float s02 = g0 + g2, a = g0 * (1.f / 24.f) + g2 * (1.f / 6.f), b12 = g1 * (1.f / 12.f);
            v = cls == 0 ? g0 * 0.25f : cls == 1 ? (s02 + g1) * (-1.f / 6.f) : cls == 2 ? (s02 - g1) * (-1.f / 6.f)
              : cls == 3 ? a + b12 : cls == 4 ? a - b12 : g2;
        }
        wp[i] = v;
    }
}

hipError_t launch_pack_wino(const float* w, float* wp, int Cin, int Cout, int CoutPad, int kd, int kw, int R, hipStream_t s) {
    hipLaunchKernelGGL(pack_wino_kernel, dim3(1024), dim3(256), 0, s, w, wp, Cin, Cout, CoutPad, kd, kw, R);
    return hipGetLastError();
}

// ================================================================================================
// ConvTranspose3d(k = 4, s = 2, p = 1) with fewer multiplications: Winograd F(2, 2) along D AND H inside every output-parity
// class.  A class (rd, rh, rw) is a 2 x 2 x 2-tap convolution over the input grid (s3r_conv_glds.hip).  Along one axis, two of its
// outputs that are neighbours — input positions 2q and 2q + 1 — read the padded input rows x0, x1, x2 = R, R + 1, R + 2 (R = 2q + r)
// through the axis' two taps g0, g1:
//     y(2q)     = x0 g0 + x1 g1 = m0 + m1        m0 = (x0 - x1) g0
//     y(2q + 1) = x1 g0 + x2 g1 = m1 - m2        m1 = x1 (g0 + g1)        m2 = (x1 - x2) g1
// — three products instead of four.  r03 did this along H (3/4 of the matrix work); nested along D and H it is NINE products
// M_ab (a, b in 0..2: the D and the H class) for 2 x 2 outputs instead of sixteen: 9/16 of the direct form's multiplications,
// each product a 2-tap (column) convolution over Cin.  Class (a, b) reads {a = 1: plain, else depth differences} x {b = 1: plain,
// else row differences} of the padded input at depth Z + (a ? 1 : 0), row R + (b ? 1 : 0):
//     Dh[z][r] = x[z][r] - x[z][r + 1],   Dd[z][r] = x[z][r] - x[z + 1][r],   Ddh[z][r] = Dh[z][r] - Dh[z + 1][r].
// The row differences Dh are always a tensor of their own (wino_diff_kernel: the input of a transposed convolution is small).  The
// DEPTH differences come in two forms with the same bits: MATERIALISED (p.xd_mode = 1: the same kernel writes Dd and Ddh too, the
// class kernel reads one tile per K step) where the four tensors stay in the Infinity Cache (d1, d2 at B = 32), or formed IN the
// kernel (p.xd_mode = 0: a depth-difference class stages the tiles of depths z and z + 1 side by side in LDS and subtracts the two
// fragments in front of the MFMA, one v_sub per matrix instruction) where writing and re-reading two more tensors would cross HBM
// (d3 at B = 32: 0.72 -> 0.69 ms; the 1.67 x operand traffic costs d1 / d2, which are L2-delivery bound, 27 / 4 %).  The transformed weights are the sums of the 2 x 2 (depth tap, row tap) weights over {a: td = 0 | both | 1} x
// {b: th = 0 | both | 1}, per (parity class, column tap).  Positions are (b, s, q, pw) = (sample, depth pair, row pair, column) over
// the input grid; the output transform Y[u][v] = sum A[u][a] A[v][b] M_ab, A = [[1, 1, 0], [0, 1, -1]], runs on the accumulator
// registers; HEAD = the fused 1 x 1 x 1 head (d3 -> d4).
// D = [Dh | Dd | Ddh] (THREE) or [Dh].  One thread per element; the index arithmetic is 32-bit mulhi division by launch
// invariants (the first version's 64-bit % and / per element ran at 2.7 TB/s).
template <bool THREE>
__global__ __launch_bounds__(256) void wino_diff_kernel(const float* __restrict__ x, float* __restrict__ D, unsigned total,
                                                        int Dp, int Hp, int Wp, FastDiv dPer, FastDiv dHW, FastDiv dW) {
    const unsigned hw = (unsigned)Hp * Wp, per = (unsigned)Dp * hw;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned pl = (unsigned)dPer.div((int)i);
        const unsigned e = i - pl * per;
        const unsigned z = (unsigned)dHW.div((int)e);
        const unsigned r = (unsigned)dW.div((int)(e - z * hw));
        const bool rn = r + 1 < (unsigned)Hp, zn = z + 1 < (unsigned)Dp;
        const float x00 = x[i];
        const float x01 = rn ? x[i + Wp] : 0.f;
        const float dh0 = rn ? x00 - x01 : 0.f;
        D[i] = dh0;
        if constexpr (THREE) {
            const float x10 = zn ? x[i + hw] : 0.f;
            const float x11 = (rn && zn) ? x[i + hw + Wp] : 0.f;
            const float dh1 = rn ? x10 - x11 : 0.f;          // Dh at depth z + 1
            D[i + (size_t)total] = zn ? x00 - x10 : 0.f;
            D[i + 2 * (size_t)total] = zn ? dh0 - dh1 : 0.f;
        }
    }
}

// the same two columns per thread (rows are an even number of floats — edge + 2 — and 8-byte aligned: half the memory instructions)
template <bool THREE>
__global__ __launch_bounds__(256) void wino_diff2_kernel(const float* __restrict__ x, float* __restrict__ D, unsigned total,
                                                         int Dp, int Hp, int Wp, FastDiv dPer, FastDiv dHW, FastDiv dW) {
    const unsigned hw = (unsigned)Hp * Wp, per = (unsigned)Dp * hw;
    for (unsigned i = (blockIdx.x * 256u + threadIdx.x) * 2u; i < total; i += gridDim.x * 512u) {
        const unsigned pl = (unsigned)dPer.div((int)i);
        const unsigned e = i - pl * per;
        const unsigned z = (unsigned)dHW.div((int)e);
        const unsigned r = (unsigned)dW.div((int)(e - z * hw));
        const bool rn = r + 1 < (unsigned)Hp, zn = z + 1 < (unsigned)Dp;
        const wv2f zero = {0.f, 0.f};
        const wv2f x00 = *reinterpret_cast<const wv2f*>(x + i);
        const wv2f x01 = rn ? *reinterpret_cast<const wv2f*>(x + i + Wp) : zero;
        const wv2f dh0 = rn ? x00 - x01 : zero;
        *reinterpret_cast<wv2f*>(D + i) = dh0;
        if constexpr (THREE) {
            const wv2f x10 = zn ? *reinterpret_cast<const wv2f*>(x + i + hw) : zero;
            const wv2f x11 = (rn && zn) ? *reinterpret_cast<const wv2f*>(x + i + hw + Wp) : zero;
            const wv2f dh1 = rn ? x10 - x11 : zero;          // Dh at depth z + 1
            *reinterpret_cast<wv2f*>(D + i + (size_t)total) = zn ? x00 - x10 : zero;
            *reinterpret_cast<wv2f*>(D + i + 2 * (size_t)total) = zn ? dh0 - dh1 : zero;
        }
    }
}

hipError_t launch_wino_diff(const float* x, float* D, long long planes, int Dp, int Hp, int Wp, int three, hipStream_t s) {
    const long long total = planes * Dp * Hp * Wp;
    if (total >= (1ll << 31)) return hipErrorInvalidValue;
    if ((Wp & 1) == 0 && ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(D)) & 7) == 0 && (total & 1) == 0) {
        const long long blocks2 = (total / 2 + 255) / 256;
        const dim3 grid2((unsigned)(blocks2 < 16384 ? blocks2 : 16384));
        const FastDiv dPer((unsigned)(Dp * Hp * Wp)), dHW((unsigned)(Hp * Wp)), dW((unsigned)Wp);
        if (three) hipLaunchKernelGGL(wino_diff2_kernel<true>, grid2, dim3(256), 0, s, x, D, (unsigned)total, Dp, Hp, Wp, dPer, dHW, dW);
        else hipLaunchKernelGGL(wino_diff2_kernel<false>, grid2, dim3(256), 0, s, x, D, (unsigned)total, Dp, Hp, Wp, dPer, dHW, dW);
        return hipGetLastError();
    }
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    const FastDiv dPer((unsigned)(Dp * Hp * Wp)), dHW((unsigned)(Hp * Wp)), dW((unsigned)Wp);
    if (three) hipLaunchKernelGGL(wino_diff_kernel<true>, grid, dim3(256), 0, s, x, D, (unsigned)total, Dp, Hp, Wp, dPer, dHW, dW);
    else hipLaunchKernelGGL(wino_diff_kernel<false>, grid, dim3(256), 0, s, x, D, (unsigned)total, Dp, Hp, Wp, dPer, dHW, dW);
    return hipGetLastError();
}

// w[Cin][Cout][4][4][4] -> Up[pc = 8][cls = 9][(chunk*2 + tw)*32 + c][CoutPad]
__global__ void pack_wino_deconv_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int CoutPad) {
    const size_t per_f = (size_t)2 * Cin * CoutPad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 72 * per_f; i += (size_t)gridDim.x * blockDim.x) {
        const int pf = (int)(i / per_f);
        const int pc = pf / 9, f = pf - pc * 9;
        const int fa = f / 3, fb = f - fa * 3;
        size_t r = i % per_f;
        const int co = (int)(r % CoutPad);
        r /= CoutPad;
        const int c = (int)(r % WBK);
        r /= WBK;
        const int tw = (int)(r & 1);
        const int cc = (int)(r >> 1);
        const int cin = cc * WBK + c;
        float v = 0.f;
        if (co < Cout) {
            const int rd = (pc >> 2) & 1, rh = (pc >> 1) & 1, rw = pc & 1;
            const int kw = 3 - rw - 2 * tw;
            const float* g = w + ((size_t)cin * Cout + co) * 64 + kw;
            // taps t = 0, 1 along an axis of parity r: kernel index 3 - r, 1 - r
            auto hsum = [&](int td) {
                const float* gd = g + (3 - rd - 2 * td) * 16;
                const float g0 = gd[(3 - rh) * 4], g1 = gd[(1 - rh) * 4];
                return fb == 0 ? g0 : fb == 2 ? g1 : g0 + g1;
            };
            v = fa == 0 ? hsum(0) : fa == 2 ? hsum(1) : hsum(0) + hsum(1);
        }
        wp[i] = v;
    }
}

hipError_t launch_pack_wino_deconv(const float* w, float* wp, int Cin, int Cout, int CoutPad, hipStream_t s) {
    hipLaunchKernelGGL(pack_wino_deconv_kernel, dim3(1024), dim3(256), 0, s, w, wp, Cin, Cout, CoutPad);
    return hipGetLastError();
}

}  // namespace s3r
