// fp32 stride-1 convolutions and ConvTranspose3d(k4 s2 p1) with FEWER multiplications: the Winograd forms.  One class GEMM
// (wino_body) serves all of them; what differs is how many classes a layer has, what is left of its kernel inside a class, and
// who applies the output transform.  This header holds what more than one of their translation units needs — the tile constants,
// the LDS-DMA wrapper and the transforms that a class kernel and its finish / hand-off passes must share to agree bit for bit:
//   s3r_wino_axis1.hip    1. one axis, F(4,3) along H (six classes, half the multiplications): input and weight transform (e2, e4)
//                         2. transposed convolutions, F(2,2) along D and H inside each output-parity class (nine classes, 9/16):
//                            the difference tensors and the weight transform                                          (d1, d2, d3)
//   s3r_wino_gemm.hip     wino_body and its launch forms: serial / class-parallel / dual (one axis), semi-fused (two axes);
//                         wino_finish_kernel, wino_plan; every wino_kernel<..> instantiation lives in this one code object
//   s3r_wino_axis2.hip    two axes, class-parallel or semi-fused: F(4,3) x F(4,3) over D, H (Conv3d k3: v1, v3, v5) or over H, W
//                         (Conv2d k3: e6, e7), F(2,4) x F(2,4) (Conv3d k4 valid: v6); their input transforms, weight transforms
//                         and finish kernels, launch_conv_wino2
//   s3r_wino_handoff.hip  the 3D hand-off pass: a producer's finish and its consumer's operand transform in one kernel
//
// One axis, F(4, 3) (Lavin & Gray): four output rows (4q .. 4q + 3) of a column need the padded input rows r0..r5 = 4q .. 4q + 5
// and the three kernel rows g0, g1, g2:
//     v0 = 4 r0 - 5 r2 + r4             u0 = g0 / 4                          y0 = m0 + m1 + m2 + m3 + m4
//     v1 = -4 r1 - 4 r2 + r3 + r4       u1 = -(g0 + g1 + g2) / 6             y1 = m1 - m2 + 2 m3 - 2 m4
//     v2 = 4 r1 - 4 r2 - r3 + r4        u2 = -(g0 - g1 + g2) / 6             y2 = m1 + m2 + 4 m3 + 4 m4
//     v3 = -2 r1 - r2 + 2 r3 + r4       u3 = g0 / 24 + g1 / 12 + g2 / 6      y3 = m1 - m2 + 8 m3 - 8 m4 + m5
//     v4 = 2 r1 - r2 - 2 r3 + r4        u4 = g0 / 24 - g1 / 12 + g2 / 6
//     v5 = 4 r1 - 5 r3 + r5             u5 = g2                              m_i = sum over (cin, kd, kw) of u_i * v_i
// so the layer becomes SIX convolutions with a (kd x 1 x kw) kernel — 9 taps instead of 27 in 3D, 3 instead of 9 in 2D, each over
// its own transformed input plane set V_i and its own transformed weights U_i — whose results are combined in registers: HALF
// the matrix work of the direct form for the same outputs (edges that are not a multiple of 4 compute a partial last group:
// 16 rows for 14, 8 for 7).  Along H alone K stays Cin x 9 (or x 3), the W axis stays contiguous (16-byte gathers where
// W % 4 == 0, whole-row stores), six classes' accumulators fit a workgroup's registers, and the kernel is the implicit GEMM of
// s3r_conv_glds.hip with a class loop around its K loop.  Every further axis multiplies the classes (36 for two) and shortens
// each class's K: a workgroup cannot hold them, so the two-axis forms (s3r_wino_axis2.hip) send class sums through slabs in HBM — which
// pays where the output is small (an edge <= 28) and not for e2 / e4.  In fp32 over 64-256 channels the forms are as accurate as
// the direct sum (rel-L2 against an fp64 convolution: direct 3e-7 .. 1e-6, one axis <= 2.3e-6, two axes <= 4.7e-6; north_star
// allows 1e-4) but they are DIFFERENT summations: results are not bit-identical to the direct kernels' nor to each other's,
// which is why the choice between them is part of the layer descriptor (s3r_algo, include/s3r.h).
//
//   wino_input_kernel   x (padded NC(D)HW, halo 1) -> V[6][B][C][Dp][ceil(H/4)][Wp]   (HBM-bound: reads x once, writes 1.5 x)
//   pack_wino_kernel    w[Cout][Cin][kd][3][kw]    -> Up[6][(chunk*T' + tap')*32 + c][CoutPad],  T' = kd*kw, 32-channel chunks
//   wino_kernel / wino_dual_kernel / wino_finish_kernel: the class kernels, s3r_wino_gemm.hip
#pragma once
#include "s3r_kernels.h"

namespace s3r {

typedef float wf32x16 __attribute__((ext_vector_type(16)));
typedef float wv2f __attribute__((ext_vector_type(2)));
template <int N> struct WVec;
template <> struct WVec<1> { typedef float type; };
template <> struct WVec<2> { typedef wv2f type; };
typedef float wv4f __attribute__((ext_vector_type(4)));
template <> struct WVec<4> { typedef wv4f type; };
template <int N>
__device__ __forceinline__ float wvget(const typename WVec<N>::type& v, int i) {
    if constexpr (N == 1) return v; else return v[i];
}

#define S3R_LDS_PTR_W(p) ((__attribute__((address_space(3))) void*)(p))

#ifndef S3R_WNB
#define S3R_WNB 2      // LDS stages.  With 16-channel K tiles: 2 stages -0.3 %, 3 = 4.  32-channel tiles halve the barriers per MFMA
#endif                  // (32 MFMAs per wave between two, like the direct path's 64 x 256 tile) and, at two stages (48 KiB, three
                        // workgroups per CU), are 1.3 % of the step faster than 16 x 3: v1 0.807 -> 0.769 ms, d3 0.824 -> 0.803
#ifndef S3R_WBK
#define S3R_WBK 32
#endif
constexpr int WBM = 64, WBK = S3R_WBK, WNB = S3R_WNB;      // K tile: one tap x WBK channels
constexpr int WNPA = WBK * WBM / 1024;                                // 1 KiB weight pieces per wave and K tile
constexpr int WCN = 64;                                  // positions per tile of the serial / class-parallel forms (head: WBN)

template <int BYTES>
__device__ __forceinline__ void wdma(__amdgpu_buffer_rsrc_t rsrc, float* lds_dst, int voffset, int soffset) {
    static_assert(BYTES == 16 || BYTES == 4, "LDS-DMA width");
    if constexpr (BYTES == 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, S3R_LDS_PTR_W(lds_dst), 16, voffset, soffset, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, S3R_LDS_PTR_W(lds_dst), 4, voffset, soffset, 0, 0);
}

// KIND 1: convolution, F(4,3) along H; KIND 2: ConvTranspose3d(k4 s2 p1), F(2,2) along D and H (the class kernels, s3r_wino_gemm.hip)
template <int KIND> struct WinoKind;
template <> struct WinoKind<1> { static constexpr int NCLS = 6, R = 4; };
template <> struct WinoKind<2> { static constexpr int NCLS = 9, R = 4; };     // R: outputs per position (2 depths x 2 rows)

// output transform of one (cout, position): m = the class sums, y = the R output rows.  Adds and explicit fmaf only (nothing
// the compiler could contract differently in the two kernels that share it).
template <int KIND>
__device__ __forceinline__ void wino_out(const float (&m)[WinoKind<KIND>::NCLS], float (&y)[WinoKind<KIND>::R]) {
    if constexpr (KIND == 1) {
        const float s12 = m[1] + m[2], d12 = m[1] - m[2];
        const float s34 = m[3] + m[4], d34 = m[3] - m[4];
        y[0] = (m[0] + s12) + s34;
        y[1] = fmaf(2.f, d34, d12);
        y[2] = fmaf(4.f, s34, s12);
        y[3] = fmaf(8.f, d34, d12) + m[5];
    } else {             // m[3 a + b]; rows first, then depths: y[2 u + v]
        const float t00 = m[0] + m[1], t01 = m[1] - m[2];
        const float t10 = m[3] + m[4], t11 = m[4] - m[5];
        const float t20 = m[6] + m[7], t21 = m[7] - m[8];
        y[0] = t00 + t10;
        y[1] = t01 + t11;
        y[2] = t10 - t20;
        y[3] = t11 - t21;
    }
}
// element offset of output i of a position from its first output (conv: rows 4q + i; transposed: depth pair u = i >> 1, row pair
// v = i & 1, two output planes / rows apart)
template <int KIND>
__device__ __forceinline__ int wino_out_off(int i, int y_ds, int y_hs) {
    if constexpr (KIND == 1) return i * y_hs;
    else return (i >> 1) * 2 * y_ds + (i & 1) * 2 * y_hs;
}
__device__ __forceinline__ float wino_act(float y, float sc, float sf, float lo) { return fmaxf(fmaf(y, sc, sf), lo); }
__device__ __forceinline__ float wino_head_act(float t, int act) {
    if (act == ACT_RELU) return fmaxf(t, 0.f);
    if (act == ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.f + __expf(-t));
    return t;
}

// One axis of a two-axis form (s3r_wino_axis2.hip): F(4,3) as above, or F(2,4), points 0, 1, -1, 2, inf (tools/wino_matrices.py
// derives and checks both sets in exact arithmetic):
//     B^T rows (2,-1,-2,1,0) (0,-2,-1,1,0) (0,2,-3,1,0) (0,-1,0,1,0) (0,2,-1,-2,1)
//     G rows (1/2,0,0,0) (-1/2,-1/2,-1/2,-1/2) (-1/6,1/6,-1/6,1/6) (1/6,1/3,2/3,4/3) (0,0,0,1)     A^T rows (1,1,1,1,0) (0,1,-1,2,1)
template <int AX> struct WAxis;
template <> struct WAxis<0> { static constexpr int N = 6, M = 4, R = 3; };      // F(4,3)
template <> struct WAxis<1> { static constexpr int N = 5, M = 2, R = 4; };      // F(2,4)

template <int AX>
__device__ __forceinline__ void wax_bt(const float (&r)[WAxis<AX>::N], float (&v)[WAxis<AX>::N]) {
    if constexpr (AX == 0) wino_rows_to_classes<4>(r, v);
    else {
        v[0] = fmaf(2.f, r[0] - r[2], r[3] - r[1]);
        v[1] = fmaf(-2.f, r[1], r[3] - r[2]);
        v[2] = fmaf(2.f, r[1], fmaf(-3.f, r[2], r[3]));
        v[3] = r[3] - r[1];
        v[4] = fmaf(2.f, r[1] - r[3], r[4] - r[2]);
    }
}
template <int AX>
__device__ __forceinline__ void wax_at(const float (&m)[WAxis<AX>::N], float (&y)[WAxis<AX>::M]) {
    if constexpr (AX == 0) wino_out<1>(m, y);
    else {
        y[0] = ((m[0] + m[1]) + m[2]) + m[3];
        y[1] = fmaf(2.f, m[3], m[1] - m[2]) + m[4];
    }
}
// transformed weight of class c from the axis' R kernel values
template <int AX>
__device__ __forceinline__ float wax_g(int c, const float (&g)[WAxis<AX>::R]) {
    if constexpr (AX == 0) {
        const float s02 = g[0] + g[2], a = g[0] * (1.f / 24.f) + g[2] * (1.f / 6.f), b12 = g[1] * (1.f / 12.f);
        return c == 0 ? g[0] * 0.25f : c == 1 ? (s02 + g[1]) * (-1.f / 6.f) : c == 2 ? (s02 - g[1]) * (-1.f / 6.f)
             : c == 3 ? a + b12 : c == 4 ? a - b12 : g[2];
    } else {
        const float e = g[0] + g[2], o = g[1] + g[3];
        return c == 0 ? g[0] * 0.5f : c == 1 ? (e + o) * -0.5f : c == 2 ? (o - e) * (1.f / 6.f)
             : c == 3 ? fmaf(g[3], 4.f / 3.f, fmaf(g[2], 2.f / 3.f, fmaf(g[1], 1.f / 3.f, g[0] * (1.f / 6.f)))) : g[3];
    }
}

// a group g of one (sample, depth group) of a 3D two-axis layer -> its row group and column: (row group, column), or — the cost
// volume's consumer, p.cv_n — (column, row group)
__device__ __forceinline__ void wino2_group_pos(const ConvParams& p, int g, int& sh, int& pw) {
    if (p.cv_n) { pw = p.dNh.div(g); sh = g - pw * p.Nh; }
    else { sh = p.dW.div(g); pw = g - sh * p.Nw; }
}

#ifdef S3R_ABLATE   // diagnostic builds: S3R_ABL=3 no operand DMA inside the K loop, 4 weights only, 5 activations only, 6 activations on a chunk's first column tap only
int wabl_mode();        // (s3r_wino_gemm.hip: S3R_ABL, read once)
#define S3R_WABL(p) (p).debug = wabl_mode()
#else
#define S3R_WABL(p) (void)0
#endif

// The class GEMM of a two-axis layer (s3r_wino_gemm.hip): q = launch_conv_wino2's view of the class convolution, one workgroup per
// (tile, class) or — semi — per (tile, depth class); cvl: leave out the cost volume's dead K tiles.  16-byte gathers where q.Nw % 4 == 0
hipError_t launch_wino2_classes(const ConvParams& q, bool semi, bool cvl, hipStream_t stream);

}  // namespace s3r
