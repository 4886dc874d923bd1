// The two-axis Winograd forms (map and transforms: s3r_wino.h): input transforms, weight transforms, finish kernels and
// launch_conv_wino2; the class GEMM between them is s3r_wino_gemm.hip's, through launch_wino2_classes.
//
// Two-axis Winograd for the small 3D layers, CLASS-PARALLEL ONLY.  A class-parallel workgroup holds ONE class's accumulators,
// so nothing limits the number of classes: nesting the transform along D and H turns v5 (3 x 3 x 3 over 7^3) into 36 class
// convolutions with a 1 x 1 x 3 kernel for 4 x 4 outputs — F(4,3) x F(4,3): 108 multiply-adds per 16 outputs where the direct
// form spends 432 and the one-axis form 216 — and v6 (4 x 4 x 4, valid, 7^3 -> 4^3) into 25 classes with a 1 x 1 x 4 kernel for
// 2 x 2 outputs: F(2,4) x F(2,4), 100 per 4 outputs instead of 256.  The class GEMM is the one-axis kernel's class-parallel form
// unchanged (wino_kernel<VEC, 1, 2, true>: a class is a plane set + a weight slab, K = Cin x kw); what is new is the input
// transform (a window of n x n rows per group), the weight transform (G x G) and the finish kernel (A^T along H, then D).
// Slabs cost ncls / (m m) x the output's bytes, which is why only layers with small outputs take it (v5: 11 MB -> 32 MB).
// The F(2,4) matrices stand with wax_bt / wax_at / wax_g in s3r_wino.h.
#include "s3r_wino.h"
#include <cstdlib>

namespace s3r {

int wino2_classes(int ax) { return ax == 1 ? 25 : 36; }      // ax 2: the 2D layers' (H, W) nesting, F(4,3) x F(4,3) again
int wino2_outputs(int ax) { return ax == 1 ? 2 : 4; }

// one thread per (plane, depth group, row group, column): an N x N window of the input, B^T along H then along D
template <int AX>
__global__ __launch_bounds__(256) void wino2_input_kernel(const float* __restrict__ x, float* __restrict__ V, unsigned total,
                                                          int Dp, int Hp, int Wp, int SD, int SH, FastDiv dW, FastDiv dSH, FastDiv dSD) {
    constexpr int N = WAxis<AX>::N, M = WAxis<AX>::M;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned row = (unsigned)dW.div((int)i);                   // ((plane, sd), sh)
        const int w = (int)(i - row * (unsigned)Wp);
        const unsigned pg = (unsigned)dSH.div((int)row);                 // (plane, sd)
        const int sh = (int)(row - pg * (unsigned)SH);
        const unsigned pl = (unsigned)dSD.div((int)pg);
        const int sd = (int)(pg - pl * (unsigned)SD);
        const float* __restrict__ src = x + ((size_t)pl * Dp + M * sd) * Hp * Wp + (size_t)M * sh * Wp + w;
        float t[N][N];                                                   // [depth][row class]
#pragma unroll
        for (int a = 0; a < N; ++a) {
            float r[N], v[N];
#pragma unroll
            for (int b = 0; b < N; ++b)
                r[b] = (M * sd + a < Dp && M * sh + b < Hp) ? src[((size_t)a * Hp + b) * Wp] : 0.f;
            wax_bt<AX>(r, v);
#pragma unroll
            for (int b = 0; b < N; ++b) t[a][b] = v[b];
        }
#pragma unroll
        for (int b = 0; b < N; ++b) {
            float r[N], v[N];
#pragma unroll
            for (int a = 0; a < N; ++a) r[a] = t[a][b];
            wax_bt<AX>(r, v);
#pragma unroll
            for (int a = 0; a < N; ++a) V[(size_t)(a * N + b) * total + i] = v[a];
        }
    }
}

hipError_t launch_wino2_input(const float* x, float* V, int ax, long long planes, int Dp, int Hp, int Wp, int SD, int SH, hipStream_t s) {
    const long long total = planes * SD * SH * Wp;
    if (total >= (1ll << 31) || (ax != 0 && ax != 1)) return hipErrorInvalidValue;
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    const FastDiv dW((unsigned)Wp), dSH((unsigned)SH), dSD((unsigned)SD);
    if (ax == 0) hipLaunchKernelGGL(wino2_input_kernel<0>, grid, dim3(256), 0, s, x, V, (unsigned)total, Dp, Hp, Wp, SD, SH, dW, dSH, dSD);
    else hipLaunchKernelGGL(wino2_input_kernel<1>, grid, dim3(256), 0, s, x, V, (unsigned)total, Dp, Hp, Wp, SD, SH, dW, dSH, dSD);
    return hipGetLastError();
}

// w[Cout][Cin][k][k][k] (k = R) -> Up[cls = a N + b][(chunk*k + tw)*32 + c][CoutPad]: G along H, then along D
template <int AX>
__global__ void pack_wino2_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int CoutPad) {
    constexpr int N = WAxis<AX>::N, R = WAxis<AX>::R;
    const size_t per_cls = (size_t)R * Cin * CoutPad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)N * N * per_cls; i += (size_t)gridDim.x * blockDim.x) {
        const int cls = (int)(i / per_cls);
        const int ca = cls / N, cb = cls - ca * N;
        size_t r = i % per_cls;
        const int co = (int)(r % CoutPad);
        r /= CoutPad;
        const int c = (int)(r % WBK);
        r /= WBK;
        const int tw = (int)(r % R);
        const int cc = (int)(r / R);
        const int cin = cc * WBK + c;
        float v = 0.f;
        if (co < Cout) {
            const float* g = w + ((size_t)co * Cin + cin) * R * R * R + tw;       // g[(kd * R + kh) * R]
            float gd[R];
#pragma unroll
            for (int kd = 0; kd < R; ++kd) {
                float gh[R];
#pragma unroll
                for (int kh = 0; kh < R; ++kh) gh[kh] = g[(kd * R + kh) * R];
                gd[kd] = wax_g<AX>(cb, gh);
            }
            v = wax_g<AX>(ca, gd);
        }
        wp[i] = v;
    }
}

__global__ void pack_wino2p_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int CoutPad);    // (ax 2, below)
hipError_t launch_pack_wino2(const float* w, float* wp, int ax, int Cin, int Cout, int CoutPad, hipStream_t s) {
    if (ax == 0) hipLaunchKernelGGL(pack_wino2_kernel<0>, dim3(1024), dim3(256), 0, s, w, wp, Cin, Cout, CoutPad);
    else if (ax == 1) hipLaunchKernelGGL(pack_wino2_kernel<1>, dim3(1024), dim3(256), 0, s, w, wp, Cin, Cout, CoutPad);
    else if (ax == 2) hipLaunchKernelGGL(pack_wino2p_kernel, dim3(1024), dim3(256), 0, s, w, wp, Cin, Cout, CoutPad);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Finish kernels.  The output tensors carry their consumer's halo, so rows are (W + 2 halo) floats long: a kernel that stores
// interiors only leaves EVERY 128-byte line partly written, and partial lines cost the memory side a read-modify-write (measured on
// v1's finish: its stores alone ran at 2.5 TB/s, its loads at 6).  So a workgroup builds whole padded slices in LDS — halo zeros
// included — and writes them out as contiguous 16-byte stores: the halo is rewritten with the zeros it already holds.
__device__ __forceinline__ void wino2_copy_out(const float* __restrict__ lds, float* __restrict__ dst, int count, int tid) {
    if ((count & 3) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
        for (int i = tid * 4; i < count; i += 1024) *reinterpret_cast<wv4f*>(dst + i) = *reinterpret_cast<const wv4f*>(lds + i);
    } else {
        for (int i = tid; i < count; i += 256) dst[i] = lds[i];
    }
}
__device__ __forceinline__ void wino2_zero_out(float* __restrict__ dst, int count, int tid) {
    if ((count & 3) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
        for (int i = tid * 4; i < count; i += 1024) *reinterpret_cast<wv4f*>(dst + i) = wv4f{0.f, 0.f, 0.f, 0.f};
    } else {
        for (int i = tid; i < count; i += 256) dst[i] = 0.f;
    }
}


// 3D, semi-fused form: one workgroup per (cout, SUB consecutive (sample, depth group) pairs — as many as give its 256 threads a
// group each): slabs [a][row][Cout][npad] (the row transform already applied by the class kernel) -> 4 output slices per pair:
// A^T along D, folded BN + activation.  y: halo-padded, y_hs = W + 2 halo, y_ds = a slice
__global__ __launch_bounds__(256) void wino2s_finish_kernel(const ConvParams p, const int npad, const int halo, const int SUB,
                                                            const FastDiv dNd, const FastDiv dMS) {
    constexpr int N = 6, M = 4;
    extern __shared__ __attribute__((aligned(16))) float fsm[];          // SUB x M slices of Hp x Wp
    const int tid = threadIdx.x;
    const int G = p.Nh * p.Nw, Wp = p.y_hs, slice = p.y_ds, MS = M * slice;
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    const int per_c = p.B * p.Nd;
    const int nrg = (per_c + SUB - 1) / SUB;
    const bool vec = (slice & 3) == 0 && (reinterpret_cast<size_t>(p.y) & 15) == 0;
    for (int item = blockIdx.x; item < p.Cout * nrg; item += gridDim.x) {
        const int mrow = item / nrg;
        const int r0 = (item - mrow * nrg) * SUB;                        // first (sample, depth group) pair
        const int nsub = per_c - r0 < SUB ? per_c - r0 : SUB;
        for (int i = tid; i < nsub * MS; i += 256) fsm[i] = 0.f;
        __syncthreads();
        const float sc = p.scale ? p.scale[mrow] : 1.f, sf = p.shift ? p.shift[mrow] : 0.f;
        for (int t = tid; t < nsub * G; t += 256) {
            const int sub = p.dHW.div(t);
            const int g = t - sub * G;
            int sh, pw;
            wino2_group_pos(p, g, sh, pw);
            const int r = r0 + sub;
            const int sd = r - dNd.div(r) * p.Nd;
            const int n = r0 * G + t;                                  // (slabs blocked by (cout, 64-position tile): wino_body, SEMI)
            const float* __restrict__ src = p.part + ((size_t)mrow * (npad >> 6) + (n >> 6)) * (N * M * 64) + (n & 63);
            float* __restrict__ o = fsm + sub * MS + (halo + M * sh) * Wp + halo + pw;
#pragma unroll
            for (int v = 0; v < M; ++v) {
                float m[N], y[M];
#pragma unroll
                for (int a = 0; a < N; ++a) m[a] = src[(a * M + v) * 64];
                wax_at<0>(m, y);
#pragma unroll
                for (int u = 0; u < M; ++u)
                    if (M * sd + u < p.Dout && M * sh + v < p.Hout) o[u * slice + v * Wp] = wino_act(y[u], sc, sf, lo);
            }
        }
        __syncthreads();
        float* __restrict__ yc = p.y + (size_t)mrow * p.y_cs;
        // every pair's slices are one contiguous run of the output (the depth halo slices of a sample's first / last pair with them)
        for (int e = vec ? tid * 4 : tid; e < nsub * MS; e += vec ? 1024 : 256) {
            const int sub = dMS.div(e);
            const int off = e - sub * MS;
            const int r = r0 + sub;
            const int b = dNd.div(r);
            const int sd = r - b * p.Nd;
            const int nsl = p.Dout - M * sd < M ? p.Dout - M * sd : M;
            if (off >= nsl * slice) continue;
            float* __restrict__ dst = yc + (size_t)b * p.y_bs + (size_t)(halo + M * sd) * slice + off;
            if (vec) *reinterpret_cast<wv4f*>(dst) = *reinterpret_cast<const wv4f*>(fsm + e);
            else *dst = fsm[e];
        }
        if (halo > 0)
            for (int sub = 0; sub < nsub; ++sub) {
                const int r = r0 + sub;
                const int b = dNd.div(r);
                const int sd = r - b * p.Nd;
                if (sd == 0) wino2_zero_out(yc + (size_t)b * p.y_bs, halo * slice, tid);
                if (sd == p.Nd - 1) wino2_zero_out(yc + (size_t)b * p.y_bs + (size_t)(halo + p.Dout) * slice, halo * slice, tid);
            }
        __syncthreads();
    }
}

// The class-parallel form of the 3D layers keeps the flat finish kernel — one thread per (cout, position), interiors only: its
// outputs are small (v3: 45 MB, v5 / v6: 11 / 4 MB) and the staged kernel's zero / barrier / copy chain costs more than the
// partial lines do (v3 42 -> 44 us, v5 11 -> 18, v6 10 -> 19).
// slabs [cls][Cout][npad] -> y: A^T along H, then along D, folded BN + activation; outputs beyond the true edge are not stored
template <int AX>
__global__ __launch_bounds__(256) void wino2_finish_flat_kernel(const ConvParams p, const int npad) {
    constexpr int N = WAxis<AX>::N, M = WAxis<AX>::M;
    const int S = p.Nd * p.Nh * p.Nw;
    const int nn = p.Ntotal;
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    const long long total = (long long)p.Cout * nn;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int mrow = (int)(i / nn);
        const int n = (int)(i - (long long)mrow * nn);
        const int b = p.dS.div(n);
        int rem = n - b * S;
        const int sd = p.dHW.div(rem);
        rem -= sd * p.Nh * p.Nw;
        int sh, pw;
        wino2_group_pos(p, rem, sh, pw);
        const float* __restrict__ src = p.part + ((size_t)mrow * (npad >> 6) + (n >> 6)) * (N * N * 64) + (n & 63);     // (blocked slabs)
        float t[N][M];                                                   // [depth class][output row]
#pragma unroll
        for (int a = 0; a < N; ++a) {
            float m[N], y[M];
#pragma unroll
            for (int c = 0; c < N; ++c) m[c] = src[(a * N + c) * 64];
            wax_at<AX>(m, y);
#pragma unroll
            for (int v = 0; v < M; ++v) t[a][v] = y[v];
        }
        const float sc = p.scale ? p.scale[mrow] : 1.f, sf = p.shift ? p.shift[mrow] : 0.f;
        float* __restrict__ yo = p.y + (size_t)b * p.y_bs + (size_t)mrow * p.y_cs + p.y_org + (size_t)M * sd * p.y_ds + M * sh * p.y_hs + pw;
#pragma unroll
        for (int v = 0; v < M; ++v) {
            float m[N], y[M];
#pragma unroll
            for (int a = 0; a < N; ++a) m[a] = t[a][v];
            wax_at<AX>(m, y);
#pragma unroll
            for (int u = 0; u < M; ++u)
                if (M * sd + u < p.Dout && M * sh + v < p.Hout) yo[(size_t)u * p.y_ds + v * p.y_hs] = wino_act(y[u], sc, sf, lo);
        }
    }
}

// ---- the same nesting for a 2D layer, over H and W (ax = 2): 36 classes of a 1 x 1 kernel — K = Cin, 36 multiply-adds per 16
// outputs where the direct form spends 144 and the one-axis form 72.  With no tap left to shift along W the positions of the whole
// sub-batch are laid out FLAT: V[cls = a 6 + b][Cin][npad], n = (sample, row group, column group), a = the column class, b = the
// row class — the class GEMM sees one "sample" npad columns wide, so every gather is 16-byte even over a 7 x 7 grid of groups.
// one thread per (cin, sample, row group, column group), positions innermost — a wave's 36 stores are 256 contiguous bytes each
// (the windows it reads lie in a few 3.6 KB planes: L1 / L2 hits): a 6 x 6 window, B^T along H then along W
__global__ __launch_bounds__(256) void wino2p_input_kernel(const float* __restrict__ x, float* __restrict__ V, unsigned total, int Cin,
                                                           int Hp, int Wp, int SH, int SW, unsigned npad, unsigned nn, FastDiv dSW,
                                                           FastDiv dSH, FastDiv dN) {
    constexpr int N = 6, M = 4;
    const size_t cstride = (size_t)Cin * npad;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned c = (unsigned)dN.div((int)i);                     // i = c nn + n, n = (sample, sh, sw)
        const unsigned n = i - c * nn;
        const unsigned row = (unsigned)dSW.div((int)n);                  // (sample, sh)
        const int sw = (int)(n - row * (unsigned)SW);
        const unsigned b = (unsigned)dSH.div((int)row);
        const int sh = (int)(row - b * (unsigned)SH);
        const float* __restrict__ src = x + (((size_t)b * Cin + c) * Hp + M * sh) * Wp + M * sw;
        float t[N][N];                                                   // [row class][column]
#pragma unroll
        for (int jc = 0; jc < N; ++jc) {
            float r[N], v[N];
#pragma unroll
            for (int ir = 0; ir < N; ++ir) r[ir] = (M * sh + ir < Hp && M * sw + jc < Wp) ? src[(size_t)ir * Wp + jc] : 0.f;
            wax_bt<0>(r, v);
#pragma unroll
            for (int ir = 0; ir < N; ++ir) t[ir][jc] = v[ir];
        }
        float* __restrict__ dst = V + (size_t)c * npad + n;
#pragma unroll
        for (int bb = 0; bb < N; ++bb) {
            float v[N];
            wax_bt<0>(t[bb], v);
#pragma unroll
            for (int a = 0; a < N; ++a) dst[(size_t)(a * N + bb) * cstride] = v[a];
        }
    }
}

// the same transform with the planes staged in LDS: a workgroup owns one channel of NS samples (NS x SH x SW <= 256 groups), loads
// their padded planes with 16-byte accesses and reads the 6 x 6 windows from LDS (the flat kernel's 36 loads per thread are 16 bytes
// apart between lanes: 3.2 TB/s); same operations per value, same bits
typedef float wv4f_u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte global access at a dword-aligned address
__global__ __launch_bounds__(256) void wino2p_input_lds_kernel(const float* __restrict__ x, float* __restrict__ V, int B, int Cin, int Hp,
                                                               int Wp, int SH, int SW, int NS, unsigned npad) {
    extern __shared__ __attribute__((aligned(16))) float w2p_sx[];
    constexpr int N = 6, M = 4;
    const int c = blockIdx.x % Cin, b0 = (blockIdx.x / Cin) * NS;
    const int ns = B - b0 < NS ? B - b0 : NS;
    const int plane = Hp * Wp, G = SH * SW;
    for (int sidx = 0; sidx < ns; ++sidx) {
        const float* __restrict__ src = x + ((size_t)(b0 + sidx) * Cin + c) * plane;
        float* dstp = w2p_sx + sidx * plane;
        if ((plane & 3) == 0) {
            for (int i = threadIdx.x; i < plane / 4; i += 256)
                reinterpret_cast<wv4f*>(dstp)[i] = reinterpret_cast<const wv4f_u*>(src)[i];      // (x: 4-byte alignment only)
        } else {
            for (int i = threadIdx.x; i < plane; i += 256) dstp[i] = src[i];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= ns * G) return;
    const int sidx = t / G, g = t - sidx * G;
    const int sh = g / SW, sw = g - sh * SW;
    const float* __restrict__ src = w2p_sx + sidx * plane + (M * sh) * Wp + M * sw;
    const size_t cstride = (size_t)Cin * npad;
    float tt[N][N];                                                      // [row class][column]
#pragma unroll
    for (int jc = 0; jc < N; ++jc) {
        float r[N], v[N];
#pragma unroll
        for (int ir = 0; ir < N; ++ir) r[ir] = (M * sh + ir < Hp && M * sw + jc < Wp) ? src[ir * Wp + jc] : 0.f;
        wax_bt<0>(r, v);
#pragma unroll
        for (int ir = 0; ir < N; ++ir) tt[ir][jc] = v[ir];
    }
    float* __restrict__ dst = V + (size_t)c * npad + (size_t)(b0 + sidx) * G + g;
#pragma unroll
    for (int bb = 0; bb < N; ++bb) {
        float v[N];
        wax_bt<0>(tt[bb], v);
#pragma unroll
        for (int a2 = 0; a2 < N; ++a2) dst[(size_t)(a2 * N + bb) * cstride] = v[a2];
    }
}

hipError_t launch_wino2p_input(const float* x, float* V, int B, int Cin, int Hp, int Wp, int SH, int SW, long long npad, hipStream_t s) {
    const long long nn = (long long)B * SH * SW, total = nn * Cin;
    if (total >= (1ll << 31) || npad >= (1ll << 31)) return hipErrorInvalidValue;
    const int G = SH * SW;
    if (G <= 256) {
        int NS = 256 / G;
        if (NS > B) NS = B;
        while (NS > 1 && (size_t)NS * Hp * Wp * 4 > 48 * 1024) --NS;
        const size_t lds = (size_t)NS * Hp * Wp * 4;
        if (lds <= 48 * 1024) {
            const long long blocks = (long long)Cin * ((B + NS - 1) / NS);
            if (blocks < (1ll << 31)) {
                hipLaunchKernelGGL(wino2p_input_lds_kernel, dim3((unsigned)blocks), dim3(256), lds, s, x, V, B, Cin, Hp, Wp, SH, SW, NS,
                                   (unsigned)npad);
                return hipGetLastError();
            }
        }
    }
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    hipLaunchKernelGGL(wino2p_input_kernel, grid, dim3(256), 0, s, x, V, (unsigned)total, Cin, Hp, Wp, SH, SW, (unsigned)npad, (unsigned)nn,
                       FastDiv((unsigned)SW), FastDiv((unsigned)SH), FastDiv((unsigned)nn));
    return hipGetLastError();
}

// w[Cout][Cin][3][3] -> Up[cls = a 6 + b][cin][CoutPad]: G along W (a), then along H (b)
__global__ void pack_wino2p_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int CoutPad) {
    const size_t per_cls = (size_t)Cin * CoutPad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 36 * per_cls; i += (size_t)gridDim.x * blockDim.x) {
        const int cls = (int)(i / per_cls);
        const int ca = cls / 6, cb = cls - ca * 6;
        const size_t r = i % per_cls;
        const int co = (int)(r % CoutPad);
        const int cin = (int)(r / CoutPad);
        float v = 0.f;
        if (co < Cout) {
            const float* g = w + ((size_t)co * Cin + cin) * 9;
            float gh[3];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float gw[3] = {g[kh * 3], g[kh * 3 + 1], g[kh * 3 + 2]};
                gh[kh] = wax_g<0>(ca, gw);
            }
            v = wax_g<0>(cb, gh);
        }
        wp[i] = v;
    }
}

// 2D: one workgroup per (cout, PL consecutive samples): slabs -> PL whole padded planes.  SEMI: [a][row][Cout][npad] (A^T along H
// already applied by the class kernel), otherwise [a 6 + b][Cout][npad]: A^T along H, then along W.  y_hs = W + 2 halo, y_cs = a plane.
// TOV (S3R_LAYOUT_WINO_HW output; halo 1, edge a multiple of 4): the planes never leave LDS — the workgroup applies the NEXT layer's
// input transform to them (wino2p_input_kernel's arithmetic on the values it would have read back) and writes that layer's 36
// plane sets V[cls][cout][position]: the positions of its PL samples are one contiguous run per class
template <bool SEMI, bool TOV>
__global__ __launch_bounds__(256) void wino2p_finish_kernel(const ConvParams p, const int npad, const int halo, const int PL) {
    constexpr int N = 6, M = 4;
    extern __shared__ __attribute__((aligned(16))) float fsm[];          // PL planes of Hp x Wp
    const int tid = threadIdx.x;
    const int G = p.Nh * p.Nw, Wp = TOV ? p.Hout + 2 : p.y_hs, plane = TOV ? Wp * Wp : p.y_cs;
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    const size_t cstride = (size_t)p.Cout * npad;
    const int nbg = (p.B + PL - 1) / PL;
    for (int item = blockIdx.x; item < p.Cout * nbg; item += gridDim.x) {
        const int mrow = item / nbg;
        const int b0 = (item - mrow * nbg) * PL;
        const int npl = p.B - b0 < PL ? p.B - b0 : PL;
        for (int i = tid; i < npl * plane; i += 256) fsm[i] = 0.f;
        __syncthreads();
        const float sc = p.scale ? p.scale[mrow] : 1.f, sf = p.shift ? p.shift[mrow] : 0.f;
        for (int t = tid; t < npl * G; t += 256) {
            const int pl = p.dS.div(t);
            const int s = t - pl * G;
            const int sh = p.dW.div(s);
            const int sw = s - sh * p.Nw;
            const int n = b0 * G + t;
            const float* __restrict__ src = p.part + ((size_t)mrow * (npad >> 6) + (n >> 6)) * ((SEMI ? N * M : N * N) * 64) + (n & 63);
            float tt[N][M];                                              // [column class][output row]
#pragma unroll
            for (int a = 0; a < N; ++a) {
                if constexpr (SEMI) {                                    // (slabs blocked by (cout, 64-position tile))
#pragma unroll
                    for (int v = 0; v < M; ++v) tt[a][v] = src[(a * M + v) * 64];
                } else {
                    float m[N], y[M];
#pragma unroll
                    for (int c = 0; c < N; ++c) m[c] = src[(a * N + c) * 64];
                    wax_at<0>(m, y);
#pragma unroll
                    for (int v = 0; v < M; ++v) tt[a][v] = y[v];
                }
            }
            float* __restrict__ o = fsm + pl * plane + (halo + M * sh) * Wp + halo + M * sw;
#pragma unroll
            for (int v = 0; v < M; ++v) {
                float m[N], y[M];
#pragma unroll
                for (int a = 0; a < N; ++a) m[a] = tt[a][v];
                wax_at<0>(m, y);
#pragma unroll
                for (int u = 0; u < M; ++u)
                    if (M * sh + v < p.Hout && M * sw + u < p.Hout) o[v * Wp + u] = wino_act(y[u], sc, sf, lo);
            }
        }
        __syncthreads();
        if constexpr (TOV) {
            for (int t = tid; t < npl * G; t += 256) {
                const int pl = p.dS.div(t);
                const int s = t - pl * G;
                const int sh = p.dW.div(s);
                const int sw = s - sh * p.Nw;
                const float* __restrict__ win = fsm + pl * plane + M * sh * Wp + M * sw;     // 6 x 6 window of the padded plane
                float tt[N][N];                                          // [row class][column]
#pragma unroll
                for (int jc = 0; jc < N; ++jc) {
                    float r[N], v[N];
#pragma unroll
                    for (int ir = 0; ir < N; ++ir) r[ir] = win[ir * Wp + jc];
                    wax_bt<0>(r, v);
#pragma unroll
                    for (int ir = 0; ir < N; ++ir) tt[ir][jc] = v[ir];
                }
                float* __restrict__ dst = p.y + (size_t)mrow * npad + (size_t)b0 * G + t;
#pragma unroll
                for (int bb = 0; bb < N; ++bb) {
                    float v[N];
                    wax_bt<0>(tt[bb], v);
#pragma unroll
                    for (int a = 0; a < N; ++a) dst[(size_t)(a * N + bb) * cstride] = v[a];
                }
            }
        } else {
            for (int pl = 0; pl < npl; ++pl)
                wino2_copy_out(fsm + pl * plane, p.y + (size_t)(b0 + pl) * p.y_bs + (size_t)mrow * p.y_cs, plane, tid);
        }
        __syncthreads();
    }
}

// which form a two-axis launch takes (same bits): class-parallel (one workgroup per class: 36 / 25 per tile) or — F(4,3) x F(4,3)
// only — semi-fused (one workgroup per depth class walks its six row classes: a third less slab traffic, six times the work
// per workgroup: for grids that fill the chip several times over).  forced: -1 the plan, 0 class-parallel, 1 semi-fused
int wino2_form(int ax, int cout, int ntotal, int forced) {
    if (ax == 1) return 0;
    if (forced >= 0) return forced ? 1 : 0;
    static const int env_form = getenv("S3R_WINO2_FORM") ? atoi(getenv("S3R_WINO2_FORM")) : -1;      // A/B switch, read once
    if (env_form >= 0) return env_form ? 1 : 0;
    const long semi_wgs = (long)((cout + WBM - 1) / WBM) * ((ntotal + WCN - 1) / WCN) * 6;
    // 3D: >= two rounds of the chip's four slots per CU.  2D: a class is Cin / 32 K tiles only, too short a workgroup on its own —
    // semi-fused from half a round on
    return semi_wgs >= (ax == 2 ? 2 : 8) * (long)cu_count() ? 1 : 0;
}
int64_t wino2_npad(int64_t ntotal) { return (ntotal + WCN - 1) / WCN * WCN; }
int64_t wino2_slab_elems(int ax, int cout, int ntotal, int form) {
    const int64_t npad = (int64_t)((ntotal + WCN - 1) / WCN) * WCN;
    return (form ? 6 * 4 : wino2_classes(ax)) * (int64_t)cout * npad;
}

// p: the CLASS convolution (wino_body): x = V, x_cs / x_ds / x_hs / x_cls its strides, Nd / Nh = depth / row groups, kd = kh = 1,
// T = kw, ncls = the class count; part = slabs; y / Dout / Hout the layer's output
hipError_t launch_conv_wino2(ConvParams p, int ax, int form, bool to_v, hipStream_t stream, int* launches) {
    if (p.Cin % WBK != 0 || p.stride != 1 || p.transposed || p.ksplit != 1 || p.head_w || p.act == ACT_SIGMOID || !p.part ||
        ax < 0 || ax > 2 || p.ncls != wino2_classes(ax))
        return hipErrorInvalidValue;
    p.kh = 1;
    S3R_WABL(p);
    p.m_tiles = (p.Cout + WBM - 1) / WBM;
    p.n_begin = 0; p.n_end = p.Ntotal;
    const int n_tiles = (p.Ntotal + WCN - 1) / WCN;
    // finish kernels: whole padded slices / planes through LDS (the output's halo comes back from its strides)
    const int halo = to_v ? 1 : (p.y_hs - p.Hout) / 2;
    if (to_v && (ax != 2 || p.Hout % 4 != 0)) return hipErrorInvalidValue;
    if (p.out_mode && (to_v || ax == 2 || form != 0)) return hipErrorInvalidValue;      // (hand-off: the 3D class-parallel form's slabs)
    if (!to_v && (halo < 0 || p.y_hs != p.Hout + 2 * halo)) return hipErrorInvalidValue;
    if (ax == 2) {
        // p describes the layer for the finish kernel (Nh x Nw groups per sample); the class GEMM runs over the flat positions
        const int plane = to_v ? (p.Hout + 2) * (p.Hout + 2) : p.y_hs * p.y_hs, G = p.Nh * p.Nw;
        if ((!to_v && p.y_cs != plane) || (size_t)plane * 4 > 64 * 1024) return hipErrorInvalidValue;
        int PL = 256 / G < 1 ? 1 : 256 / G;
        if (PL > p.B) PL = p.B;
        while (PL > 1 && (size_t)PL * plane * 4 > 64 * 1024) --PL;
        const int npad = n_tiles * WCN;
        ConvParams q = p;
        q.B = 1; q.Nd = 1; q.Nh = 1; q.Nw = npad;
        q.dS = q.dHW = q.dW = FastDiv((unsigned)npad);
        q.kd = q.kh = q.kw = 1; q.T = 1;
        q.x_org = 0; q.x_ds = 0; q.x_hs = 0; q.x_cs = npad; q.x_cls = p.Cin * npad;
        q.x_bytes = (unsigned)(4ull * 36 * p.Cin * npad);
        q.Ntotal = npad; q.n_end = npad;
        hipError_t e = launch_wino2_classes(q, form == 1, false, stream);      // (npad % 4 == 0: 16-byte gathers)
        if (e != hipSuccess) return e;
        const long long items = (long long)p.Cout * ((p.B + PL - 1) / PL);
        const dim3 fgrid((unsigned)(items < 16384 ? items : 16384));
        const size_t flds = (size_t)PL * plane * 4;
        // (aux pass: reads the slabs, writes the output planes — or, to_v, the consumer's 36 plane sets)
        AuxScope aux(stream, 4.0 * (double)p.Cout * ((double)(form == 1 ? 24 : 36) * npad + (to_v ? 36.0 * npad : (double)p.B * plane)));
        if (to_v) {
            if (form == 1) hipLaunchKernelGGL((wino2p_finish_kernel<true, true>), fgrid, dim3(256), flds, stream, p, npad, halo, PL);
            else hipLaunchKernelGGL((wino2p_finish_kernel<false, true>), fgrid, dim3(256), flds, stream, p, npad, halo, PL);
        } else if (form == 1) hipLaunchKernelGGL((wino2p_finish_kernel<true, false>), fgrid, dim3(256), flds, stream, p, npad, halo, PL);
        else hipLaunchKernelGGL((wino2p_finish_kernel<false, false>), fgrid, dim3(256), flds, stream, p, npad, halo, PL);
        if (launches) *launches = 2;
        return hipGetLastError();
    }
    if (p.y_ds != p.y_hs * p.y_hs || p.y_cs != (p.Dout + 2 * halo) * p.y_ds) return hipErrorInvalidValue;
    // The cost volume's plane sets (p.cv_n; (.., depth group, padded column, row group)): p stays the finish kernels' view, the class
    // GEMM walks q — one flat run of n * n / 4 positions per depth group, the three column taps n / 4 elements apart as "depth" taps
    // (tap order, packed weights and so the K order are the layer's own) — and leaves out the dead K tiles where a 32-bit mask holds a class's
    ConvParams q = p;
    const bool cvl = p.cv_n > 0;
    if (cvl) {
        if (ax != 0 || p.kw != 3 || p.Nw != p.cv_n || p.Nh * 4 != p.cv_n || p.Nd != p.Nh || (p.Cin & 1)) return hipErrorInvalidValue;
        q.Nd = 1; q.Nh = p.Nd; q.Nw = p.Nw * p.Nh;
        q.dS = q.dHW = FastDiv((unsigned)(q.Nh * q.Nw)); q.dW = FastDiv((unsigned)q.Nw);
        q.kd = 3; q.kw = 1; q.T = 3;
        q.x_hs = p.x_hs * p.Nh; q.x_ds = p.Nh;
        p.dNh = q.dNh = FastDiv((unsigned)p.Nh);      // (row groups per column = depth groups per sample: p.Nd == p.Nh)
    }
    const bool cvl_skip = cvl && 3 * (p.Cin / WBK) <= 32;
    if (form == 1) {
        // (only this form's finish kernel stages output slices in LDS: the class-parallel form's flat kernel has no edge limit)
        const int M = wino2_outputs(ax), G = p.Nh * p.Nw;
        if (ax != 0 || (size_t)M * p.y_ds * 4 > 64 * 1024) return hipErrorInvalidValue;
        int SUB = 256 / G < 1 ? 1 : 256 / G;               // (sample, depth group) pairs per finish workgroup
        if (SUB > p.B * p.Nd) SUB = p.B * p.Nd;
        while (SUB > 1 && (size_t)SUB * M * p.y_ds * 4 > 64 * 1024) --SUB;
        const size_t flds = (size_t)SUB * M * p.y_ds * 4;
        const FastDiv dNd((unsigned)p.Nd), dMS((unsigned)(M * p.y_ds));
        const long long items = (long long)p.Cout * ((p.B * p.Nd + SUB - 1) / SUB);
        const dim3 fgrid((unsigned)(items < 32768 ? items : 32768));
        hipError_t e = launch_wino2_classes(q, true, cvl_skip, stream);
        if (e != hipSuccess) return e;
        AuxScope aux(stream, 4.0 * (double)p.Cout * (24.0 * n_tiles * WCN + (double)p.B * p.y_cs));      // (slabs in, padded output out)
        hipLaunchKernelGGL(wino2s_finish_kernel, fgrid, dim3(256), flds, stream, p, n_tiles * WCN, halo, SUB, dNd, dMS);
        if (launches) *launches = 2;
        return hipGetLastError();
    }
    hipError_t e = launch_wino2_classes(q, false, cvl_skip, stream);
    if (e != hipSuccess) return e;
    if (launches) *launches = 2;
    if (p.out_mode) return launch_wino_handoff(p, ax, p.out_mode - 1, n_tiles * WCN, stream);
    const long long total = (long long)p.Cout * p.Ntotal;
    const long long blocks = (total + 255) / 256;
    const dim3 flat((unsigned)(blocks < 8192 ? blocks : 8192));
    AuxScope aux(stream, 4.0 * (double)p.Cout * ((double)p.ncls * n_tiles * WCN + (double)p.B * p.Dout * p.Hout * p.Nw));
    if (ax == 0) hipLaunchKernelGGL(wino2_finish_flat_kernel<0>, flat, dim3(256), 0, stream, p, n_tiles * WCN);
    else hipLaunchKernelGGL(wino2_finish_flat_kernel<1>, flat, dim3(256), 0, stream, p, n_tiles * WCN);
    if (launches) *launches = 2;
    return hipGetLastError();
}

}  // namespace s3r
