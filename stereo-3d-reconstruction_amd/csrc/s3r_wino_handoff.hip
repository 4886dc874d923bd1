// The 3D hand-off pass of the Winograd forms (map and transforms: s3r_wino.h): wino_handoff_kernel and its launcher, which the
// class-parallel launchers of s3r_wino_gemm.hip and s3r_wino_axis2.hip and the direct path's split-K finish call in place of
// their own finish pass.
#include "s3r_wino.h"

namespace s3r {

// ---- hand-off passes of the small 3D layers (v4 -> v5 -> v6 -> d1 -> d2): the producer's finish pass wrote a plain activation of a
// few MB that the consumer's operand pass read straight back — two launch-bound passes over a tensor that never leaves the L2.
// ONE pass instead: a workgroup owns one sample and CB couts; it finishes them from the producer's raw sums into LDS as the
// consumer's halo-padded input (halo +0.0), and after a barrier forms the consumer's operand from the LDS copy.  Same device functions
// (wax_at / wino_out / wino_act; wax_bt; the difference formulas of wino_diff_kernel; conv_finish_kernel's kz-ordered sum and
// epilogue), same order, same values: the bits of the two passes.  Everything here is adds, subtractions and explicit fmaf.
//   PROD 0 / 1: class slabs of the class-parallel two-axis form, F(4,3)^2 / F(2,4)^2 (wino2_finish_flat_kernel<PROD>)
//   PROD 2:     class slabs of the class-parallel transposed form, whole range (wino_finish_kernel<2, false>, n_begin = 0)
//   PROD 3:     split-K partial slabs of the direct kernel (conv_finish_kernel, convolution, dense output)
//   CONS 0 / 1: V[ncls][B][C][SG][SG][Op] of the two-axis form (wino2_input_kernel<CONS>); the plain activation is not written
//   CONS 2:     [x | Dh | Dd | Ddh] over the padded volume (wino_diff_kernel<true>); x whole, its halo rewritten with +0.0
// On = the producer's true output edge, Op = On + 2 halo the consumer's padded input edge
template <int PROD, int CONS>
__global__ __launch_bounds__(256) void wino_handoff_kernel(const ConvParams p, const int npad, const int CB, const int On, const int halo,
                                                           const int SG, const FastDiv dG1, const FastDiv dG2, const FastDiv dOp,
                                                           const FastDiv dOp2, const FastDiv dSG) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];            // CB volumes of Op^3
    const int tid = threadIdx.x;
    const int Op = On + 2 * halo, hs = Op, ds = Op * Op, vol = ds * Op, org = halo * (ds + hs + 1);
    const int S = p.Nd * p.Nh * p.Nw;                                      // the producer's positions per sample
    const int G1 = PROD == 2 ? 8 * S : S;                                  // (transposed: x 8 parity classes)
    const int G2 = CONS == 2 ? vol : SG * SG * Op;
    const int ncb = (p.Cout + CB - 1) / CB;
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    // (CONS 2: the padded edge is even — edge % 4 == 0 — so a volume, a row and `total` are even; the caller's pointer may not be 8-byte aligned)
    const bool vec2 = CONS == 2 && (Op & 1) == 0 && (reinterpret_cast<size_t>(p.y) & 7) == 0;
    for (int item = blockIdx.x; item < p.B * ncb; item += gridDim.x) {
        const int b = item / ncb;
        const int c0 = (item - b * ncb) * CB;
        const int nc = p.Cout - c0 < CB ? p.Cout - c0 : CB;
        for (int i = tid; i < nc * vol; i += 256) hsm[i] = 0.f;
        __syncthreads();
        for (int t = tid; t < nc * G1; t += 256) {
            const int cl = dG1.div(t);
            int g = t - cl * G1;
            const int mrow = c0 + cl;
            const float sc = p.scale ? p.scale[mrow] : 1.f, sf = p.shift ? p.shift[mrow] : 0.f;
            float* __restrict__ o = hsm + cl * vol + org;
            if constexpr (PROD <= 1) {
                constexpr int N = WAxis<PROD>::N, M = WAxis<PROD>::M;
                const int n = b * S + g;
                const int sd = p.dHW.div(g);
                g -= sd * p.Nh * p.Nw;
                int sh, pw;
                wino2_group_pos(p, g, sh, pw);
                const float* __restrict__ src = p.part + ((size_t)mrow * (npad >> 6) + (n >> 6)) * (N * N * 64) + (n & 63);
                float tt[N][M];                                          // [depth class][output row]
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    float m[N], y[M];
#pragma unroll
                    for (int c = 0; c < N; ++c) m[c] = src[(a * N + c) * 64];
                    wax_at<PROD>(m, y);
#pragma unroll
                    for (int v = 0; v < M; ++v) tt[a][v] = y[v];
                }
                o += M * sd * ds + M * sh * hs + pw;
#pragma unroll
                for (int v = 0; v < M; ++v) {
                    float m[N], y[M];
#pragma unroll
                    for (int a = 0; a < N; ++a) m[a] = tt[a][v];
                    wax_at<PROD>(m, y);
#pragma unroll
                    for (int u = 0; u < M; ++u)
                        if (M * sd + u < p.Dout && M * sh + v < p.Hout) o[u * ds + v * hs] = wino_act(y[u], sc, sf, lo);
                }
            } else if constexpr (PROD == 2) {
                constexpr int NCLS = WinoKind<2>::NCLS, R = WinoKind<2>::R;
                const int pc = p.dS.div(g);
                g -= pc * S;
                const int rd = (pc >> 2) & 1, rh = (pc >> 1) & 1, rw = pc & 1;
                const int n = b * S + g;
                const int pd = p.dHW.div(g);
                g -= pd * p.Nh * p.Nw;
                const int q = p.dW.div(g);
                const int pw = g - q * p.Nw;
                const float* __restrict__ src = p.part + (size_t)pc * NCLS * 64 + ((size_t)mrow * (npad >> 6) + (n >> 6)) * (8 * NCLS * 64) + (n & 63);
                float m[NCLS], y[R];
#pragma unroll
                for (int c = 0; c < NCLS; ++c) m[c] = src[c * 64];
                wino_out<2>(m, y);
                o += (2 * pd * ds + 2 * q * hs + pw) * 2 + rd * ds + rh * hs + rw;
#pragma unroll
                for (int k = 0; k < R; ++k) o[wino_out_off<2>(k, ds, hs)] = wino_act(y[k], sc, sf, lo);
            } else {
                const int n = b * S + g;
                const float* __restrict__ src = p.part + (size_t)mrow * npad + n;
                const size_t zs = (size_t)p.Cout * npad;
                float sum = src[0];                                      // the slabs in kz order, as conv_finish_kernel adds them
                for (int z = 1; z < p.ksplit; ++z) sum += src[(size_t)z * zs];
                const int pd = p.dHW.div(g);
                g -= pd * p.Nh * p.Nw;
                const int ph = p.dW.div(g);
                const int pw = g - ph * p.Nw;
                float t1 = fmaf(sum, sc, sf);
                if (p.act == ACT_RELU) t1 = fmaxf(t1, fmaf(t1, p.slope, 0.f));
                o[pd * ds + ph * hs + pw] = t1;
            }
        }
        __syncthreads();
        const size_t base = ((size_t)b * p.Cout + c0) * G2;
        const size_t total = (size_t)p.B * p.Cout * G2;
        for (int t = tid; t < (CONS == 2 && vec2 ? 0 : nc * G2); t += 256) {
            const int cl = dG2.div(t);
            const int e = t - cl * G2;
            if constexpr (CONS <= 1) {
                constexpr int N = WAxis<CONS>::N, M = WAxis<CONS>::M;
                const int row = dOp.div(e);                              // (sd, sh)
                const int w = e - row * Op;
                const int sd = dSG.div(row);
                const int sh = row - sd * SG;
                const float* __restrict__ src = hsm + cl * vol + M * sd * ds + M * sh * hs + w;
                float tt[N][N];                                          // [depth][row class]
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    float r[N], v[N];
#pragma unroll
                    for (int c = 0; c < N; ++c) r[c] = (M * sd + a < Op && M * sh + c < Op) ? src[a * ds + c * hs] : 0.f;
                    wax_bt<CONS>(r, v);
#pragma unroll
                    for (int c = 0; c < N; ++c) tt[a][c] = v[c];
                }
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    float r[N], v[N];
#pragma unroll
                    for (int a = 0; a < N; ++a) r[a] = tt[a][c];
                    wax_bt<CONS>(r, v);
#pragma unroll
                    for (int a = 0; a < N; ++a) p.y[(size_t)(a * N + c) * total + base + t] = v[a];
                }
            } else if (!vec2) {
                const int z = dOp2.div(e);
                const int r = dOp.div(e - z * ds);
                const bool rn = r + 1 < Op, zn = z + 1 < Op;
                const float* __restrict__ src = hsm + t;                 // (cl * vol + e)
                const float x00 = src[0];
                const float x01 = rn ? src[hs] : 0.f;
                const float dh0 = rn ? x00 - x01 : 0.f;
                const float x10 = zn ? src[ds] : 0.f;
                const float x11 = (rn && zn) ? src[ds + hs] : 0.f;
                const float dh1 = rn ? x10 - x11 : 0.f;                  // Dh at depth z + 1
                float* __restrict__ dst = p.y + base + t;
                dst[0] = x00;
                dst[total] = dh0;
                dst[2 * total] = zn ? x00 - x10 : 0.f;
                dst[3 * total] = zn ? dh0 - dh1 : 0.f;
            }
        }
        if constexpr (CONS == 2) {
            // two columns per thread, as wino_diff2_kernel (rows are an even number of floats: edge + 2): half the memory instructions
            if (vec2)
                for (int t = tid * 2; t < nc * G2; t += 512) {
                    const int cl = dG2.div(t);
                    const int e = t - cl * G2;
                    const int z = dOp2.div(e);
                    const int r = dOp.div(e - z * ds);
                    const bool rn = r + 1 < Op, zn = z + 1 < Op;
                    const wv2f zero = {0.f, 0.f};
                    const float* __restrict__ src = hsm + t;
                    const wv2f x00 = *reinterpret_cast<const wv2f*>(src);
                    const wv2f x01 = rn ? *reinterpret_cast<const wv2f*>(src + hs) : zero;
                    const wv2f dh0 = rn ? x00 - x01 : zero;
                    const wv2f x10 = zn ? *reinterpret_cast<const wv2f*>(src + ds) : zero;
                    const wv2f x11 = (rn && zn) ? *reinterpret_cast<const wv2f*>(src + ds + hs) : zero;
                    const wv2f dh1 = rn ? x10 - x11 : zero;
                    float* __restrict__ dst = p.y + base + t;
                    *reinterpret_cast<wv2f*>(dst) = x00;
                    *reinterpret_cast<wv2f*>(dst + total) = dh0;
                    *reinterpret_cast<wv2f*>(dst + 2 * total) = zn ? x00 - x10 : zero;
                    *reinterpret_cast<wv2f*>(dst + 3 * total) = zn ? dh0 - dh1 : zero;
                }
        }
        __syncthreads();
    }
}

hipError_t launch_wino_handoff(const ConvParams& p, int prod, int cons, int npad, hipStream_t stream) {
    if (prod < 0 || prod > 3 || cons < 0 || cons > 2 || !p.part || !p.y || npad <= 0 || (npad & 63) || p.head_w) return hipErrorInvalidValue;
    const int Op = p.y_hs;
    if (Op <= 0 || p.y_ds != Op * Op || p.y_cs != Op * Op * Op || p.y_bs != p.Cout * p.y_cs) return hipErrorInvalidValue;
    const int halo = p.y_org / (p.y_ds + p.y_hs + 1), On = Op - 2 * halo;
    if (p.y_org != halo * (p.y_ds + p.y_hs + 1) || On <= 0) return hipErrorInvalidValue;
    // the consumer's geometry: k3 p1 reads a halo of 1, k4 p0 none (edge >= 5), the transposed form a halo of 1 over an edge % 4 == 0
    if ((cons == 0 && (halo != 1 || On < 4)) || (cons == 1 && (halo != 0 || On < 5)) || (cons == 2 && (halo != 1 || (On & 3)))) return hipErrorInvalidValue;
    const int SG = cons == 0 ? (On + 3) / 4 : cons == 1 ? (On - 2) / 2 : 1;
    const int vol = Op * Op * Op;
    if (vol > 8192) return hipErrorInvalidValue;                          // (32 KiB of LDS: a padded edge of 20)
    const int CB = 8192 / vol < 8 ? 8192 / vol : 8;
    const int S = p.Nd * p.Nh * p.Nw;
    if (p.Ntotal != p.B * S || npad < p.Ntotal) return hipErrorInvalidValue;
    double slabs;
    if (prod <= 1) {
        if (p.ncls != wino2_classes(prod) || p.Dout != On || p.Hout != On || p.Nw != On || p.act == ACT_SIGMOID) return hipErrorInvalidValue;
        slabs = (double)p.ncls * npad;
    } else if (prod == 2) {
        if (!p.transposed || cons != 2 || 2 * p.Nw != On || 4 * p.Nd != On || 4 * p.Nh != On || p.act == ACT_SIGMOID) return hipErrorInvalidValue;
        slabs = 72.0 * npad;
    } else {
        if (p.transposed || cons == 2 || p.ksplit <= 1 || p.y_step > 1 || p.shuf_s || p.Nd != On || p.Nh != On || p.Nw != On || p.act == ACT_SIGMOID)
            return hipErrorInvalidValue;
        slabs = (double)p.ksplit * npad;
    }
    const int G1 = prod == 2 ? 8 * S : S, G2 = cons == 2 ? vol : SG * SG * Op;
    const double written = cons == 2 ? 4.0 * p.B * vol : (double)wino2_classes(cons) * p.B * G2;
    if ((double)p.Cout * written >= 2147483648.0) return hipErrorInvalidValue;
    const long long items = (long long)p.B * ((p.Cout + CB - 1) / CB);
    const dim3 grid((unsigned)(items < 16384 ? items : 16384));
    const size_t lds = (size_t)CB * vol * sizeof(float);
    const FastDiv dG1((unsigned)G1), dG2((unsigned)G2), dOp((unsigned)Op), dOp2((unsigned)(Op * Op)), dSG((unsigned)SG);
    // (aux pass: reads the producer's slabs, writes the consumer's operand)
    AuxScope aux(stream, 4.0 * (double)p.Cout * (slabs + written));
#define S3R_HANDOFF(PR, CO) hipLaunchKernelGGL((wino_handoff_kernel<PR, CO>), grid, dim3(256), lds, stream, p, npad, CB, On, halo, SG, dG1, dG2, dOp, dOp2, dSG)
    switch (prod * 3 + cons) {
        case 0: S3R_HANDOFF(0, 0); break;
        case 1: S3R_HANDOFF(0, 1); break;
        case 2: S3R_HANDOFF(0, 2); break;
        case 3: S3R_HANDOFF(1, 0); break;
        case 4: S3R_HANDOFF(1, 1); break;
        case 5: S3R_HANDOFF(1, 2); break;
        case 8: S3R_HANDOFF(2, 2); break;
        case 9: S3R_HANDOFF(3, 0); break;
        case 10: S3R_HANDOFF(3, 1); break;
        default: return hipErrorInvalidValue;
    }
#undef S3R_HANDOFF
    return hipGetLastError();
}

}  // namespace s3r
