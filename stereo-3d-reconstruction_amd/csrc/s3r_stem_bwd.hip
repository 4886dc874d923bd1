// Backward of the stem  y = act(conv2d(X, w; 3 -> 32, k 3, stride 2, pad 1) * scale[o] + shift[o])  (s3r_stem_backward): the weight and
// shift gradients of the encoder's first layer, read from the renders AS THE FORWARD READS THEM — fp32 or 8-bit (render_f32, the
// correctly rounded float32(u) / float32(255)), the left and right batches in two tensors without a concatenation copy.  There is no gs
// output and no input gradient: nothing upstream of an image is trained.
//
//   g, gs         s3r_conv_backward's rule:  none: g = grad_y;  ReLU: g = (y > 0.f) ? grad_y : 0.f;  gs = g * scale[o] rounded once
//   grad_shift[o] = sum g: the conv backward's OWN two kernels (convbwd_prep_kernel without a gs output + convbwd_shift_finish_kernel,
//                   launch_convbwd_prep) over (image, channel) rows of S = m^2 positions: the same code, hence the same bits.  A pass
//                   of its own over grad_y and y: the chunks of 512 flat positions it sums do not line up with the output rows the
//                   weight-gradient kernel walks.
//   grad_w[o][ci][kh][kw] = sum_{image, oh, ow} gs[image][o][oh][ow] X[image][ci][2 oh - 1 + kh][2 ow - 1 + kw]   (X is 0 outside the image)
//
// stem_bwd_gw_kernel: the GEMM M = 32 channels o, N = 27 taps (ci, kh, kw) padded to 32, K = positions on v_mfma_f32_32x32x2_f32; the five
//   dead columns are 0 in the B operand and never stored.  A workgroup is ONE wave and owns one K slice: `rps` consecutive output rows of
//   one image (stem_bwd_rows: a function of m alone, at most 32 slices per image).  It walks its rows in ascending oh and a row in segments
//   of <= 64 positions in ascending ow; per segment it stages
//     As[o][p]   gs of the 32 channels, loaded as [channel][run of positions] with 16-byte accesses where the four positions lie inside the
//                row, row stride 65 (odd: the 32 channel rows of a half-wave's fragment read land in 32 banks);
//     Xs[r][c]   the nine input rows r = 3 ci + kh (input row 2 oh - 1 + kh of channel ci), columns 2 w0 - 1 .. 2 w0 + 127, row stride 131
//                (= 3 mod 32: tap n = 3 r + kw of position p reads word 131 r + 2 p + kw, so the 27 live lanes of a half-wave read banks
//                n + const: no split into even and odd columns is needed for the stride-2 walk).  The zero padding is WRITTEN here.
//   Positions beyond the row and elements outside the image are loaded from clamped addresses and replaced by 0; the B operand is 0 as
//   well beyond the row's last position (0 * NaN would be NaN).  Lane l feeds A[o = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31]:
//   one instruction adds the positions 2 t and 2 t + 1 of the segment, in that order.  The slice's 32 x 27 sums go to slab
//   [image nsl + slice] (to grad_w itself when the call has one slab).
// stem_bwd_image_kernel: per element, an image's slabs in ascending slice order starting from slab 0 (skipped when an image is one slice).
// stem_bwd_batch_kernel: per element, the images' partials in ascending image index starting from image 0's (skipped for one image).
// An image's partial is therefore a function of in_size and its own data only.  64-bit element arithmetic; one-dimensional grids.
#include "s3r_ordered.h"

namespace s3r {

typedef float f32x16_s __attribute__((ext_vector_type(16)));
constexpr int SB_CO = 32;                      // output channels: the M tile
constexpr int SB_TAPS = 27;                    // 3 x 3 x 3 taps: the live columns of the N tile
constexpr int SB_RUN = 64;                     // positions per staged segment
constexpr int SB_ASTR = SB_RUN + 1;            // 65
constexpr int SB_XSTR = 131;                   // >= the 2 * SB_RUN + 1 = 129 input columns that serve 64 positions x 3 taps at stride 2, and = 3 mod 32
constexpr int SB_SLAB = SB_CO * SB_TAPS;       // 864

// output rows per K slice: a function of m alone; at most 32 slices per image
int stem_bwd_rows(int m) { return (m + 31) / 32; }
static int sb_slices(int m) { const int rps = stem_bwd_rows(m); return (m + rps - 1) / rps; }

template <typename TI>
__global__ __launch_bounds__(64, 3) void stem_bwd_gw_kernel(const TI* __restrict__ left, const TI* __restrict__ right, int n_left,
                                                         const float* __restrict__ y, const float* __restrict__ gy,
                                                         const float* __restrict__ scale, float* __restrict__ out, int n, int m, int rps,
                                                         int nsl, int act) {
    __shared__ float sb_lds[SB_CO * SB_ASTR + 9 * SB_XSTR];
    float* __restrict__ As = sb_lds;                                     // [32][65]
    float* __restrict__ Xs = sb_lds + SB_CO * SB_ASTR;                   // [9][131]
    const int lane = threadIdx.x;
    const long long b = blockIdx.x / nsl;
    const int z = (int)(blockIdx.x - b * nsl);
    const long long S = (long long)m * m, P = (long long)n * n;
    const TI* __restrict__ img = b < n_left ? left + (size_t)b * 3 * P : right + (size_t)(b - n_left) * 3 * P;
    const float* __restrict__ gyb = gy + (size_t)b * SB_CO * S;
    const float* __restrict__ yb = act ? y + (size_t)b * SB_CO * S : gyb;      // (never read when act is none)
    const int q4 = 4 * (lane & 15), cq = lane >> 4;                      // staging: channel c0 + cq, positions w0 + q4 .. + 3
    float scv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) scv[u] = scale ? scale[4 * u + cq] : 1.f;
    const int j = lane & 31, h = lane >> 5;                              // fragment: channel / tap j, position parity h
    const bool live = j < SB_TAPS;
    const int xr = live ? j / 3 : 0, kw = live ? j - 3 * xr : 0;
    const float* __restrict__ ar = As + j * SB_ASTR + h;
    const float* __restrict__ br = Xs + xr * SB_XSTR + kw + 2 * h;
    f32x16_s acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int oh0 = z * rps, oh1 = min(m, oh0 + rps);
    for (int oh = oh0; oh < oh1; ++oh)
        for (int w0 = 0; w0 < m; w0 += SB_RUN) {
            const int len = min(SB_RUN, m - w0);
            // -- global loads of the segment: gs operands, then the nine input rows
            v4f gv[8], yv[8];
            const bool quad = w0 + q4 + 3 < m;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t row = (size_t)(4 * u + cq) * S + (size_t)oh * m;
                if (quad) {
                    gv[u] = *reinterpret_cast<const v4f_u*>(gyb + row + w0 + q4);
                    yv[u] = act ? *reinterpret_cast<const v4f_u*>(yb + row + w0 + q4) : v4f{0.f, 0.f, 0.f, 0.f};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool ok = w0 + q4 + i < m;
                        const size_t at = row + (ok ? w0 + q4 + i : 0);          // (clamped to the row's first position)
                        const float g = gyb[at];
                        const float v = act ? yb[at] : 0.f;
                        gv[u][i] = ok ? g : 0.f;
                        yv[u][i] = ok ? v : 0.f;
                    }
                }
            }
            // (row r, columns lane and 64 + lane; the rows' last column, 128, is lane r's third element)
            float xv[19];
            const int iw0 = 2 * w0 - 1;
#pragma unroll
            for (int u = 0; u < 19; ++u) {
                const int r = u < 18 ? u >> 1 : min(lane, 8);
                const int c = u < 18 ? 64 * (u & 1) + lane : 2 * SB_RUN;
                const int ci = r / 3, kh = r - 3 * ci;
                const int ih = 2 * oh - 1 + kh, iw = iw0 + c;
                const bool ok = ih >= 0 && ih < n && iw >= 0 && iw < n;
                const size_t at = ok ? ((size_t)ci * n + ih) * n + iw : (size_t)0;      // (clamped to the image's first element)
                const float v = render_f32(img[at]);
                xv[u] = ok ? v : 0.f;
            }
            __syncthreads();                                             // the previous segment has been read
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float* __restrict__ dst = As + (4 * u + cq) * SB_ASTR + q4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = w0 + q4 + i < m;
                    const float g = act == 1 ? ((yv[u][i] > 0.f) ? gv[u][i] : 0.f) : gv[u][i];      // (act_grad's none / ReLU, s3r_ordered.h)
                    const float gs = scale ? g * scv[u] : g;
                    dst[i] = ok ? gs : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 18; ++u) Xs[(u >> 1) * SB_XSTR + 64 * (u & 1) + lane] = xv[u];
            if (lane < 9) Xs[lane * SB_XSTR + 2 * SB_RUN] = xv[18];
            __syncthreads();
            const int nt = (len + 1) >> 1;
            for (int t = 0; t < nt; ++t) {
                const float av = ar[2 * t];                              // (0 where the position is beyond the row)
                const float v = br[4 * t];
                const float bv = (live && 2 * t + h < len) ? v : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        }
    if (!live) return;
    float* __restrict__ dst = out + (size_t)blockIdx.x * SB_SLAB;        // (slab 0 when the call has one slab: grad_w itself)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[o * SB_TAPS + j] = acc[r];
    }
}

// part[b][i] = an image's slabs in ascending slice order, starting from its slab 0
__global__ __launch_bounds__(256) void stem_bwd_image_kernel(const float* __restrict__ slabs, float* __restrict__ part, int nsl) {
#pragma clang fp contract(off)
    const long long b = blockIdx.x >> 2;
    const int i = (blockIdx.x & 3) * 256 + threadIdx.x;
    if (i >= SB_SLAB) return;
    const float* __restrict__ src = slabs + (size_t)b * nsl * SB_SLAB + i;
    float p = src[0];
    int z = 1;
    for (; z + 8 <= nsl; z += 8) {                                       // eight loads in flight, then the adds in the same ascending order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(z + u) * SB_SLAB];
#pragma unroll
        for (int u = 0; u < 8; ++u) p = p + v[u];
    }
    for (; z < nsl; ++z) p = p + src[(size_t)z * SB_SLAB];
    part[(size_t)b * SB_SLAB + i] = p;
}

// grad_w[i] = the images' partials in ascending image index, starting from image 0's
__global__ __launch_bounds__(256) void stem_bwd_batch_kernel(const float* __restrict__ part, float* __restrict__ gw, int B) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SB_SLAB) return;
    float acc = part[i];
    int b = 1;
    for (; b + 8 <= B; b += 8) {                                         // eight loads in flight, then the adds in the same ascending order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(b + u) * SB_SLAB + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + v[u];
    }
    for (; b < B; ++b) acc = acc + part[(size_t)b * SB_SLAB + i];
    gw[i] = acc;
}

// [chunk sums of g: 32 B ceil(m^2 / 512)][slabs: B nsl 864][per-image partials: B 864] — the worst case over the outputs asked for
int64_t stem_backward_scratch_elems(int B, int m) {
    if (B <= 0) return 0;
    const long long S = (long long)m * m;
    return (int64_t)SB_CO * B * chunks(S) + (int64_t)B * sb_slices(m) * SB_SLAB + (int64_t)B * SB_SLAB;
}

hipError_t launch_stem_backward(const void* left, const void* right, int n_left, int u8, const float* y, const float* gy,
                                const float* scale, float* gw, float* gshift, int B, int n, int m, int act, float* scratch, hipStream_t s,
                                int* launches) {
    *launches = 0;
    const long long S = (long long)m * m;
    const int nsl = sb_slices(m), rps = stem_bwd_rows(m);
    float* part = scratch;
    float* slabs = part + (size_t)SB_CO * B * chunks(S);
    float* imgs = slabs + (size_t)B * nsl * SB_SLAB;
    if (gshift) {
        hipError_t e = launch_convbwd_prep(y, gy, nullptr, nullptr, gshift, B, SB_CO, S, act, part, s, launches);
        if (e != hipSuccess) return e;
    }
    if (gw) {
        const long long nslab = (long long)B * nsl;
        float* dst = nslab > 1 ? slabs : gw;
        if (u8)
            hipLaunchKernelGGL((stem_bwd_gw_kernel<unsigned char>), dim3((unsigned)nslab), dim3(64), 0, s, (const unsigned char*)left,
                               (const unsigned char*)right, n_left, y, gy, scale, dst, n, m, rps, nsl, act);
        else
            hipLaunchKernelGGL((stem_bwd_gw_kernel<float>), dim3((unsigned)nslab), dim3(64), 0, s, (const float*)left, (const float*)right,
                               n_left, y, gy, scale, dst, n, m, rps, nsl, act);
        ++*launches;
        const float* per_image = slabs;                                  // (an image of one slice: its slab is its partial)
        if (nsl > 1) {
            AuxScope aux(s, 4.0 * SB_SLAB * ((double)nslab + B));
            float* to = B > 1 ? imgs : gw;
            hipLaunchKernelGGL(stem_bwd_image_kernel, dim3((unsigned)(4 * B)), dim3(256), 0, s, slabs, to, nsl);
            ++*launches;
            per_image = imgs;
        }
        if (B > 1) {
            AuxScope aux(s, 4.0 * SB_SLAB * ((double)B + 1.0));
            hipLaunchKernelGGL(stem_bwd_batch_kernel, dim3(4), dim3(256), 0, s, per_image, gw, B);
            ++*launches;
        }
    }
    return hipGetLastError();
}

}  // namespace s3r
