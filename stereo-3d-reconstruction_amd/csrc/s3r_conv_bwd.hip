// Backward of one fp32 convolution layer  y = act(conv(x, w) * scale[o] + shift[o])  (s3r_conv_backward): Conv or ConvTranspose, 2D or
// 3D, any k / stride / pad / output padding, dilation 1, plain NCHW / NCDHW tensors.  The input gradient is NOT here: it is the forward
// of the adjoint layer (s3r_conv_adjoint_desc) on gs.  Three results, each optional, each with a FIXED order — no atomics, the same bits
// on every run and at every 4-byte-aligned address:
//
//   g  (B,cout,S)  the pre-activation gradient, fp32, nothing fused: act_grad (s3r_ordered.h)
//   gs = g * scale[o], rounded once (g itself when scale is NULL)                                                (convbwd_prep_kernel)
//   grad_shift[o] = sum_{b,s} g[b][o][s]   s3r_ordered.h's order, a row being channel o's S positions of one sample
//                                                                                     (convbwd_prep_kernel + convbwd_shift_finish_kernel)
//   grad_w[a][f][t] = sum_{b, q} A[b][a][q] F[b][f][q s - p + t]   (F reads 0 outside its grid)    (convbwd_gw_kernel + convbwd_finish_kernel)
//       q runs over the COARSE grid (a Conv's output, a ConvTranspose's input), A lives on it with Ca channels, F on the fine grid with
//       Cf channels:  Conv: A = gs, F = x -> [cout][cin][k..];  ConvTranspose: A = x, F = gs -> [cin][cout][k..]: torch's layouts.
//
// convbwd_prep_kernel: a WAVE owns one chunk of one (sample, channel) row (s3r_ordered.h); it stores gs and the chunk's sum of g to
//   part[o][b][chunk].  convbwd_shift_finish_kernel: one wave per channel, row_total of part[o].
//
// convbwd_gw_kernel: the GEMM M = Ca, N = Cf k^nd, K = B Q on v_mfma_f32_32x32x2_f32.  Both operands are position-contiguous and
//   channel-strided, so a fragment (32 channels at one position) is strided in memory: tiles [channels][a run of positions] go through
//   LDS with loads that are contiguous along the positions, and the row strides are ODD, so the 32 channel rows of ONE half-wave's fragment
//   read land in 32 different banks (the linear backward's 33-float padding; the two half-waves, h = 0 and 1, read positions one apart
//   and may still meet on a bank: the stride does not rule that out).  A workgroup owns up to 128 rows a (one 32-row tile per wave), 32 channels f,
//   ONE outer tap (t_d, t_h) and up to four taps t_w — NT accumulator tiles per wave that share the A fragment — over one K slice.  It
//   walks the slice in chunks: R whole coarse rows (lines along W) when a row has <= 64 positions, else one segment of <= 64 positions of
//   one row.  Per chunk it stages As[a][row][q_w] and, for the outer tap, the matching fine rows Fs[f][row][w]: one staged run of the fine
//   tensor serves every tap along W (the fragment of tap t_w is the same LDS row read at q_w s + t_w).  Coarse positions, channels
//   and taps beyond the tensors — and fine positions outside the grid (the zero padding) — are loaded from clamped addresses and replaced
//   by 0 in BOTH operands (0 * NaN would be NaN); they add +0.0 products to accumulators that started as +0.0, which changes no bit.
//   K slices: a sample's chunks are cut into `nsl` slices of whole chunks, nsl a function of the layer's PER-SAMPLE geometry only
//   (convbwd_geo: about 64 workgroups per sample) — never of B, the device or an address; a slice never spans two samples.  Slice
//   (b, z) writes slab [b nsl + z][a][f][t]; convbwd_finish_kernel adds, per element, a sample's slabs in ascending z starting from its
//   slab 0, and the per-sample partials in ascending b starting from sample 0's.  One slab in all (B = 1, nsl = 1) is written straight to grad_w.
//
// All indexing is 64-bit element arithmetic on plain pointers; the grids are one-dimensional.
#include "s3r_ordered.h"

namespace s3r {

typedef float f32x16_c __attribute__((ext_vector_type(16)));
constexpr int CB_AG = 128;           // rows a per workgroup (4 waves x 32)
constexpr int CB_FT = 32;            // channels f per workgroup
constexpr int CB_RUN = 64;           // coarse positions per staged chunk (upper bound)
constexpr int CB_LDS_MAX = 64 * 1024;

// y, gy (B,Co,S); gs (B,Co,S) or NULL; part [Co][B][nch] chunk sums of g or NULL
__global__ __launch_bounds__(256) void convbwd_prep_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                           const float* __restrict__ scale, float* __restrict__ gs,
                                                           float* __restrict__ part, int B, int Co, long long S, long long nch, int act) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= (long long)B * Co * nch) return;                          // (wave-uniform; the kernel has no barrier)
    const long long row = wid / nch, k = wid - row * nch;
    const long long b = row / Co, o = row - b * Co;
    const long long s0 = k * CHUNK + 4 * lane;
    const bool full = (k + 1) * CHUNK <= S;                           // (wave-uniform)
    const float sc = scale ? scale[o] : 1.f;
    const float* __restrict__ gr = gy + (size_t)row * S;
    v4f gv[Q], yv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        gv[j] = load4(gr, s0 + 256 * j, S, full);
        yv[j] = act ? load4(y + (size_t)row * S, s0 + 256 * j, S, full) : v4f{0.f, 0.f, 0.f, 0.f};
    }
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        v4f out;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = s0 + 256 * j + i < S;
            const float v = act_grad(yv[j][i], gv[j][i], act);
            out[i] = scale ? v * sc : v;
            a = a + (in ? v : 0.f);
        }
        if (gs) store4(gs + (size_t)row * S, s0 + 256 * j, S, out, full);
    }
    if (part) {
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) a = a + __shfl_down(a, w, 64);   // (wave_tree's adds, kept open-coded: the call changes this kernel's machine code)
        if (lane == 0) part[((size_t)o * B + b) * nch + k] = a;
    }
}

// one wave per channel o: grad_shift[o] from part[o][B][nch]
__global__ __launch_bounds__(64) void convbwd_shift_finish_kernel(const float* __restrict__ part, float* __restrict__ gshift, int B,
                                                                  long long nch) {
#pragma clang fp contract(off)
    const int o = blockIdx.x, lane = threadIdx.x;
    const float acc = row_total(part + (size_t)o * B * nch, B, nch, lane);
    if (lane == 0) gshift[o] = acc;
}

template <int NT>
__global__ __launch_bounds__(256) void convbwd_gw_kernel(const float* __restrict__ A, const float* __restrict__ F,
                                                         float* __restrict__ out, ConvBwdGeo g) {
    extern __shared__ float cb_lds[];
    float* __restrict__ As = cb_lds;                                     // [CB_AG][astr]
    float* __restrict__ Fs = cb_lds + (size_t)CB_AG * g.astr;            // [CB_FT][fstr]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    // block -> (slice, tile); tile -> (a group, f tile, outer tap, tap group), tap group fastest
    const long long slice = blockIdx.x / g.tiles;
    int tile = (int)(blockIdx.x - slice * g.tiles);
    const int tg = tile % g.ntg; tile /= g.ntg;
    const int to = tile % g.To; tile /= g.To;
    const int ft = tile % g.nft;
    const int ag = tile / g.nft;
    const long long b = slice / g.nsl;
    const int sl = (int)(slice - b * g.nsl);
    const int a0 = ag * CB_AG, f0 = ft * CB_FT, tw0 = tg * NT;
    const int td = g.nd == 3 ? to / g.k : 0, th = g.nd == 3 ? to % g.k : to;
    const int cbeg = sl * g.cps, cend = min(g.nchunks, cbeg + g.cps);
    const int arow = g.R * g.WLP, frow = g.R * g.FL;
    const float* __restrict__ Ab = A + (size_t)b * g.Ca * g.Q;
    const float* __restrict__ Fb = F + (size_t)b * g.Cf * g.Pf;
    const bool wave_on = a0 + 32 * wave < g.Ca;                          // (wave-uniform)
    f32x16_c acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    for (int c = cbeg; c < cend; ++c) {
        if (c != cbeg) __syncthreads();                                  // the previous chunk has been read
        int row0, nr, w0;
        if (g.nseg == 1) { row0 = c * g.R; nr = min(g.R, g.nrows - row0); w0 = 0; }
        else { row0 = c / g.nseg; nr = 1; w0 = (c - row0 * g.nseg) * g.WL; }
        const int wl = min(g.WL, g.mc - w0);                             // coarse positions of a row inside this chunk
        for (int idx = tid; idx < CB_AG * arow; idx += 256) {            // consecutive threads: consecutive q_w of one channel
            const int a = idx / arow, rem = idx - a * arow;
            const int i = rem / g.WLP, cc = rem - i * g.WLP;
            const bool ok = a0 + a < g.Ca && i < nr && cc < wl;
            const size_t ch = (size_t)(ok ? a0 + a : g.Ca - 1);
            const size_t q = ok ? (size_t)(row0 + i) * g.mc + w0 + cc : (size_t)0;
            const float v = Ab[ch * g.Q + q];
            As[a * g.astr + rem] = ok ? v : 0.f;
        }
        for (int idx = tid; idx < CB_FT * frow; idx += 256) {
            const int f = idx / frow, rem = idx - f * frow;
            const int i = rem / g.FL, cc = rem - i * g.FL;
            const int row = row0 + i;
            const int qd = g.nd == 3 ? row / g.mc : 0, qh = g.nd == 3 ? row - qd * g.mc : row;
            const int fd = g.nd == 3 ? qd * g.s - g.p + td : 0;
            const int fh = qh * g.s - g.p + th;
            const int fw = w0 * g.s - g.p + cc;
            const bool ok = f0 + f < g.Cf && i < nr && fd >= 0 && fd < (g.nd == 3 ? g.nf : 1) && fh >= 0 && fh < g.nf && fw >= 0 &&
                            fw < g.nf;
            const size_t ch = (size_t)(ok ? f0 + f : g.Cf - 1);
            const size_t pos = ok ? ((size_t)fd * g.nf + fh) * g.nf + fw : (size_t)0;
            const float v = Fb[ch * g.Pf + pos];
            Fs[f * g.fstr + rem] = ok ? v : 0.f;
        }
        __syncthreads();
        if (wave_on) {
            const float* __restrict__ ar = As + (32 * wave + j) * g.astr;
            const float* __restrict__ fr = Fs + j * g.fstr + tw0;
            for (int i = 0; i < nr; ++i)
                for (int cc = h; cc < g.WLP; cc += 2) {
                    const bool qok = cc < wl;
                    const float av = ar[i * g.WLP + cc];                 // (0 where cc >= wl or the channel is beyond Ca)
                    float bv[NT];
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float v = fr[i * g.FL + cc * g.s + n];
                        bv[n] = (qok && tw0 + n < g.k) ? v : 0.f;
                    }
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[n], acc[n], 0, 0, 0);
                }
        }
    }
    if (!wave_on || f0 + j >= g.Cf) return;
    float* __restrict__ dst = out + (size_t)slice * g.slab;              // (slab 0 when the call has one slab: grad_w itself)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (tw0 + n >= g.k) break;                                       // (wave-uniform)
        const size_t t = (size_t)to * g.k + tw0 + n;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = a0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (a < g.Ca) dst[((size_t)a * g.Cf + f0 + j) * g.T + t] = acc[n][r];
        }
    }
}

// grad_w[i] = sum over samples (ascending, from sample 0's) of (sum over the sample's slabs, ascending, from its slab 0)
__global__ __launch_bounds__(256) void convbwd_finish_kernel(const float* __restrict__ slabs, float* __restrict__ gw, long long total,
                                                             int B, int nsl) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* __restrict__ src = slabs + (size_t)b * nsl * total + i;
        float p = src[0];
        for (int z = 1; z < nsl; ++z) p = p + src[(size_t)z * total];
        acc = b == 0 ? p : acc + p;
    }
    gw[i] = acc;
}

static long long cb_ipow(long long v, int e) {
    long long r = 1;
    for (int i = 0; i < e; ++i) r *= v;
    return r;
}

// per-sample geometry -> tiling, chunking and K slicing; false: the staged tiles do not fit the LDS (a kernel reach of thousands of taps)
bool convbwd_geo(int deconv, int nd, int cin, int cout, int in_size, int out_size, int k, int s, int p, ConvBwdGeo* g) {
    g->nd = nd; g->k = k; g->s = s; g->p = p;
    g->Ca = deconv ? cin : cout;
    g->Cf = deconv ? cout : cin;
    g->mc = deconv ? in_size : out_size;
    g->nf = deconv ? out_size : in_size;
    g->Q = cb_ipow(g->mc, nd);
    g->Pf = cb_ipow(g->nf, nd);
    g->T = (int)cb_ipow(k, nd);
    g->To = (int)cb_ipow(k, nd - 1);
    g->NT = k < 4 ? k : 4;
    g->ntg = (k + g->NT - 1) / g->NT;
    g->nrows = (int)cb_ipow(g->mc, nd - 1);
    for (int run = CB_RUN;; run /= 2) {
        if (run < 2) return false;
        if (g->mc <= run) {
            g->WL = g->mc; g->nseg = 1;
            g->WLP = (g->WL + 1) & ~1;
            g->R = run / g->WLP < 1 ? 1 : run / g->WLP;
            if (g->R > g->nrows) g->R = g->nrows;
        } else {
            g->WL = run; g->WLP = run; g->R = 1;
            g->nseg = (g->mc + run - 1) / run;
        }
        const long long FL = (long long)(g->WLP - 1) * s + (long long)g->ntg * g->NT;
        const long long astr = ((long long)g->R * g->WLP) | 1, fstr = ((long long)g->R * FL) | 1;
        const long long lds = 4 * (CB_AG * astr + CB_FT * fstr);
        if (lds > CB_LDS_MAX) continue;
        g->FL = (int)FL; g->astr = (int)astr; g->fstr = (int)fstr; g->lds_bytes = (int)lds;
        break;
    }
    g->nchunks = g->nseg == 1 ? (g->nrows + g->R - 1) / g->R : g->nrows * g->nseg;
    g->nag = (g->Ca + CB_AG - 1) / CB_AG;
    g->nft = (g->Cf + CB_FT - 1) / CB_FT;
    const long long tiles = (long long)g->nag * g->nft * g->To * g->ntg;
    if (tiles >= (1ll << 24)) return false;
    g->tiles = (int)tiles;
    long long want = (64 + tiles - 1) / tiles;
    if (want > g->nchunks) want = g->nchunks;
    if (want < 1) want = 1;
    g->cps = (int)((g->nchunks + want - 1) / want);
    g->nsl = (g->nchunks + g->cps - 1) / g->cps;
    g->slab = (long long)g->Ca * g->Cf * g->T;
    return true;
}

// [gs: B cout S][chunk sums of g: cout B ceil(S / 512)][slabs: B nsl Ca Cf T when B nsl > 1] — the worst case over the outputs
int64_t conv_backward_scratch_elems(const ConvBwdGeo& g, int B, int cout, int64_t S) {
    const long long nslab = (long long)B * g.nsl;
    return (int64_t)B * cout * S + (int64_t)cout * B * chunks(S) + (nslab > 1 ? nslab * g.slab : 0);
}

// gs (when non-NULL) and grad_shift (when non-NULL; part: cout B ceil(S / 512) floats): the prep pass and the row totals.  A caller with a
// weight-gradient kernel of its own (s3r_stem_bwd.hip) asks for grad_shift alone, scale = gs = NULL
hipError_t launch_convbwd_prep(const float* y, const float* gy, const float* scale, float* gs, float* gshift, int B, int cout, int64_t S,
                               int act, float* part, hipStream_t s, int* launches) {
    const long long nch = chunks(S);
    const long long waves = (long long)B * cout * nch;
    const double Y = (double)B * cout * (double)S;
    {
        AuxScope aux(s, 4.0 * (Y * (act ? 2.0 : 1.0) + (scale ? cout : 0) + (gs ? Y : 0.0) + (gshift ? (double)cout * B * nch : 0.0)));
        hipLaunchKernelGGL(convbwd_prep_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, y, gy, scale, gs,
                           gshift ? part : nullptr, B, cout, (long long)S, nch, act);
    }
    ++*launches;
    if (gshift) {
        AuxScope aux(s, 4.0 * ((double)cout * B * nch + cout));
        hipLaunchKernelGGL(convbwd_shift_finish_kernel, dim3((unsigned)cout), dim3(64), 0, s, part, gshift, B, nch);
        ++*launches;
    }
    return hipGetLastError();
}

hipError_t launch_conv_backward(const ConvBwdGeo& g, int deconv, const float* x, const float* y, const float* gy, const float* scale,
                                float* gs, float* gw, float* gshift, int B, int cout, int64_t S, int act, float* scratch, hipStream_t s,
                                int* launches) {
    *launches = 0;
    const long long nch = chunks(S);
    float* gs_buf = scratch;
    float* part = scratch + (size_t)B * cout * S;
    float* slabs = part + (size_t)cout * B * nch;
    const float* gsr = gs;                                               // what the GEMM reads as gs
    const bool plain = act == 0 && !scale;                               // gs == grad_y, bit for bit
    float* gs_out = gs;
    if (!gs && gw) {
        if (plain) gsr = gy;
        else gs_out = gs_buf, gsr = gs_buf;
    }
    if (gs_out || gshift) {
        hipError_t e = launch_convbwd_prep(y, gy, scale, gs_out, gshift, B, cout, S, act, part, s, launches);
        if (e != hipSuccess) return e;
    }
    if (gw) {
        const float* A = deconv ? x : gsr;
        const float* F = deconv ? gsr : x;
        const long long nslab = (long long)B * g.nsl;
        float* dst = nslab > 1 ? slabs : gw;
        const dim3 grid((unsigned)(nslab * g.tiles));
#define S3R_CB_LAUNCH(NT) hipLaunchKernelGGL((convbwd_gw_kernel<NT>), grid, dim3(256), (size_t)g.lds_bytes, s, A, F, dst, g)
        switch (g.NT) {
            case 1: S3R_CB_LAUNCH(1); break;
            case 2: S3R_CB_LAUNCH(2); break;
            case 3: S3R_CB_LAUNCH(3); break;
            default: S3R_CB_LAUNCH(4); break;
        }
#undef S3R_CB_LAUNCH
        ++*launches;
        if (nslab > 1) {
            AuxScope aux(s, 4.0 * (double)g.slab * ((double)nslab + 1.0));
            hipLaunchKernelGGL(convbwd_finish_kernel, dim3((unsigned)((g.slab + 255) / 256)), dim3(256), 0, s, slabs, gw, g.slab, B, g.nsl);
            ++*launches;
        }
    }
    return hipGetLastError();
}

}  // namespace s3r
