// Backward of the point-head linear layer  y = act(x W^T + bias)  (s3r_linear_backward): x (B,Cin), W (Cout,Cin) in torch layout,
// y and grad_y (B,Cout), act none / ReLU / sigmoid.  Three results, each optional, each with a FIXED summation order — no atomics,
// the same bits on every run and at every 4-byte-aligned address (every access below is one dword per lane: nothing depends on
// a wider alignment, so there is no second code path an address could select):
//
//   g (B,Cout), the pre-activation gradient, fp32, nothing fused (contraction off): act_grad (s3r_ordered.h)
//   grad_bias[o] = sum_b g[b][o]          one accumulator that starts as g[0][o], plain adds in ascending b   (linbwd_prep_kernel)
//   grad_w[o][i] = sum_b g[b][o] x[b][i]  a GEMM with M = Cout, N = Cin, K = B                                 (linbwd_gw_kernel)
//   grad_x[b][i] = sum_o g[b][o] w[o][i]  a GEMM with M = B, N = Cin, K = Cout                                 (linbwd_gx_kernel)
//
// linbwd_prep_kernel: one thread per output column o walks b in ascending order: it applies the activation rule, stores g into
//   scratch (ReLU / sigmoid only, and only when grad_w or grad_x is asked for: with act none the GEMMs read grad_y itself) and keeps the bias sum.  Lanes are consecutive in o, so
//   every load and store is a whole 128-byte line per 32 lanes.  It is skipped when act is none and grad_bias is not asked for.
//
// linbwd_gw_kernel: v_mfma_f32_32x32x2_f32, A = g (lane (r, h): g[2t + h][o0 + r]), B = x (lane (j, h): x[2t + h][i0 + j]).  Both
//   operands are K-major in memory, so a fragment is one coalesced dword load per lane (128 bytes per 32 lanes) and needs no LDS.
//   A wave owns 32 output rows x 128 columns (four accumulator tiles that share the A fragment) and walks the WHOLE batch in
//   ascending b, 16 rows per block of loads (8 + 32 loads in flight per lane): no split-K, no scratch.  The four waves of a workgroup
//   own four consecutive 32-row tiles over the same 128 columns, so the x block they share is fetched from HBM once.  The kernel is
//   write-bound (p1: 134 MB): accumulator register r of a tile holds row o0 + (r & 3) + 8 (r >> 2) + 4 h at column i0 + j, so ONE
//   store instruction writes two whole 128-byte row segments (lanes 0..31 one row, lanes 32..63 another), with the default cache
//   policy: MI355X_MICROARCH.md's table of store flavours has every byte leave L2 once under plain and nt alike and prices nt
//   on data somebody reads next (nt-handoff) as a loss — the optimizer reads grad_w next.
//
// linbwd_gx_kernel: A = g staged through LDS (g is tiny, but its fragment — 32 batch rows at one o — is strided in memory):
//   a workgroup stages 32 batch rows x 128 o as gs[o][row] (padded to 33: conflict-free both ways), B = w (lane (j, h):
//   w[2t + h][i0 + j], coalesced).  A workgroup's four waves own four consecutive 32-column tiles of one K slice; K runs in ascending
//   o inside a slice.  N = Cin alone gives too few tiles for the layers behind p1 (p3: 32 column tiles, K = 6144), so K is split over
//   workgroups into `ksplit` slices of whole 128-o chunks; slice kz writes slab [kz][b][i] into scratch and linbwd_finish_kernel adds
//   the slabs in ascending kz starting from slab 0 (as linear_finish_kernel does).  The split is a function of (Cin, Cout) ONLY
//   (linbwd_split: about 2048 waves over the column tiles) — never of the batch, the device or an address — so the scratch query
//   is monotone in the batch.  ksplit == 1 writes grad_x directly.
//
// Which shapes take which path: every positive (B, Cin, Cout) runs these same kernels.  Rows / columns / k beyond the tensor are
// loaded from a clamped address and replaced by 0 in BOTH operands (0 * NaN would be NaN), and never stored; a K tail adds +0.0
// products to an accumulator that started as +0.0, which changes no bit: under round-to-nearest a sum is -0.0 only when BOTH addends
// are -0.0, so an accumulator that starts as +0.0 never holds -0.0 and acc + (+0.0) == acc bit for bit.  All indexing is 64-bit element arithmetic on plain
// pointers; the grids are one-dimensional (no 65535 limit on a tile count).
#include "s3r_ordered.h"

namespace s3r {

typedef float f32x16_b __attribute__((ext_vector_type(16)));

// one thread per o; b ascending; g stored when gbuf != NULL, the bias sum when gbias != NULL.  y is NULL when act is none
__global__ __launch_bounds__(64) void linbwd_prep_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                         float* __restrict__ gbuf, float* __restrict__ gbias, int B, int Cout,
                                                         int act) {
#pragma clang fp contract(off)
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o >= Cout) return;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= B; b += 8) {                    // eight rows' loads in flight, then the adds in order
        float v[8], yy[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t at = (size_t)(b + u) * Cout + o;
            v[u] = gy[at];
            yy[u] = act ? y[at] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float g = act_grad(yy[u], v[u], act);
            if (gbuf) gbuf[(size_t)(b + u) * Cout + o] = g;
            s = (b + u == 0) ? g : s + g;
        }
    }
    for (; b < B; ++b) {
        const size_t at = (size_t)b * Cout + o;
        const float g = act_grad(act ? y[at] : 0.f, gy[at], act);
        if (gbuf) gbuf[at] = g;
        s = (b == 0) ? g : s + g;
    }
    if (gbias) gbias[o] = s;
}

constexpr int GW_NT = 4;        // 32-column accumulator tiles per wave (share one A fragment)
constexpr int GW_KB = 8;        // k-steps (of two batch rows) per block of loads

__global__ __launch_bounds__(256) void linbwd_gw_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                        float* __restrict__ gw, int B, int Cin, int Cout, int nog) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const long long og = blockIdx.x % nog, ig = blockIdx.x / nog;        // row groups fastest: neighbours share the x block
    const long long o0 = (og * 4 + wave) * 32, i0 = ig * (32 * GW_NT);
    if (o0 >= Cout) return;                                              // (wave-uniform; the kernel has no barrier)
    const bool ov = o0 + j < Cout;
    const size_t oc = (size_t)(ov ? o0 + j : Cout - 1);
    bool iv[GW_NT];
    size_t ic[GW_NT];
#pragma unroll
    for (int n = 0; n < GW_NT; ++n) {
        iv[n] = i0 + 32 * n + j < Cin;
        ic[n] = (size_t)(iv[n] ? i0 + 32 * n + j : Cin - 1);
    }
    f32x16_b acc[GW_NT];
#pragma unroll
    for (int n = 0; n < GW_NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    for (int b0 = 0; b0 < B; b0 += 2 * GW_KB) {
        float a[GW_KB], xv[GW_NT][GW_KB];
#pragma unroll
        for (int u = 0; u < GW_KB; ++u) {
            const int b = b0 + 2 * u + h;
            const bool bv = b < B;
            const size_t bc = (size_t)(bv ? b : B - 1);
            const float av = g[bc * Cout + oc];
            a[u] = (bv && ov) ? av : 0.f;
#pragma unroll
            for (int n = 0; n < GW_NT; ++n) {
                const float v = x[bc * Cin + ic[n]];
                xv[n][u] = (bv && iv[n]) ? v : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < GW_KB; ++u)
#pragma unroll
            for (int n = 0; n < GW_NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], xv[n][u], acc[n], 0, 0, 0);
    }
#pragma unroll
    for (int n = 0; n < GW_NT; ++n) {
        if (i0 + 32 * n >= Cin) break;                                   // (wave-uniform)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long o = o0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (o < Cout && iv[n]) gw[(size_t)o * Cin + (size_t)(i0 + 32 * n + j)] = acc[n][r];
        }
    }
}

constexpr int GX_KC = 128;      // o per staged chunk (64 k-steps); K slices are whole chunks
constexpr int GX_KB = 16;       // k-steps per block of loads

__global__ __launch_bounds__(256) void linbwd_gx_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                        float* __restrict__ out, int B, int Cin, int Cout, int kper, int nig,
                                                        int ksplit) {
    __shared__ float gs[GX_KC][33];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const long long ig = blockIdx.x % nig, rest = blockIdx.x / nig;
    const int kz = (int)(rest % ksplit);
    const long long b0 = (rest / ksplit) * 32;
    const long long col = (ig * 4 + wave) * 32 + j;
    const bool cv = col < Cin;
    const size_t cc = (size_t)(cv ? col : Cin - 1);
    const int kbeg = kz * kper, kend = min(Cout, kbeg + kper);
    f32x16_b acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += GX_KC) {
        if (k0 != kbeg) __syncthreads();                                 // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < (32 * GX_KC) / 256; ++e) {
            const int idx = threadIdx.x + 256 * e;
            const int r = idx / GX_KC, c = idx % GX_KC;                  // consecutive threads: consecutive o of one batch row
            const bool ok = k0 + c < kend && b0 + r < B;
            const float v = g[(size_t)(ok ? b0 + r : B - 1) * Cout + (size_t)(ok ? k0 + c : Cout - 1)];
            gs[c][r] = ok ? v : 0.f;
        }
        __syncthreads();
        for (int t0 = 0; t0 < GX_KC / 2 && k0 + 2 * t0 < kend; t0 += GX_KB) {
            float wv[GX_KB], av[GX_KB];
#pragma unroll
            for (int u = 0; u < GX_KB; ++u) {
                const int o = k0 + 2 * (t0 + u) + h;
                const bool ok = o < kend && cv;
                const float v = w[(size_t)(o < kend ? o : Cout - 1) * Cin + cc];
                wv[u] = ok ? v : 0.f;
                av[u] = gs[2 * (t0 + u) + h][j];                         // lane j: batch row b0 + j (0 where o >= kend or the row is beyond B)
            }
#pragma unroll
            for (int u = 0; u < GX_KB; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], wv[u], acc, 0, 0, 0);
        }
    }
    if (!cv) return;
    float* __restrict__ dst = out + (ksplit > 1 ? (size_t)kz * B * Cin : (size_t)0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long b = b0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (b < B) dst[(size_t)b * Cin + (size_t)col] = acc[r];
    }
}

// grad_x = slab 0 + slab 1 + ... in ascending slice order, eight loads in flight per thread
__global__ __launch_bounds__(256) void linbwd_finish_kernel(const float* __restrict__ part, float* __restrict__ gx, long long total,
                                                            int ksplit) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float s = part[i];
    int z = 1;
    for (; z + 8 <= ksplit; z += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = part[(size_t)(z + u) * total + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; z < ksplit; ++z) s += part[(size_t)z * total + i];
    gx[i] = s;
}

// K split of grad_x: slices of whole 128-o chunks, about 2048 waves over the ceil(Cin / 32) column tiles; (Cin, Cout) only
static void linbwd_split(int Cin, int Cout, int* ksplit, int* kper) {
    const long long itiles = ((long long)Cin + 31) / 32;
    const long long chunks = ((long long)Cout + GX_KC - 1) / GX_KC;
    long long want = (2048 + itiles - 1) / itiles;
    if (want > chunks) want = chunks;
    if (want < 1) want = 1;
    const long long per = (chunks + want - 1) / want;                    // chunks per slice
    *kper = (int)(per * GX_KC);
    *ksplit = (int)((chunks + per - 1) / per);
}

// [g: B Cout][slabs: ksplit B Cin when ksplit > 1] — the worst case over the outputs a call may ask for
int64_t linear_backward_scratch_elems(int B, int Cin, int Cout) {
    int ks, kper;
    linbwd_split(Cin, Cout, &ks, &kper);
    return (int64_t)B * Cout + (ks > 1 ? (int64_t)ks * B * Cin : 0);
}

hipError_t launch_linear_backward(const float* x, const float* w, const float* y, const float* gy, float* gx, float* gw, float* gb,
                                  int B, int Cin, int Cout, int act, float* scratch, hipStream_t s, int* launches) {
    *launches = 0;
    const float* g = gy;
    if (act || gb) {
        float* gbuf = (act && (gw || gx)) ? scratch : nullptr;          // g is stored only when a GEMM will read it
        hipLaunchKernelGGL(linbwd_prep_kernel, dim3((unsigned)(((long long)Cout + 63) / 64)), dim3(64), 0, s, y, gy, gbuf, gb, B, Cout,
                           act);
        if (act) g = gbuf;
        ++*launches;
    }
    if (gw) {
        const long long nog = ((long long)Cout + 127) / 128, nig = ((long long)Cin + 32 * GW_NT - 1) / (32 * GW_NT);
        hipLaunchKernelGGL(linbwd_gw_kernel, dim3((unsigned)(nog * nig)), dim3(256), 0, s, g, x, gw, B, Cin, Cout, (int)nog);
        ++*launches;
    }
    if (gx) {
        int ks, kper;
        linbwd_split(Cin, Cout, &ks, &kper);
        float* slabs = scratch + (size_t)B * Cout;
        const long long nig = ((long long)Cin + 127) / 128, nbt = ((long long)B + 31) / 32;
        hipLaunchKernelGGL(linbwd_gx_kernel, dim3((unsigned)(nig * ks * nbt)), dim3(256), 0, s, g, w, ks > 1 ? slabs : gx, B, Cin,
                           Cout, kper, (int)nig, ks);
        ++*launches;
        if (ks > 1) {
            const long long total = (long long)B * Cin;
            hipLaunchKernelGGL(linbwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, slabs, gx, total, ks);
            ++*launches;
        }
    }
    return hipGetLastError();
}

}  // namespace s3r
