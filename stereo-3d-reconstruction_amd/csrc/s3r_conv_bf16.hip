// bf16 MFMA path, the dispatch unit (s3r_bf16.h has the path's essay and the map of its units): which instruction shape, tile and
// split-K a layer gets, the split-K scratch size, launch_conv_bf16 over the two gather units' launchers, and the two kernels
// that belong to no gather: the split-K finish and the weight pack.
#include "s3r_bf16.h"
#include <cstdlib>

#ifndef S3R_BF16_MFMA_DEFAULT
#define S3R_BF16_MFMA_DEFAULT 32      // the matrix instruction used when S3R_BF16_MFMA is not set (see conv_bf16_shape)
#endif

namespace s3r {

#ifdef S3R_ABLATE   // diagnostic builds only: S3R_ABL=1 no epilogue stores, 2 one K tile only, 3 no DMA in the loop, 7 timeline
static int abl_mode_h() { static const int m = getenv("S3R_ABL") ? atoi(getenv("S3R_ABL")) : 0; return m; }
static int timeline_family = BF16_TAP;      // the family launch_conv_bf16 launched last: whose buffer s3r_debug_read_timeline_h reads
#endif

// which instruction the library uses: S3R_BF16_MFMA = 16 | 32 (read per call: the A/B tools flip it in-process;
// the weights must be packed under the same value — the Python module keys its pack cache on it)
int conv_bf16_shape() {
    const char* e = getenv("S3R_BF16_MFMA");
    if (e && atoi(e) == 16) return 16;
    if (e && atoi(e) == 32) return 32;
    return S3R_BF16_MFMA_DEFAULT;
}

// split-K finish: y[pos][cout] = bf16(act(scale * sum_kz slab + shift)); one thread per (position, cout pair)
__global__ __launch_bounds__(256) void conv_finish_bf16_kernel(const ConvParamsH p, int mpad) {
    const int S = p.Nd * p.Nh * p.Nw;
    const int cls = blockIdx.y;                       // (this kernel's own grid: y = output parity class)
    const int rd = (cls >> 2) & 1, rh = (cls >> 1) & 1, rw = cls & 1;
    const int half = p.CoutPad >> 1;
    const long long total = (long long)p.Ntotal * half;
    unsigned short* __restrict__ y = reinterpret_cast<unsigned short*>(p.y);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / half);
        const int co = (int)(i - (long long)n * half) * 2;
        if (co >= p.Cout) continue;
        const float* __restrict__ src = p.part + ((size_t)cls * p.ksplit * mpad + n) * p.CoutPad + co;
        float2 s = *reinterpret_cast<const float2*>(src);
        for (int z = 1; z < p.ksplit; ++z) {
            const float2 t = *reinterpret_cast<const float2*>(src + (size_t)z * mpad * p.CoutPad);
            s.x += t.x; s.y += t.y;
        }
        const auto [b, pd, ph, pw] = decode_pos(p, n, S);
        const int ye = out_offset(p, b, pd, ph, pw, rd, rh, rw);
        const bool c1 = co + 1 < p.Cout;
        float v0 = fmaf(s.x, p.scale ? p.scale[co] : 1.f, p.shift ? p.shift[co] : 0.f);
        float v1 = c1 ? fmaf(s.y, p.scale ? p.scale[co + 1] : 1.f, p.shift ? p.shift[co + 1] : 0.f) : 0.f;
        if (p.act == ACT_RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
        else if (p.act == ACT_SIGMOID) { v0 = 1.f / (1.f + __expf(-v0)); v1 = 1.f / (1.f + __expf(-v1)); }
        const unsigned pk = pack_bf16(v0, v1);
        if (c1) *reinterpret_cast<unsigned*>(y + (size_t)ye + co) = pk;
        else y[(size_t)ye + co] = (unsigned short)(pk & 0xffffu);
    }
}

hipError_t launch_finish_bf16(const ConvParamsH& p, int bm, hipStream_t stream) {
    if (p.ksplit <= 1) return hipSuccess;
    const long long total = (long long)p.Ntotal * (p.CoutPad >> 1);
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(conv_finish_bf16_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), p.transposed ? 8 : 1),
                       dim3(256), 0, stream, p, p.m_tiles * bm);
    return hipGetLastError();
}

// Tile / gather choice (tools/layer_bench.py --dtype bf16, B = 256, MI355X):
//   * stride-1 layers with 4+ taps per plane and K >= 256 whose 256-position plane image leaves room for THREE
//     workgroups per CU (e2, e4, e6, e7, v1, v3, v5, d1, d2, d3) run the plane-reuse gather with 32-channel K tiles (code 22): 5-25 %
//     faster than the per-tap / row-reuse kernels, and 2-7 % faster than its own 64-channel form (code 6, two
//     workgroups per CU): overlapping one workgroup's image reload and stores with the others' MFMAs is worth
//     more than whole-line gathers once the image is fetched only once per kh*kw taps;
//   * everything else (stride 2, shallow K, v6's 16-position planes) runs the per-tap kernel with 128-position
//     tiles — more workgroups per CU to overlap loads and stores, 64-channel K tiles wherever Cin % 64 == 0 — and
//     128-cout workgroup tiles (code 3) where Cout % 128 == 0: these layers are bound by L2 -> LDS delivery;
//   * the row-reuse gather (codes 9 / 10) remains for deep stride-1 layers with an odd number of 64-cout tiles.
int conv_bf16_pick_tm(const ConvParamsH& p) {
    const long classes = (p.transposed ? 8 : 1) * (long)p.ksplit;
    const long n_tiles = p.CoutPad / HBN;
    auto wgs = [&](int tm) { return ((p.Ntotal + 128 * tm - 1) / (128 * tm)) * n_tiles * classes; };
    // The K summation order of a layer must not depend on the batch (a sample's result is batch-invariant): the
    // plane / row-reuse kernels and the 32-channel per-tap kernel accumulate chunk32-major, the 64-channel per-tap
    // kernel chunk64-major.  So the FAMILY is chosen from per-sample geometry, only the tile from the batch.
    const int pr = plane_rows(p, 256, 32);
    const bool plane_family = pr > 0 && pr <= 576 && (p.Cin / 32) % p.ksplit == 0 && p.kh * p.kw >= 4 &&
                              (long)p.Cin * p.T >= 256;      // (e2, K = 288: -12 % once its planes tile exactly)
    // (transposed classes have only 4 taps per image: its 256 x 128-cout form, code 23, amortises the image over twice
    //  the couts — d1 -10 %, d2 -6 %; the 9-tap layers are level or slower with it)
    if (plane_family && rows_strips(p)) return 40;           // (same K order as the plane kernel: a per-batch choice)
    if (plane_family && wgs(2) >= 512) return (p.transposed && n_tiles % 2 == 0 && wgs(2) / 2 >= 512) ? 23 : 22;
    // row-reuse (32-channel K order, like the plane kernel): small batches of deep plane-family layers (v5 at B = 32)
    const bool deep = !p.transposed && p.kw >= 3 && (long)p.Cin * p.T >= 64 * 27;
    const bool reuse = p.stride == 1 && deep && rowreuse_rows(p, 128) <= 64 * NPA_MAX;
    if (plane_family) return reuse ? 9 : 17;
    // the per-tap family (64-channel K tiles where Cin allows): 128 x 128-cout tiles when the channel axis has an even
    // number of 64-cout tiles and the grid stays full (e5 -9 %, v2 -14 %, v4 -11 %, v6 -21 % vs the row-reuse gather)
    if (n_tiles % 2 == 0 && !p.head_w) return wgs(1) / 2 >= 1024 ? 3 : 1;
    // pointwise layers (e8: 1 x 1, 256 -> 32): 32-channel K tiles — with one tap the channels are walked in the same order
    // either way (bit-identical), and the half-size tiles leave room for more workgroups per CU: 0.045 -> 0.040 ms
    if (p.T == 1 && !p.head_w) return 17;
    if (reuse) return (wgs(2) >= 1024 && p.Nw >= 7 && rowreuse_rows(p, 256) <= 64 * NPA_MAX) ? 10 : 9;
    return 1;
}

int conv_bf16_pick_ksplit(const ConvParamsH& p) {
    // per-sample geometry at a nominal batch (batch-invariant, as in the fp32 path); 128 here: this path's
    // named configuration is batch 256, where splitting v5 / v6 / d1 further costs 15-30 % of their time
    const int chunks = p.Cin / HKC;
    const long S = (long)p.Nd * p.Nh * p.Nw;
    const long wg_nom = ((128 * S + 127) / 128) * (p.CoutPad / HBN) * (p.transposed ? 8 : 1);
    int ks = 1;
    while (wg_nom * ks < 1024 && chunks % (2 * ks) == 0 && (chunks / (2 * ks)) * p.T >= 64) ks *= 2;
    return ks;
}

int64_t conv_bf16_scratch_elems(const ConvParamsH& p, int tm) {
    if (p.ksplit <= 1) return 0;
    const Bf16Tile* t = bf16_tile(tm);
    if (!t) return 0;                            // (both callers come through resolve_launch_h, which lets no other code by)
    // the row-persistent kernel never splits K (launch_rows refuses); a forced 40 with a forced split keeps the size it always had
    const int bm = t->family == BF16_ROWS ? 2560 : 128 * t->tm;
    const int64_t mpad = (int64_t)((p.Ntotal + bm - 1) / bm) * bm;
    return (int64_t)(p.transposed ? 8 : 1) * p.ksplit * mpad * p.CoutPad;
}

static hipError_t launch_shape(int sh, const ConvParamsH& p, int tm, hipStream_t stream) {
    const Bf16Tile* t = bf16_tile(tm);
    if (!t) return hipErrorInvalidValue;
#ifdef S3R_ABLATE
    timeline_family = t->family;
#endif
    const bool tap_unit = t->family == BF16_TAP || t->family == BF16_ROWREUSE;
    return tap_unit ? launch_bf16_tap(sh, *t, p, stream) : launch_bf16_plane(sh, *t, p, stream);
}

hipError_t launch_conv_bf16(const ConvParamsH& pin, int tm, hipStream_t stream) {
    ConvParamsH p = pin;
#ifdef S3R_ABLATE
    p.debug = abl_mode_h();
#endif
    if (p.Cin % HKC != 0 || p.CoutPad % HBN != 0 || p.ksplit < 1 || (p.Cin / HKC) % p.ksplit != 0 ||
        (p.ksplit > 1 && !p.part))
        return hipErrorInvalidValue;
    return launch_shape(conv_bf16_shape(), p, tm, stream);
}

// ------------------------------------------------------------------------------------------------
// weight packing for the bf16 kernels (fp32 torch layout -> bf16, K-tile major, pre-swizzled):
//   wp[cls][kt = chunk*T + tap][cout tile][row 0..63][slot][8]   (64 B per row)
//     slot holds channel group kg = slot ^ swz<32>(row),  cin = chunk*32 + kg*8 + e
//     row -> cout of the 64-cout tile, so that the couts a lane ends up holding are consecutive (epilogue_h):
//       SH = 32: row = tn*32 + c; MFMA output row c sits in lane half h = (c>>2)&1, register r = (c&3) + 4*(c>>3):
//                cout = tn*32 + 16*h + r
//       SH = 16: row = ct*16 + i; MFMA output row i sits in lane group g = i>>2, register r = i&3:
//                cout = 16*g + 4*ct + r
__global__ void pack_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int Cin, int Cout,
                                 int CoutPad, int T, int transposed, int sh) {
    const size_t per_cls = (size_t)T * Cin * CoutPad;
    const size_t total = (transposed ? 8 : 1) * per_cls;
    const int n_tiles = CoutPad / 64;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cls = (int)(i / per_cls);
        size_t r = i % per_cls;
        const int e = (int)(r & 7); r >>= 3;
        const int slot = (int)(r & 3); r >>= 2;
        const int row = (int)(r & 63); r >>= 6;
        const int tile = (int)(r % n_tiles); r /= n_tiles;
        const int tap = (int)(r % T);
        const int cc = (int)(r / T);
        int co;
        if (sh == 32) {
            const int tn = row >> 5, c = row & 31;
            co = tile * 64 + tn * 32 + 16 * ((c >> 2) & 1) + (c & 3) + 4 * (c >> 3);
        } else {
            const int ct = row >> 4, ii = row & 15;
            co = tile * 64 + 16 * (ii >> 2) + 4 * ct + (ii & 3);
        }
        const int kg = slot ^ swz<32>(row);
        const int cin = cc * 32 + kg * 8 + e;
        float v = 0.f;
        if (co < Cout) {
            if (!transposed) {
                v = w[((size_t)co * Cin + cin) * T + tap];
            } else {
                const int rd = (cls >> 2) & 1, rh = (cls >> 1) & 1, rw = cls & 1;
                const int td = (tap >> 2) & 1, th = (tap >> 1) & 1, tw = tap & 1;
                const int kd = 3 - rd - 2 * td, kh = 3 - rh - 2 * th, kw = 3 - rw - 2 * tw;
                v = w[((size_t)cin * Cout + co) * 64 + (kd * 4 + kh) * 4 + kw];
            }
        }
        wp[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
    }
}

hipError_t launch_pack_bf16(const float* w, void* wp, int Cin, int Cout, int CoutPad, int T, int transposed,
                            hipStream_t s) {
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(1024), dim3(256), 0, s, w, reinterpret_cast<unsigned short*>(wp), Cin, Cout,
                       CoutPad, T, transposed, conv_bf16_shape());
    return hipGetLastError();
}

}  // namespace s3r

#ifdef S3R_ABLATE
extern "C" int s3r_debug_read_timeline_h(unsigned long long* out, int nblocks) {
    if (nblocks > 65536) nblocks = 65536;
    return s3r::timeline_family == s3r::BF16_PLANE ? s3r::read_timeline_plane(out, nblocks) : s3r::read_timeline_tap(out, nblocks);
}
#endif
