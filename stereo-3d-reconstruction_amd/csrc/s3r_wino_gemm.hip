// The class GEMM of the Winograd forms (s3r_wino.h has the map and the transforms) and everything that launches it: wino_body, the
// kernels around it, the one-axis finish pass, wino_plan and the launchers.  Every wino_kernel<..> is instantiated HERE, so one
// code object holds them all; the two-axis launcher (s3r_wino_axis2.hip) reaches its six through launch_wino2_classes.
#include "s3r_wino.h"
#include "s3r_cv_live.h"
#include <cstdlib>
#include <type_traits>

namespace s3r {

int wino_bk() { return WBK; }

#ifdef S3R_ABLATE
// S3R_ABL=7: per-workgroup timeline stamps (s_memrealtime, 100 MHz) of the class kernels, tools/timeline.py --wino:
// [cu key, start, loop start, loop end, end, stores issued]
__device__ unsigned long long s3r_wino_timeline[6 * 65536];
#endif

// ================================================================================================
// The class kernels.  ONE body serves the Winograd forms,
//     KIND 1: convolution, F(4,3) along H (6 classes, 4 output rows per group)
//     KIND 2: ConvTranspose3d(k4 s2 p1), F(2,2) along D and H inside every output-parity class (9 classes, 2 x 2 outputs)
// in two launch forms:
//     serial (CP = false): a workgroup owns a tile of 64 couts x BN positions (position = one group of R output rows of one
//         column) and walks ALL classes back to back, one accumulator set per class; the output transform, the folded BN +
//         ReLU (and d3's fused 1 x 1 x 1 head) run on the registers.  4 waves as WM x WN = 2 x 2 (32 couts x 32 positions per
//         wave, BN = 64: one MFMA tile per class — 109 registers for six classes, four workgroups per CU; r03's 64 x 128 tiles
//         held two and measured 3-13 % slower on every layer).  The fused head adds the two waves' 32-cout sums through LDS;
//     class-parallel (CP = true): a workgroup owns ONE class of a tile, runs that class's K loop — the same MFMA sequence in the
//         same order as the serial form, so the same bits — and writes the raw class sums to a slab part[class][cout][n];
//         wino_finish_kernel then applies the output transform and the epilogue through the SAME device functions
//         (wino_out / wino_act, s3r_wino.h) in the same operation order: bit-identical to the serial form.  It multiplies the
//         workgroup count by the class count (x 6 / x 9) and divides a workgroup's serial K walk by it: the form for
//         grids that leave the chip short of workgroups (small batches; v5; d1) and for the REMAINDER of a launch whose
//         workgroup count is a little over a multiple of the chip's slots (wino_dual_kernel: bulk serial + remainder
//         class-parallel in one launch — the direct path's plan_tail_cut idea with the class axis as the finer unit).
// Because the two forms agree bit for bit, which one runs may depend on the batch size (a sample's bits never do).
//
// p (convolution): the CLASS convolution — p.x = V, x_cs / x_ds / x_hs its strides (x_hs = one V row per group), p.x_cls the class
//   stride, Nh = groups per plane, T = kd * kw, x_org = 0; p.y the layer's padded output, p.Hout its true height (the last group's
//   missing rows are not stored).
// p (transposed): the layer's own parameters (make_params) with Nd = depth pairs, Nh = row pairs (n / 2), p.x = the padded input,
//   p.xd = its row differences Dh (x's shape and strides; p.xd_mode = 1: followed by Dd and Ddh), p.w = the 72 (parity class, class) slabs.
// p.part: class-parallel slabs [class][Cout][npad], npad = the position range's tile count x BN.
// XM (transposed form): the depth differences are materialised (p.xd = [Dh | Dd | Ddh]) instead of formed here
// SEMI (two-axis convolution, below): the workgroup owns ONE depth class a of its tile and walks that class's six row classes
// serially (plane sets / weight slabs 6 a .. 6 a + 5); the row transform runs on the registers and the four row outputs go,
// raw, to the slab part[a][row][cout][n] for wino2s_finish_kernel to transform along D
// CVL (two-axis convolution whose input is the cost volume's plane sets, p.cv_n > 0): p is launch_conv_wino2's re-aimed view — Nd = 1,
// Nh = depth groups, Nw = the n * n / 4 positions of one, the three column taps as "depth" taps x_ds = n / 4 apart — and the K walk
// leaves out the (chunk, tap) tiles that read structural zeros only (s3r_cv_live.h): one mask per workgroup, so the ring, the
// counted vmcnt and the barriers see a shorter class and nothing else.  The tiles left out added w * (+0) to a finite sum: same bits
template <int VEC, int KIND, int WN, bool CP, bool HEAD, bool XM = false, bool SEMI = false, bool CVL = false>
__device__ __forceinline__ void wino_body(const ConvParams& p, const int bid_in, const int nwg_in, const int n_begin,
                                          const int n_end, float* __restrict__ wsmem) {
    constexpr bool DECONV = KIND == 2;
    constexpr int NCLS = WinoKind<KIND>::NCLS, R = WinoKind<KIND>::R;
    constexpr int WM = 4 / WN, TM = 2 / WM, BN = 32 * WN;
    constexpr int NACC = CP ? 1 : NCLS;
    static_assert(KIND == 1 || KIND == 2, "F(4,3) convolution or F(2,2) transposed convolution");
    static_assert(!SEMI || (KIND == 1 && !CP && !HEAD), "the semi-fused form: serial F(4,3) row classes of one depth class");
    static_assert(WN == 4 || WN == 2, "4 waves as 1 x 4 or 2 x 2");
    static_assert(!HEAD || (DECONV && !CP && WN == 2), "the fused head: serial transposed form");
    static_assert(!CVL || (KIND == 1 && (CP || SEMI)), "live K tiles: the two-axis forms of the cost volume's consumer");
    float* As = wsmem;                                   // [WNB][WBK][64]
    constexpr int BSTG = (DECONV ? 2 : 1) * WBK * BN;    // B floats per stage (transposed: depths z and z + 1 side by side)
    float* Bs = wsmem + WNB * WBK * WBM;                 // [WNB][BSTG]
    constexpr int PB = 64 * VEC;                         // floats per B piece
    constexpr int NPIECE_B = WBK * BN / PB;
    static_assert(NPIECE_B % 4 == 0, "B pieces divide over the 4 waves");
    constexpr int NPB = NPIECE_B / 4;
    constexpr bool B_WIDE = BN >= PB;
    constexpr int PPR = B_WIDE ? BN / PB : 1;
    constexpr int RPP = B_WIDE ? 1 : PB / BN;
    constexpr int LPR_B = BN / VEC;
    constexpr int NPD = WNPA + NPB;                      // DMAs per wave per K tile (WNPA 1 KiB weight pieces + NPB gathers)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int j = lane & 31, h = lane >> 5;
#ifdef S3R_ABLATE
    unsigned long long tl0 = 0, tl1 = 0, tl2 = 0;
    if (p.debug == 7) tl0 = __builtin_amdgcn_s_memrealtime();
#endif

    const int n_tiles = (n_end - n_begin + BN - 1) / BN;
    int bid = bid_in, cls0 = 0, pc = 0;                  // cls0: the one class of a class-parallel workgroup; pc: output parity class
    if constexpr (CP || SEMI) {
        // an XCD walks a contiguous run of items, class-major: neighbouring workgroups share a class's weight slab (and the
        // transformed rows their tiles have in common) in that XCD's L2
        const int nwg = nwg_in;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
        const int item = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
        const int ntile = p.m_tiles * n_tiles;
        const int c = item / ntile;
        bid = item - c * ntile;
        if constexpr (DECONV) { pc = c / NCLS; cls0 = c - pc * NCLS; } else cls0 = SEMI ? c * NCLS : c;
    } else if constexpr (DECONV) {
        // an XCD walks its run of tiles with the 8 parity classes of a tile back to back (they read the same input tile)
        const int nwg = nwg_in >> 3;
        const int item = (bid & 7) * nwg + (bid >> 3);
        bid = item >> 3;
        pc = item & 7;
    } else {
        const int nwg = nwg_in;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    const int rd = (pc >> 2) & 1, rh = (pc >> 1) & 1, rw = pc & 1;
    const int m_tile = bid % p.m_tiles, n_tile = bid / p.m_tiles;
    const int m0 = m_tile * WBM, n0 = n_begin + n_tile * BN;
    const int S = p.Nd * p.Nh * p.Nw;
    const int T = DECONV ? 2 : p.T;                      // taps per class: (depth tap,) column tap
    const int chunks = p.Cin / WBK;
    const int nkt = T * chunks;                          // K tiles per class
    int nrun = nkt;                                      // ... that a class walks
    unsigned live = 0;                                   // (CVL) bit chunk * 3 + tap: the K tile is live; the same for every class
    if constexpr (CVL) {                                 // (the launcher keeps nkt <= 32)
        // the tile's first and last position as (sample, depth group) g and column: Nw positions per g, Nh row groups per column (and
        // Nh depth groups per sample), through the launch's fast divisions
        const int last = (n0 + BN < n_end ? n0 + BN : n_end) - 1, half_c = p.Cin >> 1;
        const int g = p.dW.div(n0), sd = g - p.dNh.div(g) * p.Nh;
        const bool one = p.dW.div(last) == g;
        const int w_lo = p.dNh.div(n0 - g * p.Nw), w_hi = p.dNh.div(last - g * p.Nw);
        for (int tw = 0; tw < 3; ++tw) {
            const bool l0 = !s3r_cv_ktile_dead_at(p.cv_n, 0, tw, one, sd, w_lo, w_hi);
            const bool l1 = !s3r_cv_ktile_dead_at(p.cv_n, 1, tw, one, sd, w_lo, w_hi);
            for (int cc = 0; cc < chunks; ++cc)          // (a chunk that holds channels of both halves is live when either is)
                if ((cc * WBK < half_c && l0) || (cc * WBK + WBK > half_c && l1)) live |= 1u << (cc * 3 + tw);
        }
        nrun = __builtin_popcount(live);
    }
    const int total = NACC * nrun;

    int bvoff;
    {
        int col, lrow;
        if (B_WIDE) { col = (wave % PPR) * PB + lane * VEC; lrow = 0; }
        else        { col = (lane % LPR_B) * VEC;           lrow = lane / LPR_B; }
        int n = n0 + col;
        if (n >= n_end) n = n_end - VEC;                 // tail tile: fetch a valid group, never stored
        const int b = p.dS.div(n);
        int rem = n - b * S;
        const int pd = p.dHW.div(rem);
        rem -= pd * p.Nh * p.Nw;
        const int q = p.dW.div(rem);
        const int pw = rem - q * p.Nw;
        if constexpr (DECONV)        // padded indices: depth 2 pd + rd (+ 1), row 2q + rh (+ 1), column pw + rw + tw
            bvoff = (b * p.Cin * p.x_cs + (2 * pd + rd) * p.x_ds + (2 * q + rh) * p.x_hs + pw + rw + lrow * p.x_cs) * 4;
        else
            bvoff = (b * p.Cin * p.x_cs + p.x_org + pd * p.x_ds + q * p.x_hs + pw + lrow * p.x_cs) * 4;
    }
    const int avoff = ((lane >> 4) * p.CoutPad + (lane & 15) * 4) * 4;
    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t drsrc =                 // (transposed form: the row differences)
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(DECONV ? p.xd : p.x), 0, (int)p.x_bytes, 0x00020000);
    const size_t x_el = (size_t)p.x_bytes / 4;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.w), 0,
        (int)((unsigned)(DECONV ? 72 : (p.ncls ? p.ncls : NCLS)) * (unsigned)T * (unsigned)p.Cin * (unsigned)p.CoutPad * 4u),
        0x00020000);
    const int b_row0 = B_WIDE ? wave / PPR : wave * RPP;
    constexpr int B_ROW_STEP = B_WIDE ? 4 / PPR : 4 * RPP;
    const int b_lds0 = B_WIDE ? b_row0 * BN + (wave % PPR) * PB : wave * PB;
    constexpr int B_LDS_STEP = B_WIDE ? B_ROW_STEP * BN : 4 * PB;
    const int cs4 = p.x_cs * 4;

    // cursor of the NEXT K tile to fetch (scalar): class, chunk, tap; c_kt = its row block in the packed class slabs
    int c_cls = cls0, c_cc = 0, c_td = 0, c_tw = 0, c_tap = 0;
    int c_kt = (DECONV ? pc * NCLS + cls0 : cls0) * nkt;
    int c_a = cls0 / 3, c_b = cls0 - 3 * (cls0 / 3);     // (transposed form) the class's depth / row part
    unsigned c_rem = live;                               // (CVL) the class's live K tiles still to fetch
#ifdef S3R_ABLATE   // diagnostic builds only (tools/README.md): what the operand DMAs of the K loop cost the matrix pipe
    bool abl_loop = false;                               // set once the prologue's tiles are out
#endif
    auto issue = [&](int buf) __attribute__((always_inline)) {
#ifdef S3R_ABLATE
        // (6: the activation tile of a (class, chunk) fetched for its first column tap only — the traffic a tap-shared B tile would have)
        const bool skip_a = abl_loop && (p.debug == 3 || p.debug == 5);
        const bool skip_b = abl_loop && (p.debug == 3 || p.debug == 4 || (p.debug == 6 && (DECONV ? c_tap != 0 : c_tw != 0)));
#else
        constexpr bool skip_a = false, skip_b = false;
#endif
        if constexpr (CVL) {                             // the class's next live K tile: chunk c_tap / 3, column tap c_tap % 3
            c_tap = __builtin_ctz(c_rem);
            c_kt = c_cls * nkt + c_tap;
        }
        if (!skip_a) {
#pragma unroll
            for (int q = 0; q < WNPA; ++q)
                wdma<16>(wrsrc, As + buf * WBK * WBM + (wave + 4 * q) * 256, avoff,
                         (c_kt * WBK * p.CoutPad + m0) * 4 + (wave + 4 * q) * 4 * p.CoutPad * 4);
        }
        float* sb = Bs + buf * BSTG + b_lds0;
        if constexpr (DECONV) {
            // along an axis, F-class 0: differences at index R, 1: plain at R + 1, 2: differences at R + 1
            const int b_base = ((c_cc * WBK + b_row0) * p.x_cs + (c_a ? p.x_ds : 0) + (c_b ? p.x_hs : 0) + c_tap) * 4;
            if (skip_b) {
            } else if constexpr (XM) {
                // materialised differences: one tile of x / Dh / Dd / Ddh (a descriptor per K tile: the tensors together may pass
                // 2 GiB, and a 4-way choice between ready-made descriptors makes the compiler build a lookup table in scratch)
                const int t_idx = (c_a != 1 ? 2 : 0) + (c_b != 1 ? 1 : 0);          // 0: x, 1: Dh, 2: Dd, 3: Ddh
                const float* tb = t_idx == 0 ? p.x : p.xd + (size_t)(t_idx - 1) * x_el;
                const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(tb), 0, (int)p.x_bytes, 0x00020000);
#pragma unroll
                for (int q = 0; q < NPB; ++q) wdma<4 * VEC>(trsrc, sb + q * B_LDS_STEP, bvoff, b_base + q * B_ROW_STEP * cs4);
            } else if (c_b == 1) {
                // row part b: plain / row differences (two descriptors); depth part a: a difference class fetches depth z + 1 as well
#pragma unroll
                for (int q = 0; q < NPB; ++q) wdma<4 * VEC>(xrsrc, sb + q * B_LDS_STEP, bvoff, b_base + q * B_ROW_STEP * cs4);
                if (c_a != 1) {
#pragma unroll
                    for (int q = 0; q < NPB; ++q)
                        wdma<4 * VEC>(xrsrc, sb + WBK * BN + q * B_LDS_STEP, bvoff, b_base + p.x_ds * 4 + q * B_ROW_STEP * cs4);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NPB; ++q) wdma<4 * VEC>(drsrc, sb + q * B_LDS_STEP, bvoff, b_base + q * B_ROW_STEP * cs4);
                if (c_a != 1) {
#pragma unroll
                    for (int q = 0; q < NPB; ++q)
                        wdma<4 * VEC>(drsrc, sb + WBK * BN + q * B_LDS_STEP, bvoff, b_base + p.x_ds * 4 + q * B_ROW_STEP * cs4);
                }
            }
            ++c_kt;
            if (++c_tap == 2) {
                c_tap = 0;
                if (++c_cc == chunks) {
                    c_cc = 0; ++c_cls;
                    if (++c_b == 3) { c_b = 0; ++c_a; }
                }
            }
        } else if constexpr (CVL) {
            const int cc = c_tap / 3;
            const int b_base = (c_cls * p.x_cls + (cc * WBK + b_row0) * p.x_cs + (c_tap - 3 * cc) * p.x_ds) * 4;
            if (!skip_b) {
#pragma unroll
                for (int q = 0; q < NPB; ++q) wdma<4 * VEC>(xrsrc, sb + q * B_LDS_STEP, bvoff, b_base + q * B_ROW_STEP * cs4);
            }
            c_rem &= c_rem - 1;
            if (c_rem == 0) { c_rem = live; ++c_cls; }
        } else {
            const int b_base = (c_cls * p.x_cls + (c_cc * WBK + b_row0) * p.x_cs + c_td * p.x_ds + c_tw) * 4;
            if (!skip_b) {
#pragma unroll
                for (int q = 0; q < NPB; ++q) wdma<4 * VEC>(xrsrc, sb + q * B_LDS_STEP, bvoff, b_base + q * B_ROW_STEP * cs4);
            }
            ++c_kt;
            if (++c_tw == p.kw) { c_tw = 0; ++c_td; }
            if (++c_tap == T) {
                c_tap = 0; c_td = 0; c_tw = 0;
                if (++c_cc == chunks) { c_cc = 0; ++c_cls; }
            }
        }
    };

    wf32x16 acc[NACC][TM];
#pragma unroll
    for (int c = 0; c < NACC; ++c)
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][t][r] = 0.f;

    // tiles 0 .. WNB-2 go out; tile 0 has landed once at most WNB-2 tiles' DMAs are outstanding
#pragma unroll
    for (int i = 0; i < WNB - 1; ++i)
        if (i < total) issue(i);
    if (total >= WNB - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((WNB - 2) * NPD) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#ifdef S3R_ABLATE
    abl_loop = true;
    if (p.debug == 7) tl1 = __builtin_amdgcn_s_memrealtime();
#endif

    const int a_off = h * WBM + wm * TM * 32 + j * TM;
    const int b_off = h * BN + wn * 32 + j;
    typedef typename WVec<TM>::type AV;
    int cur = 0, g = 0;
    // diff (transposed form, depth part a != 1): the B fragment is the difference of the two depth tiles of the stage
    auto run_class = [&](wf32x16 (&ac)[TM], const bool diff) __attribute__((always_inline)) {
        for (int kt = 0; kt < nrun; ++kt, ++g) {
            const bool more = g + WNB - 1 < total;
            if (more) issue(cur == 0 ? WNB - 1 : cur - 1);        // into the stage tile g - 1 was read from
            const float* a = As + cur * WBK * WBM + a_off;
            const float* b = Bs + cur * BSTG + b_off;
            if (DECONV && diff) {
#pragma unroll
                for (int ks = 0; ks < WBK / 2; ++ks) {
                    const AV av = *reinterpret_cast<const AV*>(a + ks * 2 * WBM);
                    const float bv = b[ks * 2 * BN] - b[WBK * BN + ks * 2 * BN];
#pragma unroll
                    for (int t = 0; t < TM; ++t) ac[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wvget<TM>(av, t), bv, ac[t], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < WBK / 2; ++ks) {
                    const AV av = *reinterpret_cast<const AV*>(a + ks * 2 * WBM);
                    const float bv = b[ks * 2 * BN];
#pragma unroll
                    for (int t = 0; t < TM; ++t) ac[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wvget<TM>(av, t), bv, ac[t], 0, 0, 0);
                }
            }
            if (more) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((WNB - 2) * NPD) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            cur = cur + 1 == WNB ? 0 : cur + 1;
        }
    };
    static_assert(WNB == 2 || !DECONV, "the transposed form issues a class-dependent number of DMAs per K tile: vmcnt(0) only");
    constexpr bool otf = DECONV && !XM;                  // depth differences formed here
    if constexpr (CP) run_class(acc[0], otf && cls0 / 3 != 1);
    else {
#pragma unroll
        for (int c = 0; c < NACC; ++c) run_class(acc[c], otf && c / 3 != 1);
    }

#ifdef S3R_ABLATE
    if (p.debug == 7) tl2 = __builtin_amdgcn_s_memrealtime();
    auto tl_finish = [&]() __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)      // (the "=s" constraint below does not exist for the host pass)
        if (p.debug == 7 && tid == 0 && blockIdx.x < 65536) {
            const unsigned long long t_issued = __builtin_amdgcn_s_memrealtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned hw = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 4);
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* t = s3r_wino_timeline + 6 * (size_t)blockIdx.x;
            t[5] = t_issued;
            t[0] = ((unsigned long long)(xcc & 15u) << 8) | ((hw >> 8) & 0xffu);
            t[1] = tl0; t[2] = tl1; t[3] = tl2; t[4] = __builtin_amdgcn_s_memrealtime();
        }
#endif
    };
#define S3R_TL_FINISH() tl_finish()
#if defined(__HIP_DEVICE_COMPILE__)      // (the "v" constraint does not exist for the host pass)
    if (p.debug == 1) {       // timing-only: no epilogue (accumulators kept live)
#pragma unroll
        for (int c = 0; c < NACC; ++c)
#pragma unroll
            for (int t = 0; t < TM; ++t) asm volatile("" ::"v"(acc[c][t]));
        S3R_TL_FINISH();
        return;
    }
#endif
#else
#define S3R_TL_FINISH() (void)0
#endif
    // rows of this lane: cout m0 + mbase + dm, dm = ((r & 3) + 8 (r >> 2)) * TM + tm
    const int mbase = wm * TM * 32 + 4 * h * TM;
    const int mlimit = p.Cout - (m0 + mbase);
    if constexpr (CP) {
        // ---- class-parallel: the raw class sums to the slab, blocked [cout][64-position tile][class][64]: all classes of a tile's
        // positions are one contiguous run (what the finish kernel reads per position); every lane of the tile has a slot
        static_assert(BN == 64 || !CP, "class-parallel slabs are blocked in 64-position tiles");
        const int cg = DECONV ? pc * NCLS + cls0 : cls0;
        const int nblk = DECONV ? 8 * NCLS : (p.ncls ? p.ncls : NCLS);       // classes per block
        float* __restrict__ slab = p.part + (((size_t)(m0 + mbase) * n_tiles + n_tile) * nblk + cg) * 64 + wn * 32 + j;
        const size_t mstride = (size_t)n_tiles * nblk * 64;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = ((r & 3) + 8 * (r >> 2)) * TM + tm;
                if (dm >= mlimit) continue;
                slab[(size_t)dm * mstride] = acc[0][tm][r];
            }
        S3R_TL_FINISH();
        return;
    } else if constexpr (SEMI) {
        // ---- semi-fused two-axis form: the four row outputs of this depth class, raw, to part[(a * 4 + row)][cout][n - n_begin]
        // blocked by (cout, tile): the 24 partial rows of a tile's 64 positions are one 6 KiB run, so the finish kernel — which
        // needs all 24 of a position — reads a few contiguous blocks instead of 24 streams 11 MB apart
        const int a = cls0 / NCLS;
        static_assert(BN == 64 || !SEMI, "semi-fused slabs are blocked in 64-position tiles");
        float* __restrict__ slab = p.part + (((size_t)(m0 + mbase) * n_tiles + n_tile) * (6 * R) + a * R) * 64 + wn * 32 + j;
        const size_t mstride = (size_t)n_tiles * (6 * R) * 64;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = ((r & 3) + 8 * (r >> 2)) * TM + tm;
                if (dm >= mlimit) continue;
                float m[NCLS], y[R];
#pragma unroll
                for (int c = 0; c < NCLS; ++c) m[c] = acc[c][tm][r];
                wino_out<KIND>(m, y);
#pragma unroll
                for (int i = 0; i < R; ++i) slab[(size_t)dm * mstride + i * 64] = y[i];
            }
        S3R_TL_FINISH();
        return;
    } else {
        // ---- epilogue: per-cout constants through LDS (every wave is past the last barrier: the ring is idle)
        float* ep_sc = wsmem;
        float* ep_sf = wsmem + WBM;
        float* ep_hw = wsmem + 2 * WBM;
        if (tid < WBM) {
            const int m = m0 + tid;
            ep_sc[tid] = (p.scale && m < p.Cout) ? p.scale[m] : 1.f;
            ep_sf[tid] = (p.shift && m < p.Cout) ? p.shift[m] : 0.f;
            if constexpr (HEAD) ep_hw[tid] = (p.head_w && m < p.Cout) ? p.head_w[m] : 0.f;
        }
        __syncthreads();
        const int n = n0 + wn * 32 + j;
        const bool ok = n < n_end;
        int e0, row1 = R;                                    // first output element of the group; rows of it that exist
        {
            const int nn = ok ? n : 0;
            const int b = p.dS.div(nn);
            int rem = nn - b * S;
            const int pd = p.dHW.div(rem);
            rem -= pd * p.Nh * p.Nw;
            const int q = p.dW.div(rem);
            const int pw = rem - q * p.Nw;
            if constexpr (DECONV)    // outputs (2 (2 pd + u) + rd, 2 (2 q + v) + rh, 2 pw + rw), u, v = 0, 1
                e0 = b * p.y_bs + p.y_org + (2 * pd * p.y_ds + 2 * q * p.y_hs + pw) * 2 + rd * p.y_ds + rh * p.y_hs + rw;
            else {
                e0 = b * p.y_bs + p.y_org + pd * p.y_ds + R * q * p.y_hs + pw;
                row1 = p.Hout - R * q;
            }
        }
        const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
        if constexpr (HEAD) {
            // the workgroup's 64 couts are the whole channel axis: this wave holds 32 of them (16 in this lane, 16 in lane j + 32),
            // the wave beside it (wm ^ 1, same wn) the other 32: in-lane chains, the lane halves' sum, then the two waves' sum
            // through LDS (wino_finish_kernel<2, true> walks the couts in this order)
            float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = (r & 3) + 8 * (r >> 2);
                const float sc = ep_sc[mbase + dm], sf = ep_sf[mbase + dm], hw = ep_hw[mbase + dm];
                const float m[9] = {acc[0][0][r], acc[NACC > 1 ? 1 : 0][0][r], acc[NACC > 2 ? 2 : 0][0][r],
                                    acc[NACC > 3 ? 3 : 0][0][r], acc[NACC > 4 ? 4 : 0][0][r], acc[NACC > 5 ? 5 : 0][0][r],
                                    acc[NACC > 6 ? 6 : 0][0][r], acc[NACC > 7 ? 7 : 0][0][r], acc[NACC > 8 ? 8 : 0][0][r]};
                float y[4];
                wino_out<2>(m, y);
                t0 = fmaf(wino_act(y[0], sc, sf, lo), hw, t0);
                t1 = fmaf(wino_act(y[1], sc, sf, lo), hw, t1);
                t2 = fmaf(wino_act(y[2], sc, sf, lo), hw, t2);
                t3 = fmaf(wino_act(y[3], sc, sf, lo), hw, t3);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            t0 += __shfl_xor(t0, 32, 64);
            t1 += __shfl_xor(t1, 32, 64);
            t2 += __shfl_xor(t2, 32, 64);
            t3 += __shfl_xor(t3, 32, 64);
            float* ex = wsmem + 4 * WBM + (wn * 32 + j) * 4;          // behind the epilogue constants
            if (wm == 1 && h == 0) { ex[0] = t0; ex[1] = t1; ex[2] = t2; ex[3] = t3; }
            __syncthreads();
            if (wm == 0 && h == 0 && ok) {
                const float hsc = p.head_scale ? p.head_scale[0] : 1.f, hsf = p.head_shift ? p.head_shift[0] : 0.f;
                p.y[e0] = wino_head_act(fmaf(t0 + ex[0], hsc, hsf), p.head_act);
                p.y[e0 + wino_out_off<KIND>(1, p.y_ds, p.y_hs)] = wino_head_act(fmaf(t1 + ex[1], hsc, hsf), p.head_act);
                p.y[e0 + wino_out_off<KIND>(2, p.y_ds, p.y_hs)] = wino_head_act(fmaf(t2 + ex[2], hsc, hsf), p.head_act);
                p.y[e0 + wino_out_off<KIND>(3, p.y_ds, p.y_hs)] = wino_head_act(fmaf(t3 + ex[3], hsc, hsf), p.head_act);
            }
        } else {
            const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, (int)p.y_bytes, 0x00020000);
            const int yvo0 = (e0 + (m0 + mbase) * p.y_cs) * 4;
            const int row_bytes = p.y_cs * 4;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dm = ((r & 3) + 8 * (r >> 2)) * TM + tm;
                    if (dm >= mlimit) continue;
                    const float sc = ep_sc[mbase + dm], sf = ep_sf[mbase + dm];
                    float m[NCLS], y[R];
#pragma unroll
                    for (int c = 0; c < NCLS; ++c) m[c] = acc[c][tm][r];
                    wino_out<KIND>(m, y);
                    const int so = dm * row_bytes;
                    if (ok) {
#pragma unroll
                        for (int i = 0; i < R; ++i)
                            if (i < row1) {
                                const float v = wino_act(y[i], sc, sf, lo);
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrsrc,
                                                                      yvo0 + 4 * wino_out_off<KIND>(i, p.y_ds, p.y_hs), so, 0);
                            }
                    }
                    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
        }
        S3R_TL_FINISH();
    }
}
#undef S3R_TL_FINISH

// registers: six classes of one 32 x 32 tile = 96 accumulators (109 in all: four workgroups per CU), nine = 144 (three per CU);
// the class-parallel form 16
template <int VEC, int KIND, int WN, bool CP, bool HEAD, bool XM = false, bool SEMI = false, bool CVL = false>
__global__ __launch_bounds__(256, (CP || KIND == 1 ? 4 : 3)) void wino_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsmem[];
    wino_body<VEC, KIND, WN, CP, HEAD, XM, SEMI, CVL>(p, blockIdx.x, gridDim.x, p.n_begin, p.n_end, wsmem);
}

// bulk (serial form, positions [n_begin, n_cut)) + remainder (class-parallel form, positions [n_cut, n_end)) in ONE launch: the
// remainder's short workgroups fill the slots the bulk's last round leaves
template <int VEC, int KIND, bool HEAD = false, bool XM = false>
__global__ __launch_bounds__(256, (KIND == 1 ? 4 : 3)) void wino_dual_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsmem[];
    if ((int)blockIdx.x < p.big_wgs)
        wino_body<VEC, KIND, 2, false, HEAD, XM>(p, blockIdx.x, p.big_wgs, p.n_begin, p.n_cut, wsmem);
    else
        wino_body<VEC, KIND, 2, true, false, XM>(p, (int)blockIdx.x - p.big_wgs, (int)gridDim.x - p.big_wgs, p.n_cut, p.n_end, wsmem);
}

// ---- class-parallel finish: y = act(transform(class sums) * scale + shift) over positions [n_begin, n_end), through the same
// wino_out / wino_act as the serial epilogue.  One thread per (parity class,) cout and position; HEAD: one thread per position
// walks the couts in the serial epilogue's order (the two lane halves' 32-cout chains, then their sum).
template <int KIND, bool HEAD>
__global__ __launch_bounds__(256) void wino_finish_kernel(const ConvParams p, const int n_begin, const int n_end, const int npad) {
    constexpr bool DECONV = KIND == 2;
    constexpr int NCLS = WinoKind<KIND>::NCLS, R = WinoKind<KIND>::R;
    const int S = p.Nd * p.Nh * p.Nw;
    const int nn = n_end - n_begin;
    const int pc = DECONV ? (int)blockIdx.y : 0;
    const int rd = (pc >> 2) & 1, rh = (pc >> 1) & 1, rw = pc & 1;
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    // slabs blocked [cout][64-position tile][class][64] (wino_body, CP): class c of (cout mm, position nl) at blk(mm, nl)[c * 64]
    constexpr int NBLK = DECONV ? 8 * NCLS : NCLS;
    const int ntl = npad >> 6;
    const float* __restrict__ base = p.part + (size_t)pc * NCLS * 64;       // (pc = 0 for convolutions)
    auto blk = [&](int mm, int nl) { return base + ((size_t)mm * ntl + (nl >> 6)) * (NBLK * 64) + (nl & 63); };
    const long long total = HEAD ? nn : (long long)p.Cout * nn;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int mrow = HEAD ? 0 : (int)(i / nn);
        const int nl = (int)(i - (long long)mrow * nn);
        const int n = n_begin + nl;
        const int b = p.dS.div(n);
        int rem = n - b * S;
        const int pd = p.dHW.div(rem);
        rem -= pd * p.Nh * p.Nw;
        const int q = p.dW.div(rem);
        const int pw = rem - q * p.Nw;
        int e0, row1 = R;
        if constexpr (DECONV)
            e0 = b * p.y_bs + p.y_org + (2 * pd * p.y_ds + 2 * q * p.y_hs + pw) * 2 + rd * p.y_ds + rh * p.y_hs + rw;
        else {
            e0 = b * p.y_bs + p.y_org + pd * p.y_ds + R * q * p.y_hs + pw;
            row1 = p.Hout - R * q;
        }
        if constexpr (HEAD) {
            // the serial epilogue's order: per wave (couts 32 wm ..), per lane half (4 hh + ..), a chain over the 16 registers;
            // then the lane halves' sum, then the two waves' sum
            float tw[2][R];
#pragma unroll
            for (int wm = 0; wm < 2; ++wm) {
                float th[2][R];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
                    for (int k = 0; k < R; ++k) th[hh][k] = 0.f;
                    for (int r = 0; r < 16; ++r) {
                        const int mm = 32 * wm + 4 * hh + (r & 3) + 8 * (r >> 2);
                        if (mm >= p.Cout) continue;                    // (padded couts carry head weight 0: t + 0 = t)
                        const float sc = p.scale ? p.scale[mm] : 1.f, sf = p.shift ? p.shift[mm] : 0.f, hw = p.head_w[mm];
                        float m[NCLS], y[R];
#pragma unroll
                        for (int c = 0; c < NCLS; ++c) m[c] = blk(mm, nl)[c * 64];
                        wino_out<KIND>(m, y);
#pragma unroll
                        for (int k = 0; k < R; ++k) th[hh][k] = fmaf(wino_act(y[k], sc, sf, lo), hw, th[hh][k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < R; ++k) tw[wm][k] = th[0][k] + th[1][k];
            }
            const float hsc = p.head_scale ? p.head_scale[0] : 1.f, hsf = p.head_shift ? p.head_shift[0] : 0.f;
#pragma unroll
            for (int k = 0; k < R; ++k)
                p.y[e0 + wino_out_off<KIND>(k, p.y_ds, p.y_hs)] = wino_head_act(fmaf(tw[0][k] + tw[1][k], hsc, hsf), p.head_act);
        } else {
            const float sc = p.scale ? p.scale[mrow] : 1.f, sf = p.shift ? p.shift[mrow] : 0.f;
            float m[NCLS], y[R];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) m[c] = blk(mrow, nl)[c * 64];
            wino_out<KIND>(m, y);
            float* __restrict__ yo = p.y + (size_t)mrow * p.y_cs + e0;
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (k < row1) yo[wino_out_off<KIND>(k, p.y_ds, p.y_hs)] = wino_act(y[k], sc, sf, lo);
        }
    }
}

template <int KIND>
static hipError_t launch_wino_finish(const ConvParams& p, int n_begin, int n_end, int npad, hipStream_t stream) {
    const long long total = p.head_w ? (long long)(n_end - n_begin) : (long long)p.Cout * (n_end - n_begin);
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192), KIND == 2 ? 8 : 1);
    if constexpr (KIND == 2) {
        if (p.head_w) hipLaunchKernelGGL((wino_finish_kernel<KIND, true>), grid, dim3(256), 0, stream, p, n_begin, n_end, npad);
        else hipLaunchKernelGGL((wino_finish_kernel<KIND, false>), grid, dim3(256), 0, stream, p, n_begin, n_end, npad);
    } else {
        hipLaunchKernelGGL((wino_finish_kernel<KIND, false>), grid, dim3(256), 0, stream, p, n_begin, n_end, npad);
    }
    return hipGetLastError();
}

// ---- launch planning ---------------------------------------------------------------------------
#ifdef S3R_ABLATE   // (S3R_WABL, s3r_wino.h)
int wabl_mode() { static const int m = getenv("S3R_ABL") ? atoi(getenv("S3R_ABL")) : 0; return m; }
#endif

int64_t wino_slab_elems(int kind, int cout, int ntotal, const WinoLaunch& L) {
    if (L.mode == WINO_SERIAL) return 0;
    const int ncls = kind == 2 ? 72 : 6;
    const int n0 = L.mode == WINO_DUAL ? L.n_cut : 0;
    const int64_t npad = (int64_t)((ntotal - n0 + WCN - 1) / WCN) * WCN;
    return (int64_t)ncls * cout * npad;
}

// Which form a layer's launch takes (all forms produce the same bits, so this may follow the batch).  forced >= 0 (tuning,
// tests): 0 serial, 1 class-parallel, 2 dual.  Otherwise a cost model in units of one K step of a 64 x 64 tile on one CU
// (13.4 ns at the fp32 MFMA peak), fitted to tools/layer_bench.py --algo 2 sweeps at B = 1 .. 32:
//   kcls = K per class (Cin x taps), u = serial workgroups per CU;
//   serial          ceil(u) workgroups of ncls * kcls steps each, at 0.9 of the pipe (a workgroup left alone on its CU: 0.7)
//   class-parallel  ceil(u * ncls) workgroups of kcls steps at 0.9, + 100 steps each for their slab's round trip, + a finish launch
//   dual            k serial workgroups per CU (k = floor(u), or one fewer when the last would run alone) + 0.6 of the remainder
//                   class-parallel
WinoLaunch wino_plan(int kind, int cout, int kcls, int ntotal, bool head, int forced) {
    WinoLaunch L;
    L.mode = WINO_SERIAL; L.n_cut = 0;
    const int m_tiles = (cout + WBM - 1) / WBM;
    const int pcs = kind == 2 ? 8 : 1;
    const int ncls = kind == 2 ? 9 : 6;
    const long W = (long)m_tiles * ((ntotal + WCN - 1) / WCN) * pcs;                 // serial workgroups (64-position tiles)
    if (forced < 0) {
        static const int env_mode = getenv("S3R_WINO_FORM") ? atoi(getenv("S3R_WINO_FORM")) : -1;      // A/B switch, read once
        forced = env_mode;
    }
    const int occ = kind == 2 ? 3 : 4;                   // serial workgroups a CU holds at once (registers)
    const int CUS = cu_count();
    const double u = (double)W / (double)CUS;            // serial workgroups per CU
    int kb = (int)u;                                     // bulk rounds of a dual launch: whole workgroups per CU
    if (forced >= 0) {
        L.mode = forced <= WINO_DUAL ? forced : WINO_SERIAL;
        if ((double)kb >= u) kb -= 1;                    // (a forced dual launch always leaves a remainder)
    } else {
        (void)head;
        constexpr double EFF = 0.9, EFF_ALONE = 0.7, SLAB = 100.0, LAUNCH = 220.0, TAIL = 0.6;
        const double unit = (double)ncls * kcls;
        // w workgroups per CU, `occ` at a time: the last one alone on its CU runs at EFF_ALONE
        auto serial_cost = [&](int w) {
            const int rem = w % occ;
            return (w - (rem == 1 ? 1 : 0)) * unit / EFF + (rem == 1 ? unit / EFF_ALONE : 0.0);
        };
        const double serial = serial_cost((int)__builtin_ceil(u));
        const double cp = __builtin_ceil(u * ncls) * (kcls / EFF + SLAB) + LAUNCH;
        double best = serial;
        if (cp < best) { best = cp; L.mode = WINO_CP; }
        // (the remainder's short workgroups run beside the bulk's last round: TAIL of their own time shows)
        // k = floor(u), or one fewer when that would leave a CU's last bulk workgroup alone
        for (int k : {(int)u, (int)u % occ == 1 ? (int)u - 1 : 0}) {
            if (k < 1 || (double)k >= u) continue;
            const double dual = serial_cost(k) + TAIL * __builtin_ceil((u - k) * ncls) * (kcls / EFF + SLAB) + LAUNCH;
            if (dual < 0.97 * best) { best = dual; L.mode = WINO_DUAL; kb = k; }
        }
    }
    if (L.mode == WINO_DUAL) {
        const long n_main = ((long)kb * CUS) / (m_tiles * pcs);                        // whole N tiles in the bulk
        L.n_cut = (int)(n_main * WCN);
        if (L.n_cut <= 0 || L.n_cut >= ntotal) { L.mode = L.n_cut <= 0 ? WINO_CP : WINO_SERIAL; L.n_cut = 0; }
    }
    return L;
}

// The two run-time switches of a transposed layer as template arguments: f(head, xm), two std::bool_constant — the fused head
// (p.head_w; HEAD_OK = false: a form that leaves the head to its finish pass) and materialised depth differences (p.xd_mode).
// A convolution (KIND 1) has neither.
template <int KIND, bool HEAD_OK, class F>
static void wino_switches(const ConvParams& p, F f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if constexpr (KIND == 2) {
        if constexpr (HEAD_OK) {
            if (p.head_w) return p.xd_mode ? f(yes, yes) : f(yes, no);
        }
        return p.xd_mode ? f(no, yes) : f(no, no);
    } else {
        f(no, no);
    }
}

template <int VEC, int KIND>
static hipError_t launch_wino_forms(ConvParams p, const WinoLaunch& L, hipStream_t stream) {
    const int ntotal = p.Ntotal;
    if (p.out_mode && (KIND != 2 || L.mode != WINO_CP)) return hipErrorInvalidValue;      // (the hand-off pass reads whole-range class slabs)
    const size_t lds = (size_t)WNB * WBK * (WBM + (KIND == 2 ? 2 : 1) * WCN) * sizeof(float);
    const int pcs = KIND == 2 ? 8 : 1;
    constexpr int NCLS = WinoKind<KIND>::NCLS;
    p.n_begin = 0; p.n_end = ntotal;
    if (L.mode == WINO_SERIAL) {
        const dim3 grid(p.m_tiles * ((ntotal + WCN - 1) / WCN) * pcs);
        wino_switches<KIND, true>(p, [&](auto head, auto xm) {
            hipLaunchKernelGGL((wino_kernel<VEC, KIND, 2, false, decltype(head)::value, decltype(xm)::value>), grid, dim3(256), lds, stream, p);
        });
        return hipGetLastError();
    }
    if (!p.part) return hipErrorInvalidValue;
    const int n0 = L.mode == WINO_DUAL ? L.n_cut : 0;
    const int cp_tiles = (ntotal - n0 + WCN - 1) / WCN;
    const int cp_wgs = p.m_tiles * cp_tiles * NCLS * pcs;
    if (L.mode == WINO_DUAL) {
        p.n_cut = n0;
        p.big_wgs = p.m_tiles * (n0 / WCN) * pcs;
        const dim3 grid(p.big_wgs + cp_wgs);
        wino_switches<KIND, true>(p, [&](auto head, auto xm) {
            hipLaunchKernelGGL((wino_dual_kernel<VEC, KIND, decltype(head)::value, decltype(xm)::value>), grid, dim3(256), lds, stream, p);
        });
    } else {
        wino_switches<KIND, false>(p, [&](auto, auto xm) {
            hipLaunchKernelGGL((wino_kernel<VEC, KIND, 2, true, false, decltype(xm)::value>), dim3(cp_wgs), dim3(256), lds, stream, p);
        });
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.out_mode) return launch_wino_handoff(p, 2, p.out_mode - 1, cp_tiles * WCN, stream);
    // (aux pass: reads the class slabs of the class-parallel range, writes that range's outputs)
    AuxScope aux(stream, 4.0 * (double)(ntotal - n0) * p.Cout * (pcs * NCLS + (p.head_w ? 0.0 : pcs * WinoKind<KIND>::R)));
    return launch_wino_finish<KIND>(p, n0, ntotal, cp_tiles * WCN, stream);
}

// p: see wino_body.  Returns the kernel launches made through *launches (may be null).
hipError_t launch_conv_wino(ConvParams p, const WinoLaunch& L, hipStream_t stream, int* launches) {
    if (p.Cin % WBK != 0 || p.stride != 1 || p.transposed || p.ksplit != 1 || p.head_w || p.act == ACT_SIGMOID)
        return hipErrorInvalidValue;
    p.kh = 1;
    S3R_WABL(p);
    p.m_tiles = (p.Cout + WBM - 1) / WBM;
    if (launches) *launches = L.mode == WINO_SERIAL ? 1 : 2;
    return p.Nw % 4 == 0 ? launch_wino_forms<4, 1>(p, L, stream) : launch_wino_forms<1, 1>(p, L, stream);
}

hipError_t launch_deconv_wino(ConvParams p, const WinoLaunch& L, hipStream_t stream, int* launches) {
    if (p.Cin % WBK != 0 || !p.transposed || p.ksplit != 1 || !p.xd || p.act == ACT_SIGMOID || (p.head_w && p.Cout > WBM))
        return hipErrorInvalidValue;
    S3R_WABL(p);
    p.m_tiles = (p.Cout + WBM - 1) / WBM;
    if (launches) *launches = L.mode == WINO_SERIAL ? 1 : 2;
    if (p.Nw % 4 != 0) return hipErrorInvalidValue;       // (16-byte gathers only: the library's policy asks for an edge % 4 == 0)
    return launch_wino_forms<4, 2>(p, L, stream);
}

// the two-axis forms' class GEMM (declared in s3r_wino.h; launch_conv_wino2 makes q and every refusal)
hipError_t launch_wino2_classes(const ConvParams& q, bool semi, bool cvl, hipStream_t stream) {
    const dim3 grid(q.m_tiles * ((q.Ntotal + WCN - 1) / WCN) * (semi ? 6 : q.ncls));
    const size_t lds = (size_t)WNB * WBK * (WBM + WCN) * sizeof(float);
    if (semi) {
        if (cvl) hipLaunchKernelGGL((wino_kernel<4, 1, 2, false, false, false, true, true>), grid, dim3(256), lds, stream, q);
        else if (q.Nw % 4 == 0) hipLaunchKernelGGL((wino_kernel<4, 1, 2, false, false, false, true>), grid, dim3(256), lds, stream, q);
        else hipLaunchKernelGGL((wino_kernel<1, 1, 2, false, false, false, true>), grid, dim3(256), lds, stream, q);
    } else {
        if (cvl) hipLaunchKernelGGL((wino_kernel<4, 1, 2, true, false, false, false, true>), grid, dim3(256), lds, stream, q);
        else if (q.Nw % 4 == 0) hipLaunchKernelGGL((wino_kernel<4, 1, 2, true, false>), grid, dim3(256), lds, stream, q);
        else hipLaunchKernelGGL((wino_kernel<1, 1, 2, true, false>), grid, dim3(256), lds, stream, q);
    }
    return hipGetLastError();
}

#ifdef S3R_ABLATE
}  // namespace s3r
extern "C" int s3r_debug_read_timeline_wino(unsigned long long* out, int nblocks) {
    if (nblocks > 65536) nblocks = 65536;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(s3r::s3r_wino_timeline), sizeof(unsigned long long) * 6 * (size_t)nblocks) == hipSuccess ? nblocks : -1;
}
extern "C" int s3r_debug_clear_timeline_wino() {
    void* ptr = nullptr;
    if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(s3r::s3r_wino_timeline)) != hipSuccess) return -1;
    return hipMemset(ptr, 0, sizeof(unsigned long long) * 6 * 65536) == hipSuccess ? 0 : -1;
}
namespace s3r {
#endif

}  // namespace s3r
