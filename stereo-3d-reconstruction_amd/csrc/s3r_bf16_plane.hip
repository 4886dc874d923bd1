// bf16 MFMA path (s3r_bf16.h has the path's essay and the map of its units), the stride-1 family that sums K in the plane
// kernel's order: plane reuse (conv_bf16p_kernel: one gather per kh*kw taps) and the row-persistent kernel of the shallow front
// layer (conv_bf16w_kernel: the same bits, chosen by batch size).
#include "s3r_bf16.h"

namespace s3r {

#ifdef S3R_ABLATE
// S3R_ABL=7: per-workgroup timeline stamps of the plane kernel (s_memrealtime, 100 MHz); read_timeline_plane reads them:
// [cu key, entry, tables done, first image landed, loop end, epilogue issued, stores landed]
static __device__ unsigned long long s3r_timeline_h[8 * 65536];
#endif

// Plane-reuse variant (stride-1 layers): ALL kh*kw taps of one (KC-channel chunk, td) group
// read the same gathered input PLANE, shifted by th*in_p + tw positions, so the A operand is fetched once per
// kh*kw taps (9 for a 3x3[x3] conv, 4 for a transposed-conv class) instead of once per tap / per kw taps.
//
// LDS A image = for every (batch, depth) plane the tile touches, the contiguous run of padded-input positions
// u = ph*in_p + pw .. that its output positions need, plus
// HALO = (kh-1)*in_p + kw-1 trailing positions; MFMA row r reads LDS row lrow[r] + th*in_p + tw.  The image is
// SINGLE-buffered (two or three workgroups per CU overlap one's reload with the others' MFMAs); the weights
// stream through a 3-slot ring with one barrier per tap.
constexpr int NPA_PL = 15;     // 8-row A pieces per wave, upper bound (registers), 128-byte rows
constexpr int NPA_PL32 = 12;   // 16-row pieces, 64-byte rows
// weight ring slots of the plane kernel: a tap's weights are requested pl_nb - 1 taps ahead.  Three slots (two taps of lead) is the
// measured optimum: r06 built the ring for any depth and five slots (four taps of lead; + 8 KiB per workgroup, which takes e4 / v3 /
// v5 / d3 from three workgroups per CU to two) measured e4 + 19 %, d3 + 17 %, v3 + 11 %, v5 + 13 % SLOWER at B = 256, e7 / d1 / d2
// - 2 ... - 3 % (gpurun_out/r6e/ab, A/B on one device): occupancy, not the weights' latency, is what these loops live on.
#ifndef S3R_PL_NB32
#define S3R_PL_NB32 3
#endif
constexpr int pl_nb(int kc) { return kc == 32 ? S3R_PL_NB32 : 3; }
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void wait_vm_n(int n) {      // n is wave-uniform and small: one immediate form per value
    switch (n) {
        case 0: wait_vm<0>(); break;
        case 1: wait_vm<1>(); break;
        case 2: wait_vm<2>(); break;
        case 3: wait_vm<3>(); break;
        case 4: wait_vm<4>(); break;
        case 5: wait_vm<5>(); break;
        case 6: wait_vm<6>(); break;
        case 7: wait_vm<7>(); break;
        default: wait_vm<8>(); break;
    }
}

// KC = 64: 128-byte image rows (whole lines), two workgroups per CU; KC = 32: 64-byte rows, half the LDS, three
// workgroups per CU (and the only form for Cin = 32).
// NH = 64-cout halves per workgroup (2: a 256 x 128 tile, the image serves twice the couts; two workgroups per CU).
// HEAD: the fused pointwise-head epilogue is its own instantiation (d3 only).  Compiled into the same kernel behind a
// run-time test (r01), the two epilogues shared one register allocation at the 168-VGPR cap of three waves per SIMD
// and every layer's kernel spilled 40 bytes per lane to scratch; now the plain kernel needs 113 VGPRs and none.  The
// head instantiation still spills its 40 bytes at three waves per SIMD — measured faster (d3 1.32 vs 1.45 ms) than
// giving it 176 registers at two.
template <int SH, int TM, int KC, int NH, bool HEAD = false>
__global__ __launch_bounds__(256, (KC == 64 || NH == 2) ? 2 : 3) void conv_bf16p_kernel(const ConvParamsH p, int r_max) {
    static_assert(!HEAD || NH == 1, "the fused head needs the whole channel axis in one 64-cout tile");
    typedef Mf<SH> M;
    constexpr int MT = M::MT;
    constexpr int NPT = 32 * TM / MT, NCT = 64 / MT, NKS = KC / M::KS;
    constexpr int BM = 128 * TM;
    constexpr int BNW = HBN * NH;                  // couts per workgroup
    constexpr int ROWB = KC * 2;                   // bytes per LDS row
    constexpr int LPR = ROWB / 16;                 // lanes (16-byte slots) per row
    constexpr int RPP = 64 / LPR;                  // rows per 1 KiB LDS-DMA piece
    constexpr int B_BYTES = BNW * ROWB;            // one tap's weight tile
    constexpr int NPB = B_BYTES / 4096;            // its pieces per wave
    constexpr int NPA_CAP = KC == 64 ? NPA_PL : NPA_PL32;
    constexpr int PL_NB = pl_nb(KC);               // weight ring slots; a tap's weights are requested PL_D taps ahead
    constexpr int PL_D = PL_NB - 1;
    static_assert(NPB * (PL_D - 1) <= 8, "wait_vm_n covers 0 .. 8");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int a_bytes = r_max * ROWB;
    char* Bs = smem + a_bytes;                                        // [PL_NB][64][ROWB]
    int* yoff = reinterpret_cast<int*>(Bs + PL_NB * B_BYTES);         // [BM] output element offsets, -1 = none
    int* lrow = yoff + BM;                                            // [BM] LDS row of each tile position (tap 0,0)
    float* ep = reinterpret_cast<float*>(lrow + BM);                  // [3][64] scale / shift / head weight
    int* asrc = reinterpret_cast<int*>(Bs + (PL_NB - 1) * B_BYTES);  // [r_max] source byte offset of each image row
                                                                      // (prologue only: aliases the last ring slot)
    // The prologue (tables, first image) and the epilogue are short, latency-bound instruction streams that run beside
    // two other workgroups' K loops on the same SIMDs; as the YOUNGEST wave of its SIMD this one loses every issue
    // arbitration (priority, then age) and a timeline showed 3-4 us of tables and 4.4-5.8 us of epilogue per workgroup
    // (tools/timeline_bf16.py).  Raised priority outside the K loop lets those phases through; the loop runs at 0.
    __builtin_amdgcn_s_setprio(S3R_PRIO_EDGE);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane % MT, lk = lane / MT;
#ifdef S3R_ABLATE
    unsigned long long tl[6] = {0, 0, 0, 0, 0, 0};
    if (p.debug == 7) tl[0] = __builtin_amdgcn_s_memrealtime();
#endif

    int bid = blockIdx.x, cls = 0;
    wg_order(p.transposed, bid, cls);
    const int n_tiles_w = p.n_tiles / NH;
    const int n_tile = (bid % n_tiles_w) * NH;     // first 64-cout tile of this workgroup
    const int m_tile = bid / n_tiles_w;
    const int m0 = m_tile * BM, n0 = n_tile * HBN;
    const int rd = (cls >> 2) & 1, rh = (cls >> 1) & 1, rw = cls & 1;
    const int kz = blockIdx.z;

    const int S = p.Nd * p.Nh * p.Nw, P = p.Nh * p.Nw;
    const int T = p.T, kh = p.kh, kw = p.kw;
    const int taps_g = kh * kw;
    const int chunks = (p.Cin / KC) / p.ksplit;
    const int gpc = p.kd;                                    // groups (image loads) per chunk
    const int ngroups = S3R_ABLH(p, 2) ? 1 : chunks * gpc;
    const int total = ngroups * taps_g;
    const int cls_x = p.transposed ? (rd - 1) * p.x_ds + (rh - 1) * p.x_hs + (rw - 1) * p.x_ws : 0;
    const int in_p = p.x_hs / p.x_ws;                        // padded input row length, in positions
    const int halo = (kh - 1) * in_p + kw - 1;
    const int umax = (p.Nh - 1) * in_p + p.Nw - 1;
    const int LP = umax + 1 + halo;                          // image rows of a whole plane

    // ---- geometry of the tile's first and last position (wave-uniform)
    const int m1 = (m0 + BM < p.Ntotal ? m0 + BM : p.Ntotal) - 1;
    int pl0, u0, pl1, u1;
    {
        pl0 = p.dHW.div(m0);
        int nl = m0 - pl0 * P;
        int ph = p.dW.div(nl);
        u0 = ph * in_p + (nl - ph * p.Nw);
        pl1 = p.dHW.div(m1);
        nl = m1 - pl1 * P;
        ph = p.dW.div(nl);
        u1 = ph * in_p + (nl - ph * p.Nw);
    }
    const int nseg = pl1 - pl0 + 1;
    const int len0 = (nseg > 1 ? umax : u1) - u0 + 1 + halo; // image rows of the first plane's segment

    const EpRegs epr = load_ep(p, tid, n0, BNW);

    // ---- the first two taps' weights depend on nothing the prologue computes: fetch them before it
    const int w_tile = p.n_tiles * 4096;
    int bvoff[NPB];
#pragma unroll
    for (int q = 0; q < NPB; ++q) {
        if constexpr (KC == 32) {
            bvoff[q] = (wave + 4 * q) * 1024 + lane * 16;     // stored pre-swizzled for 64-byte rows
        } else {
            const int r = (wave + 4 * q) * RPP + lane / LPR;
            const int kg = (lane % LPR) ^ swz<64>(r);
            bvoff[q] = (kg >> 2) * (T * w_tile) + r * 64 + (((kg & 3) ^ swz<32>(r)) << 4);
        }
    }
    const size_t w_cls = (size_t)cls * T * (p.Cin / HKC) * w_tile;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.w) + w_cls), 0,
        (int)((unsigned)T * (unsigned)(p.Cin / HKC) * (unsigned)w_tile), 0x00020000);
    int b_cc = kz * chunks, b_tap = 0, b_slot = 0;            // cursor of the NEXT weight tile to fetch
    auto issue_b = [&]() {
        const int b_base = ((b_cc * (KC / 32) * T + b_tap) * p.n_tiles + n_tile) * 4096;
#pragma unroll
        for (int q = 0; q < NPB; ++q) dma16(wrsrc, Bs + b_slot * B_BYTES + ((wave + 4 * q) << 10), bvoff[q], b_base);
        if (++b_tap == T) { b_tap = 0; ++b_cc; }
        if (++b_slot == PL_NB) b_slot = 0;
    };
#pragma unroll
    for (int i = 0; i < PL_D; ++i)
        if (i < total) issue_b();

    for (int t = tid; t < BM; t += 256) {
        const int n = m0 + t;
        const bool ok = n < p.Ntotal;
        const int nn = ok ? n : p.Ntotal - 1;
        const auto [b, pd, ph, pw] = decode_pos(p, nn, S);
        const int ye = out_offset(p, b, pd, ph, pw, rd, rh, rw);
        yoff[t] = ok ? ye : -1;
        const int sgm = b * p.Nd + pd - pl0, u = ph * in_p + pw;
        lrow[t] = sgm == 0 ? u - u0 : len0 + (sgm - 1) * LP + u;
    }
    // source of every image row: (plane, position inside the padded plane)
    for (int j = tid; j < r_max; j += 256) {
        int sgm, off;
        if (j < len0) { sgm = 0; off = j + u0; }
        else { sgm = 1 + (j - len0) / LP; off = (j - len0) - (sgm - 1) * LP; }
        int pl = pl0 + sgm;
        if (sgm >= nseg) { pl = pl1; off = 0; }              // past the image: any valid address, never read
        const int b = p.dS.div(pl * P);
        const int pd = pl - b * p.Nd;
        asrc[j] = (b * p.x_bs + p.x_org + pd * p.x_ds + off * p.x_ws + cls_x) * 2;
    }
    // publish the LDS tables.  NOT __syncthreads(): the compiler drains vmcnt before a barrier it knows about, which would
    // wait out the two weight tiles and the per-cout constants requested above (an L2 / HBM round trip in the prologue
    // of every workgroup) — they only have to land by the first tap / the epilogue
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- loop-invariant DMA source offsets
    // A pieces (RPP rows each) are dealt round-robin to the four waves; r_max is a whole number of pieces
    int avoff[NPA_CAP];
#pragma unroll
    for (int q = 0; q < NPA_CAP; ++q) {
        const int j = (wave + 4 * q) * RPP + lane / LPR;
        avoff[q] = (j < r_max ? asrc[j] : 0) + (((lane % LPR) ^ swz<KC>(j)) << 4);
    }
    int lr[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) lr[pt] = lrow[wave * 32 * TM + pt * MT + li];
    int b_off[NCT * NH];
#pragma unroll
    for (int ct = 0; ct < NCT * NH; ++ct) {
        const int row = ct * MT + li;
        b_off[ct] = row * ROWB + ((lk ^ swz<KC>(row)) << 4);
    }

    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    int a_cc = kz * chunks, a_td = 0;                         // cursor of the NEXT image to fetch
    auto issue_a = [&]() {
        const int a_base = (a_cc * KC + a_td * p.x_ds) * 2;
#pragma unroll
        for (int q = 0; q < NPA_CAP; ++q)
            if ((wave + 4 * q) * RPP < r_max) dma16(xrsrc, smem + ((wave + 4 * q) << 10), avoff[q], a_base);
        if (++a_td == gpc) { a_td = 0; ++a_cc; }
    };
    typename M::acc_t acc[NH][NPT][NCT];
#pragma unroll
    for (int nh = 0; nh < NH; ++nh)
#pragma unroll
        for (int a = 0; a < NPT; ++a)
#pragma unroll
            for (int b = 0; b < NCT; ++b)
#pragma unroll
                for (int r = 0; r < M::NACC; ++r) acc[nh][a][b][r] = 0.f;

#ifdef S3R_ABLATE
    if (p.debug == 7) tl[1] = __builtin_amdgcn_s_memrealtime();
#endif
    issue_a();                                                // (asrc aliases the LAST ring slot, first filled
                                                              //  behind the loop's first barrier)

    __builtin_amdgcn_s_setprio(0);
    int tt = 0, c_slot = 0;
    for (int g = 0; g < ngroups; ++g) {
        int tapoff = 0, c_tw = 0;
        const int ntaps = taps_g;
        for (int t = 0; t < ntaps; ++t, ++tt) {
            // this tap's weights (and, at t == 0, the image) have landed; the next tap's may still be in flight.
            // (s_barrier as inline asm: the compiler drains vmcnt before every barrier it knows about, which
            // would cut the weight prefetch back to one tap)
            // (the taps tt + 1 .. tt + PL_D - 1 requested behind it may still be in flight; at t == 0 the image, requested last, must
            // have landed too)
            {
                const int ahead = total - 1 - tt < PL_D - 1 ? total - 1 - tt : PL_D - 1;
                if (t == 0) wait_vm<0>();
                else wait_vm_n(NPB * ahead);
            }
            asm volatile("s_barrier" ::: "memory");           // ... for every wave; ring slot (tt + PL_D) % PL_NB is free
#ifdef S3R_ABLATE
            if (p.debug == 7 && tt == 0) tl[2] = __builtin_amdgcn_s_memrealtime();
#endif
            if (tt + PL_D < total && !S3R_ABLH(p, 3)) issue_b();
            const char* b = Bs + c_slot * B_BYTES;
            int a_off[NPT];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
                const int row = lr[pt] + tapoff;
                a_off[pt] = row * ROWB + ((lk ^ swz<KC>(row)) << 4);
            }
            // fragments of k-step q+1 are requested before the MFMAs of k-step q
            bf16x8 av[2][NPT], bv[2][NCT * NH];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) av[0][pt] = *reinterpret_cast<const bf16x8*>(smem + a_off[pt]);
#pragma unroll
            for (int ct = 0; ct < NCT * NH; ++ct) bv[0][ct] = *reinterpret_cast<const bf16x8*>(b + b_off[ct]);
#pragma unroll
            for (int q = 0; q < NKS; ++q) {
                if (q < NKS - 1) {
#pragma unroll
                    for (int pt = 0; pt < NPT; ++pt)
                        av[(q + 1) & 1][pt] = *reinterpret_cast<const bf16x8*>(smem + (a_off[pt] ^ ((q + 1) * M::NK * 16)));
#pragma unroll
                    for (int ct = 0; ct < NCT * NH; ++ct)
                        bv[(q + 1) & 1][ct] = *reinterpret_cast<const bf16x8*>(b + (b_off[ct] ^ ((q + 1) * M::NK * 16)));
                }
#pragma unroll
                for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                    for (int ct = 0; ct < NCT * NH; ++ct)
                        acc[ct / NCT][pt][ct % NCT] = mma<SH>(bv[q & 1][ct], av[q & 1][pt], acc[ct / NCT][pt][ct % NCT]);
            }
            // pin the issue order (the scheduler otherwise reuses the fragment registers and serialises
            // read -> wait -> MFMA): k-step 0's reads, then per k-step one read of the NEXT step behind each MFMA
            if constexpr (NKS > 1) {
                __builtin_amdgcn_sched_group_barrier(0x100, NPT + NCT * NH, 0);
#pragma unroll
                for (int q = 0; q < NKS - 1; ++q)
#pragma unroll
                    for (int i = 0; i < NCT * NH * NPT; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i < NPT + NCT * NH) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                __builtin_amdgcn_sched_group_barrier(0x008, NCT * NH * NPT, 0);
            }
            if (++c_slot == PL_NB) c_slot = 0;
            ++tapoff;
            if (++c_tw == kw) { c_tw = 0; tapoff += in_p - kw; }
        }
        asm volatile("s_barrier" ::: "memory");               // every wave is done with this image
        if (g + 1 < ngroups && !S3R_ABLH(p, 3)) issue_a();
    }

#ifdef S3R_ABLATE
    if (p.debug == 7) tl[3] = __builtin_amdgcn_s_memrealtime();
#endif
    __builtin_amdgcn_s_setprio(S3R_PRIO_EDGE);
    store_ep(epr, ep, tid, BNW);
#pragma unroll
    for (int nh = 0; nh < NH; ++nh)
        epilogue_h<SH, TM, HEAD>(p, acc[nh], yoff, ep + nh * 192, smem + wave * (32 * ST_ROW), wave, li, lk, m0, n0 + nh * HBN,
                                 cls, kz, BM);
#ifdef S3R_ABLATE
    if (p.debug == 7 && tid == 0 && blockIdx.y == 0 && blockIdx.z == 0 && blockIdx.x < 65536) {
        tl[4] = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tl[5] = __builtin_amdgcn_s_memrealtime();
        const unsigned hw = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 4);
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* t = s3r_timeline_h + 8 * (size_t)blockIdx.x;
        t[0] = ((unsigned long long)(xcc & 15u) << 8) | ((hw >> 8) & 0xffu);
        for (int i = 0; i < 6; ++i) t[1 + i] = tl[i];
    }
#endif
}

// LDS rows (128 B each) of the plane-reuse kernel's A image for a BM-position tile: an upper bound over all
// tiles (see conv_bf16p_kernel), in whole 1 KiB LDS-DMA pieces (8 / 16 rows); 0 = layer not eligible
int plane_rows(const ConvParamsH& p, int bm, int kc) {
    if (p.stride != 1 || p.Cin % kc != 0 || p.x_hs % p.x_ws != 0) return 0;
    const int in_p = p.x_hs / p.x_ws, P = p.Nh * p.Nw;
    const int halo = (p.kh - 1) * in_p + p.kw - 1;
    // tiles start at multiples of bm: when rows / planes divide bm (or bm divides the plane) they are never straddled
    // (e2: 112^2 = 49 x 256; d3: 16^2 = 256; d2: 4 planes of 64, d1: 16 planes of 16 per tile)
    const int rows_touched = (bm % p.Nw == 0) ? bm / p.Nw : (bm + p.Nw - 2) / p.Nw + 1;
    const int nseg = (P % bm == 0) ? 1 : (bm % P == 0) ? bm / P : (bm + P - 2) / P + 1;
    const int r = bm + (in_p - p.Nw) * rows_touched + nseg * halo;
    const int unit = kc == 64 ? 8 : 16;            // rows per 1 KiB LDS-DMA piece
    return (r + unit - 1) / unit * unit;
}

template <int SH, int TM, int KC, int NH = 1>
static hipError_t launch_tm_plane(ConvParamsH p, hipStream_t stream) {
    constexpr int BM = 128 * TM;
    p.m_tiles = (p.Ntotal + BM - 1) / BM;
    p.n_tiles = p.CoutPad / HBN;
    const int r_max = plane_rows(p, BM, KC);
    if (r_max == 0 || r_max > (KC == 64 ? 32 * NPA_PL : 64 * NPA_PL32) || (p.Cin / KC) % p.ksplit != 0)
        return hipErrorInvalidValue;
    if (NH == 2 && (p.n_tiles % 2 != 0 || p.head_w)) return hipErrorInvalidValue;
    const size_t lds = (size_t)r_max * KC * 2 + pl_nb(KC) * HBN * NH * KC * 2 + 2 * BM * sizeof(int) + EP_BYTES * NH;
    if (lds > 160 * 1024 || r_max * 4 > HBN * NH * KC * 2) return hipErrorInvalidValue;
    static LdsAttr lds_attr;
    dim3 grid(p.m_tiles * (p.n_tiles / NH) * (p.transposed ? 8 : 1), 1, p.ksplit);      // (class inside blockIdx.x: wg_order)
    if constexpr (NH == 1) {
        if (p.head_w && p.ksplit == 1) {
            static LdsAttr lds_attr_h;
            const hipError_t ah = lds_attr_h.ensure(reinterpret_cast<const void*>(&conv_bf16p_kernel<SH, TM, KC, NH, true>), 160 * 1024);
            if (ah != hipSuccess) return ah;
            hipLaunchKernelGGL((conv_bf16p_kernel<SH, TM, KC, NH, true>), grid, dim3(256), lds, stream, p, r_max);
            return hipGetLastError();
        }
    }
    if (p.head_w) return hipErrorInvalidValue;
    const hipError_t attr = lds_attr.ensure(reinterpret_cast<const void*>(&conv_bf16p_kernel<SH, TM, KC, NH, false>), 160 * 1024);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((conv_bf16p_kernel<SH, TM, KC, NH, false>), grid, dim3(256), lds, stream, p, r_max);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? launch_finish_bf16(p, BM, stream) : e;
}

// ------------------------------------------------------------------------------------------------
// Row-persistent variant for the shallow front layer (e2: Conv2d 32 -> 64, k3 s1 p1 over 112 x 112; K = 288).  In the
// plane kernel above such a layer is all fixed cost: 11.6 us of tables, first image, epilogue and store tail per
// workgroup around 1.2 us of MFMAs, its input fetched 1.9 times over (every tile reloads its halo rows), its output
// stored in 32-position pieces (tools/timeline_bf16.py).  Here a workgroup of SEVEN waves owns a strip
// of output rows of one image and slides down it FOUR output rows (448 positions = 7 waves x 2 tiles of 32) per step:
//   * the layer's weights (9 taps x 4 KiB per 64 couts) are fetched ONCE per workgroup and stay in LDS;
//   * input rows live in a ring of ten 8-KiB slots (a padded row is 114 x 64 B; slot = padded row mod 10); a step
//     reads six of them and, at its start, requests the four NEW rows of the next step — one contiguous 29 KB run of the
//     channels-last input, each row as eight whole 1-KiB LDS-DMA pieces — so every input row crosses HBM -> LDS once;
//   * ONE workgroup barrier per step (rows landed for everyone / everyone done with the rows about to be replaced),
//     none inside it: 72 MFMAs per wave straight through, operands from LDS only;
//   * the position -> (row, column) tables are computed once per workgroup: a step moves two scalar offsets;
//   * the four output rows of a step are 448 x 128 B = 56 KB contiguous in the channels-last output.
// The K order (tap-major, two 16-channel k-steps per tap) is the plane kernel's, so the two produce the same bits and
// the library is free to pick by batch size (the rows kernel needs >= 256 strips to fill the chip).
constexpr int RW_WAVES = 7;
constexpr int RW_R = 4;                          // output rows per step
constexpr int RW_NS = 10;                        // ring slots (input rows)
constexpr int RW_SLOT = 128 * 64;                // bytes per slot: 128 positions x 32 channels (114 used)
constexpr int RW_LDS = RW_NS * RW_SLOT + 9 * 4096 + RW_WAVES * 32 * ST_ROW + 448 * 4 + EP_BYTES;

template <int SH>
__global__ __launch_bounds__(64 * RW_WAVES) void conv_bf16w_kernel(const ConvParamsH p, int strips, int units) {
    typedef Mf<SH> M;
    constexpr int MT = M::MT;
    constexpr int NPT = 64 / MT, NCT = 64 / MT, NKS = HKC / M::KS;
    constexpr int W = 112, WP = 114;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                               // [RW_NS][128][64 B]
    char* wts = smem + RW_NS * RW_SLOT;                              // [9 taps][64 rows][64 B] (pre-swizzled by the pack kernel)
    char* stage = wts + 9 * 4096 + 0;                                // [RW_WAVES][32][ST_ROW]
    int* yoff = reinterpret_cast<int*>(stage + RW_WAVES * 32 * ST_ROW);   // [448] output element offset inside a step
    float* ep = reinterpret_cast<float*>(yoff + 448);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane % MT, lk = lane / MT;
    const int n_tile = blockIdx.y, n0 = n_tile * HBN;

    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.w), 0, (int)(9u * (unsigned)p.n_tiles * 4096u), 0x00020000);

    // ---- once per workgroup: the weights, the per-cout constants, the position tables
    for (int pc = wave; pc < 36; pc += RW_WAVES) {                   // 36 pieces of 1 KiB: tap = pc >> 2
        const int tap = pc >> 2;
        dma16(wrsrc, wts + pc * 1024, lane * 16, ((tap * p.n_tiles + n_tile) * 4 + (pc & 3)) * 1024);
    }
    const EpRegs epr = load_ep(p, tid, n0);
    for (int t = tid; t < RW_R * W; t += 64 * RW_WAVES) {
        const int dr = t / W, c = t - dr * W;
        yoff[t] = dr * p.y_hs + c * p.y_ws;
    }
    store_ep(epr, ep, tid);                                          // (__syncthreads inside: also publishes yoff)

    // per lane: the two position tiles' (row in step, column), and per tw the byte offset inside a slot
    int dr[NPT], colpart[NPT][3];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
        const int n = wave * 64 + pt * MT + li;
        dr[pt] = n / W;
        const int c = n - dr[pt] * W;
#pragma unroll
        for (int tw = 0; tw < 3; ++tw) colpart[pt][tw] = (c + tw) * 64 + ((lk ^ swz<32>(c + tw)) << 4);
    }
    int b_off[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int row = ct * MT + li;
        b_off[ct] = row * 64 + ((lk ^ swz<32>(row)) << 4);
    }
    // DMA source offset of this lane inside a 16-position piece: position l >> 2, channel group (l & 3) ^ swz(position).
    // A slot starts at a multiple of 128 LDS rows and a piece at a multiple of 16, so the swizzle of an LDS row depends
    // on the lane only: ONE loop-invariant offset, the piece's 1 KiB goes into the scalar offset.
    const int pvoff = (lane >> 2) * 64 + (((lane & 3) ^ swz<32>(lane >> 2)) << 4);
    // rows [r0, r0 + nr) of the padded image at byte offset `img` -> their ring slots; 8 pieces per row
    auto issue_rows = [&](int img, int r0, int nr) {
        for (int pc = wave; pc < nr * 8; pc += RW_WAVES) {
            const int rr = pc >> 3, i = pc & 7;
            const int prow = r0 + rr;
            const int slot = prow % RW_NS;
            dma16(xrsrc, ring + slot * RW_SLOT + i * 1024, pvoff, img + prow * (WP * 64) + i * 1024);
        }
    };

    const int rows_per_strip = W / strips;                           // (launcher: a multiple of RW_R)
    const int steps = rows_per_strip / RW_R;
    for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int b = unit / strips, st = unit - b * strips;
        const int img = (b * p.x_bs) * 2;                            // byte offset of the padded image (x_org = 0: halo 1, pad 1)
        const int row0 = st * rows_per_strip;                        // first output row = first padded input row of the strip
        __syncthreads();                                             // every wave is done with the previous unit's rows
        issue_rows(img, row0, RW_R + 2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int s = 0; s < steps; ++s) {
            const int p0 = row0 + s * RW_R;                          // padded input row of tap row 0 of the step's first output row
            __builtin_amdgcn_s_barrier();                            // this step's rows have landed for every wave; the rows of
            asm volatile("" ::: "memory");                           // step s - 1 that the next request replaces are free
            if (s + 1 < steps) issue_rows(img, p0 + RW_R + 2, RW_R);
            int slotoff[NPT][3];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                for (int th = 0; th < 3; ++th) slotoff[pt][th] = ((p0 + dr[pt] + th) % RW_NS) * RW_SLOT;
            typename M::acc_t acc[NPT][NCT];
#pragma unroll
            for (int a = 0; a < NPT; ++a)
#pragma unroll
                for (int c = 0; c < NCT; ++c)
#pragma unroll
                    for (int r = 0; r < M::NACC; ++r) acc[a][c][r] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int th = tap / 3, tw = tap - th * 3;
                const char* b = wts + tap * 4096;
#pragma unroll
                for (int q = 0; q < NKS; ++q) {
                    bf16x8 av[NPT], bv[NCT];
#pragma unroll
                    for (int pt = 0; pt < NPT; ++pt)
                        av[pt] = *reinterpret_cast<const bf16x8*>(ring + ((slotoff[pt][th] + colpart[pt][tw]) ^ (q * M::NK * 16)));
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) bv[ct] = *reinterpret_cast<const bf16x8*>(b + (b_off[ct] ^ (q * M::NK * 16)));
#pragma unroll
                    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) acc[pt][ct] = mma<SH>(bv[ct], av[pt], acc[pt][ct]);
                }
            }
            const int ybase = b * p.y_bs + p.y_org + (row0 + s * RW_R) * p.y_hs;
            // the rows of step s + 1 (requested at the top of this step, a whole MFMA phase ago) and the previous step's stores are
            // all that is outstanding here: wait for them BEFORE this step's stores go out, so that the wait does not have to know
            // how many stores the epilogue issues (it used to be vmcnt(8) behind it: a count shared silently by two functions)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            epilogue_h<SH, 2, false, true>(p, acc, yoff, ep, stage + wave * (32 * ST_ROW), wave, li, lk, 0, n0, 0, 0, 0, ybase);
        }
    }
}

// can the row-persistent kernel serve this layer, and in how many row strips per image?  (0 = no.)  Geometry: e2's.  The
// kernel is bit-identical to the plane family, so — unlike the choice of family — this may depend on the batch: it needs
// >= 512 strips of >= 28 rows to fill 256 CUs with two work units each.
int rows_strips(const ConvParamsH& p) {
    if (p.transposed || p.stride != 1 || p.kd != 1 || p.kh != 3 || p.kw != 3 || p.Cin != 32 || p.Nd != 1 ||
        p.Nh != 112 || p.Nw != 112 || p.x_ws != 32 || p.x_hs != 114 * 32 || p.x_org != 0 || p.ksplit != 1 || p.head_w ||
        (p.Cout & 7) != 0 || p.act == ACT_SIGMOID)
        return 0;
    for (int strips = 1; strips <= 4; strips *= 2)
        if ((long)p.B * strips >= 512) return strips;
    return 0;
}

template <int SH>
static hipError_t launch_rows(ConvParamsH p, hipStream_t stream) {
    const int strips = rows_strips(p);
    if (!strips) return hipErrorInvalidValue;
    p.n_tiles = p.CoutPad / HBN;
    p.m_tiles = 0;
    static LdsAttr lds_attr;
    const hipError_t attr = lds_attr.ensure(reinterpret_cast<const void*>(&conv_bf16w_kernel<SH>), RW_LDS);
    if (attr != hipSuccess) return attr;
    static int cus[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    if (!cus[dev] && (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus[dev] < 1))
        cus[dev] = 256;
    const int units = p.B * strips;
    const int per_tile = cus[dev] / p.n_tiles > 0 ? cus[dev] / p.n_tiles : 1;       // one workgroup per CU in all
    dim3 grid(units < per_tile ? units : per_tile, p.n_tiles, 1);
    hipLaunchKernelGGL((conv_bf16w_kernel<SH>), grid, dim3(64 * RW_WAVES), RW_LDS, stream, p, strips, units);
    return hipGetLastError();
}

template <int SH>
static hipError_t launch_plane_sh(const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream) {
    if (t.family == BF16_ROWS) return launch_rows<SH>(p, stream);            // row-persistent (e2 at large batches)
    if (t.nh == 2) return launch_tm_plane<SH, 2, 32, 2>(p, stream);          // 256 positions x 128 couts
    if (t.kc32) return t.tm == 1 ? launch_tm_plane<SH, 1, 32>(p, stream) : launch_tm_plane<SH, 2, 32>(p, stream);
    return t.tm == 1 ? launch_tm_plane<SH, 1, 64>(p, stream) : launch_tm_plane<SH, 2, 64>(p, stream);
}
hipError_t launch_bf16_plane(int sh, const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream) {
    return sh == 16 ? launch_plane_sh<16>(t, p, stream) : launch_plane_sh<32>(t, p, stream);
}

#ifdef S3R_ABLATE
int read_timeline_plane(unsigned long long* out, int nblocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(s3r_timeline_h), sizeof(unsigned long long) * 8 * (size_t)nblocks) == hipSuccess ? nblocks : -1;
}
#endif

}  // namespace s3r
