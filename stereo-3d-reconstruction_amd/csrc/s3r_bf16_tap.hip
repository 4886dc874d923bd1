// bf16 MFMA path (s3r_bf16.h has the path's essay and the map of its units), the two double-buffered gathers that work at any
// stride: per tap (conv_bf16_kernel: every K tile gathers one tap's input positions again; stride 2, shallow K, pointwise layers)
// and row reuse (conv_bf16r_kernel: one gather per kw taps; deep stride-1 layers with an odd number of 64-cout tiles).
#include "s3r_bf16.h"

namespace s3r {

#ifdef S3R_ABLATE
// S3R_ABL=7: per-workgroup timeline stamps of the per-tap kernel (s_memrealtime, 100 MHz); read_timeline_tap reads them
static __device__ unsigned long long s3r_timeline_h[8 * 65536];
#endif

// (the fused-head epilogue keeps 3 constants per cout live: its own instantiation, one workgroup fewer per CU,
// so that the plain kernel stays free of scratch; KC = 64 doubles the LDS per workgroup)
constexpr int min_waves_h(int tm, int kc, bool head) {
    return kc == 64 ? (tm == 1 ? 3 : 1) : (tm >= 4 ? 2 : (head ? 3 : 4));
}

// Per-tap kernel.  K tile = ONE tap x KC channels.  KC = 64 (Cin % 64 == 0) makes every gathered piece a WHOLE
// 128-byte line of the channels-last input (KC = 32 fetches half of each line, and the other half again one
// chunk later: the operand path of these layers is L2 -> LDS bound) and halves the barriers per FLOP.
// The packed weights stay in the 32-channel layout for both: with KC = 64 a lane's 16 bytes come from chunk
// 2j or 2j+1 by a per-lane source offset (LDS-DMA destinations are lane-linear, sources are free).
// NH = 64-cout halves per workgroup: 2 (a 128 x 128 tile; Cout % 128 == 0) gathers the activations once for twice
// the couts — 1.5x the FLOPs per byte brought into LDS, for the layers this kernel keeps (stride 2), which are
// bound by exactly that.
// tap visiting order of stride-2 3x3x3 layers (tap id = (td*3 + th)*3 + tw, 5 bits each, 9 per word): parity classes,
// each along a Gray path —  0 2 8 6 24 26 20 18 | 1 7 25 19 | 3 5 23 21 | 9 11 17 15 | 4 22 | 10 16 | 12 14 | 13
constexpr unsigned long long S2_3D_A = 0x19535832040ull, S2_3D_B = 0xb4d6e51cf27ull, S2_3D_C = 0xd7320ab11f1ull;

template <int SH, int TM, int KC, bool HEAD, int NH>
__global__ __launch_bounds__(256, NH == 2 ? (KC == 64 ? 2 : 3) : min_waves_h(TM, KC, HEAD)) void conv_bf16_kernel(const ConvParamsH p) {
    static_assert(NH == 1 || !HEAD, "the fused head needs the whole channel axis in one 64-cout tile");
    typedef Mf<SH> M;
    constexpr int MT = M::MT;
    constexpr int NPT = 32 * TM / MT;              // position tiles per wave
    constexpr int NCT = 64 / MT;                   // cout tiles per 64-cout block
    constexpr int NKS = KC / M::KS;                // MFMA k steps per K tile
    constexpr int BM = 128 * TM;
    constexpr int BNW = HBN * NH;                  // couts per workgroup
    constexpr int ROWB = KC * 2;                   // bytes per LDS row
    constexpr int LPR = ROWB / 16;                 // lanes (16-byte slots) per row
    constexpr int RPP = 64 / LPR;                  // rows per 1 KiB LDS-DMA piece
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BNW * ROWB;
    constexpr int NPA = A_BYTES / 4096, NPB = B_BYTES / 4096;     // pieces per wave per K tile

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                               // [2][BM][ROWB]
    char* Bs = smem + 2 * A_BYTES;                 // [2][BNW][ROWB]
    int* xoff = reinterpret_cast<int*>(smem + 2 * A_BYTES + 2 * B_BYTES);   // [BM] input byte offsets
    int* yoff = xoff + BM;                                                   // [BM] output element offsets, -1 = none
    float* ep = reinterpret_cast<float*>(yoff + BM);                         // [NH][3][64] scale / shift / head weight

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane % MT, lk = lane / MT;

    int bid = blockIdx.x, cls = 0;
    wg_order(p.transposed, bid, cls);
    const int n_tiles_w = p.n_tiles / NH;          // workgroup cout tiles
    const int n_tile = (bid % n_tiles_w) * NH;     // first 64-cout tile (fastest: neighbours share the gathered input)
    const int m_tile = bid / n_tiles_w;
    const int m0 = m_tile * BM, n0 = n_tile * HBN;
    const int rd = (cls >> 2) & 1, rh = (cls >> 1) & 1, rw = cls & 1;
    const int kz = blockIdx.z;

    const int S = p.Nd * p.Nh * p.Nw;
    const int T = p.T;
    const int chunks = (p.Cin / KC) / p.ksplit;
    const int nkt = S3R_ABLH(p, 2) ? 1 : T * chunks;
#ifdef S3R_ABLATE   // S3R_ABL=7: [cu key, entry, tables done, first K tile landed, loop end, epilogue issued, stores landed, ticks spent in the
    unsigned long long tl[7] = {0, 0, 0, 0, 0, 0, 0};      // loop's `s_waitcnt vmcnt(0)` (operands of the NEXT K tile not landed yet)]
    if (p.debug == 7) tl[0] = __builtin_amdgcn_s_memrealtime();
#endif

    const EpRegs epr = load_ep(p, tid, n0, BNW);
    // ---- decode this tile's positions once: input corner (bytes) and output offset (elements)
    for (int t = tid; t < BM; t += 256) {
        const int n = m0 + t;
        const bool ok = n < p.Ntotal;
        const int nn = ok ? n : p.Ntotal - 1;
        const auto [b, pd, ph, pw] = decode_pos(p, nn, S);
        int xe = b * p.x_bs + p.x_org + (pd * p.x_ds + ph * p.x_hs + pw * p.x_ws) * p.stride;
        if (p.transposed) xe += (rd - 1) * p.x_ds + (rh - 1) * p.x_hs + (rw - 1) * p.x_ws;
        const int ye = out_offset(p, b, pd, ph, pw, rd, rh, rw);
        xoff[t] = xe * 2;
        yoff[t] = ok ? ye : -1;
    }
    __syncthreads();

    // ---- loop-invariant DMA source offsets (the swizzle is applied on the source side)
    const int w_tile = p.n_tiles * 4096;           // bytes between consecutive 32-channel weight tiles (kt32 + 1)
    int avoff[NPA], bvoff[NPB];
#pragma unroll
    for (int q = 0; q < NPA; ++q) {
        const int pl = (wave + 4 * q) * RPP + lane / LPR;          // position inside the tile
        const int kg = (lane % LPR) ^ swz<KC>(pl);
        avoff[q] = xoff[pl] + kg * 16;
    }
#pragma unroll
    for (int q = 0; q < NPB; ++q) {
        if constexpr (KC == 32) {
            bvoff[q] = (wave + 4 * q) * 1024 + lane * 16;          // stored pre-swizzled for 64-byte rows
        } else {
            const int r = (wave + 4 * q) * RPP + lane / LPR;       // cout row (consecutive 64-cout tiles are 4 KiB apart)
            const int kg = (lane % LPR) ^ swz<64>(r);              // 16-byte channel group 0..7 of the 64
            bvoff[q] = (kg >> 2) * (T * w_tile) + r * 64 + (((kg & 3) ^ swz<32>(r)) << 4);
        }
    }

    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    // packed weights: [cls][kt32 = chunk32*T + tap][cout tile][64 rows][64 B]
    const size_t w_cls = (size_t)cls * T * (p.Cin / HKC) * w_tile;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.w) + w_cls), 0,
        (int)((unsigned)T * (unsigned)(p.Cin / HKC) * (unsigned)w_tile), 0x00020000);

    int c_td = 0, c_th = 0, c_tw = 0, c_tap = 0, c_cc = kz * chunks;
    // Stride-2 3x3[x3] layers visit their taps by PARITY CLASS.  At stride 2 a tap index 0 and a tap index 2 along an
    // axis read the same input rows (planes, columns) one output position apart, tap index 1 reads the others: the
    // taps fall into classes that gather the same pixels — the 4 (8 in 3D) "corner" taps, 2 + 2 (4 + 4 + 4) edge groups,
    // ..., the centre alone.  In kh-major order the second gather of a pixel comes up to 6 K tiles after the first — of
    // every workgroup on the XCD, ~10 MB of other gathers against a 4 MB L2 — and e3 / v2 fetched 1.5x / 1.6x their
    // input.  Walking each class along a Gray path (consecutive taps differ along one axis) puts every re-read one
    // K tile behind the read it repeats.  The packed weights stay in tap order (c_tap indexes them); the order is a
    // function of the layer's geometry only, so a sample's K order is the same in every batch.
    const bool s2_order = p.stride == 2 && !p.transposed && p.kh == 3 && p.kw == 3 && (p.kd == 1 || p.kd == 3);
    int c_v = 0;                                   // visit index 0 .. T-1 (s2_order)
    auto visit = [&](int v) {                      // -> c_td, c_th, c_tw, c_tap of visit v
        // (orders packed in immediates: a table in memory put a load on the path of every K tile's DMA issue)
        if (p.kd == 1) {
            c_tap = (int)((0x453716820ull >> (4 * v)) & 15ull);                       // 0 2 8 6 | 1 7 | 3 5 | 4
        } else {
            const int g = v / 9, i = v - g * 9;                                       // 27 ids, 5 bits each, 9 per word
            const unsigned long long w = g == 0 ? S2_3D_A : (g == 1 ? S2_3D_B : S2_3D_C);
            c_tap = (int)((w >> (5 * i)) & 31ull);
        }
        c_td = c_tap / 9;
        const int r = c_tap - c_td * 9;
        c_th = r / 3;
        c_tw = r - c_th * 3;
    };
    if (s2_order) visit(0);

    auto issue = [&](int buf) {
        const int b_base = ((c_cc * (KC / 32) * T + c_tap) * p.n_tiles + n_tile) * 4096;
#pragma unroll
        for (int q = 0; q < NPB; ++q)
            dma16(wrsrc, Bs + buf * B_BYTES + (wave + 4 * q) * 1024, bvoff[q], b_base);
        const int a_base = (c_cc * KC + (c_td * p.x_ds + c_th * p.x_hs + c_tw * p.x_ws)) * 2;
#pragma unroll
        for (int q = 0; q < NPA; ++q)
            dma16(xrsrc, As + buf * A_BYTES + (wave + 4 * q) * 1024, avoff[q], a_base);
        if (s2_order) {
            if (++c_v == T) { c_v = 0; ++c_cc; }
            visit(c_v);
        } else {
            if (++c_tw == p.kw) { c_tw = 0; if (++c_th == p.kh) { c_th = 0; ++c_td; } }
            if (++c_tap == T) { c_tap = 0; c_td = 0; c_th = 0; c_tw = 0; ++c_cc; }
        }
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
    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef S3R_ABLATE
    if (p.debug == 7) tl[2] = __builtin_amdgcn_s_memrealtime();
#endif

    // fragment byte offsets inside a K tile image: row*ROWB + ((NK*q + lk) ^ swz(row))*16; q toggles the bits above lk's
    int a_off[NPT], b_off[NCT * NH];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
        const int row = wave * 32 * TM + pt * MT + li;
        a_off[pt] = row * ROWB + ((lk ^ swz<KC>(row)) << 4);
    }
#pragma unroll
    for (int ct = 0; ct < NCT * NH; ++ct) {
        const int row = ct * MT + li;
        b_off[ct] = row * ROWB + ((lk ^ swz<KC>(row)) << 4);
    }

    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt && !S3R_ABLH(p, 3)) issue(cur ^ 1);
        const char* a = As + cur * A_BYTES;
        const char* b = Bs + cur * B_BYTES;
#pragma unroll
        for (int q = 0; q < NKS; ++q) {
            bf16x8 av[NPT], bv[NCT * NH];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) av[pt] = *reinterpret_cast<const bf16x8*>(a + (a_off[pt] ^ (q * M::NK * 16)));
#pragma unroll
            for (int ct = 0; ct < NCT * NH; ++ct) bv[ct] = *reinterpret_cast<const bf16x8*>(b + (b_off[ct] ^ (q * M::NK * 16)));
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                for (int ct = 0; ct < NCT * NH; ++ct)
                    acc[ct / NCT][pt][ct % NCT] = mma<SH>(bv[ct], av[pt], acc[ct / NCT][pt][ct % NCT]);
        }
#ifdef S3R_ABLATE
        unsigned long long w0 = 0;
        if (p.debug == 7) w0 = __builtin_amdgcn_s_memrealtime();
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef S3R_ABLATE
        if (p.debug == 7) tl[6] += __builtin_amdgcn_s_memrealtime() - w0;
#endif
        __syncthreads();
    }
#ifdef S3R_ABLATE
    if (p.debug == 7) tl[3] = __builtin_amdgcn_s_memrealtime();
#endif

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
        t[7] = tl[6];
    }
#endif
}

template <int SH, int TM, int KC, bool HEAD, int NH>
static hipError_t launch_tm_k(const ConvParamsH& p, hipStream_t stream) {
    constexpr int BM = 128 * TM;
    constexpr size_t lds = (size_t)2 * BM * KC * 2 + 2 * HBN * NH * KC * 2 + 2 * BM * sizeof(int) + EP_BYTES * NH;
    static_assert(lds <= 160 * 1024, "tile does not fit the LDS");
    if (lds > 48 * 1024) {
        static LdsAttr lds_attr;
        const hipError_t attr = lds_attr.ensure(reinterpret_cast<const void*>(&conv_bf16_kernel<SH, TM, KC, HEAD, NH>), (int)lds);
        if (attr != hipSuccess) return attr;
    }
    dim3 grid(p.m_tiles * (p.n_tiles / NH) * (p.transposed ? 8 : 1), 1, p.ksplit);
    hipLaunchKernelGGL((conv_bf16_kernel<SH, TM, KC, HEAD, NH>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// kc32: the caller forces 32-channel K tiles (tile code + 16); otherwise 64 wherever the layer allows it.
// NH = 2: 128-cout workgroup tiles (Cout % 128 == 0, no fused head).
template <int SH, int TM, int NH>
static hipError_t launch_tm(ConvParamsH p, bool kc32, hipStream_t stream) {
    constexpr int BM = 128 * TM;
    p.m_tiles = (p.Ntotal + BM - 1) / BM;
    p.n_tiles = p.CoutPad / HBN;
    const bool head = p.head_w && p.ksplit == 1;
    if (NH == 2 && (p.n_tiles % 2 != 0 || head)) return hipErrorInvalidValue;
    const bool kc64 = !kc32 && p.Cin % 64 == 0 && (p.Cin / 64) % p.ksplit == 0;
    hipError_t e;
    if constexpr (NH == 2) {
        e = kc64 ? launch_tm_k<SH, TM, 64, false, 2>(p, stream) : launch_tm_k<SH, TM, 32, false, 2>(p, stream);
    } else {
        e = kc64 ? (head ? launch_tm_k<SH, TM, 64, true, 1>(p, stream) : launch_tm_k<SH, TM, 64, false, 1>(p, stream))
                 : (head ? launch_tm_k<SH, TM, 32, true, 1>(p, stream) : launch_tm_k<SH, TM, 32, false, 1>(p, stream));
    }
    return e == hipSuccess ? launch_finish_bf16(p, BM, stream) : e;
}

// ------------------------------------------------------------------------------------------------
// Row-reuse variant: the kw taps of one (chunk, td, th) group read the SAME gathered input
// rows shifted by one position, so the A operand is fetched ONCE per group instead of once per tap.
//
// LDS A image = the input positions the tile needs for a fixed (td, th), in input order: for every run of
// tile positions inside one output row, a segment of stride*(run-1)+kw consecutive input positions
// (64 B = 32 channels each); MFMA row r reads LDS row lrow[r] + tw for tap tw.  No position is computed that
// is not stored (the halo columns sit in LDS but no MFMA row maps to them), the gather is kw (x stride)
// times smaller, and it is CONTIGUOUS in HBM (whole runs of positions) instead of 64-byte pieces.
// The weights of the group's kw taps (kw x 4 KiB, consecutive in the packed image) ride along, so there
// is one barrier per GROUP.
template <int SH, int TM>
__global__ __launch_bounds__(256, 2) void conv_bf16r_kernel(const ConvParamsH p, int r_max) {
    typedef Mf<SH> M;
    constexpr int MT = M::MT;
    constexpr int NPT = 32 * TM / MT, NCT = 64 / MT, NKS = HKC / M::KS;
    constexpr int BM = 128 * TM;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kw = p.kw;
    const int a_bytes = r_max * 64, stage_bytes = a_bytes + kw * 4096;
    int* yoff = reinterpret_cast<int*>(smem + 2 * stage_bytes);     // [BM] output element offsets, -1 = none
    int* lrow = yoff + BM;                                            // [BM] LDS row of each tile position (tap tw = 0)
    float* ep = reinterpret_cast<float*>(lrow + BM);                  // [3][64] scale / shift / head weight

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane % MT, lk = lane / MT;

    int bid = blockIdx.x, cls = 0;
    wg_order(p.transposed, bid, cls);
    const int n_tile = bid % p.n_tiles;
    const int m_tile = bid / p.n_tiles;
    const int m0 = m_tile * BM, n0 = n_tile * HBN;
    const int rd = (cls >> 2) & 1, rh = (cls >> 1) & 1, rw = cls & 1;
    const int kz = blockIdx.z;

    const int S = p.Nd * p.Nh * p.Nw;
    const int T = p.T;
    const int chunks = (p.Cin / HKC) / p.ksplit;
    const int ngroups = S3R_ABLH(p, 2) ? 1 : chunks * p.kd * p.kh;
    const int cls_x = p.transposed ? (rd - 1) * p.x_ds + (rh - 1) * p.x_hs + (rw - 1) * p.x_ws : 0;

    // ---- geometry of the tile's first position (wave-uniform): its output row and column
    int rowid0, pw0;
    {
        const int b = p.dS.div(m0);
        int rem = m0 - b * S;
        const int pd = p.dHW.div(rem);
        rem -= pd * p.Nh * p.Nw;
        const int ph = p.dW.div(rem);
        pw0 = rem - ph * p.Nw;
        rowid0 = (b * p.Nd + pd) * p.Nh + ph;
    }
    const int seg0 = p.stride * (p.Nw - pw0 - 1) + kw;       // LDS rows of the first (partial) run
    const int segw = p.stride * (p.Nw - 1) + kw;             // LDS rows of a full output row
    const int last_row = p.B * p.Nd * p.Nh - 1;

    const EpRegs epr = load_ep(p, tid, n0);
    for (int t = tid; t < BM; t += 256) {
        const int n = m0 + t;
        const bool ok = n < p.Ntotal;
        const int nn = ok ? n : p.Ntotal - 1;
        const auto [b, pd, ph, pw] = decode_pos(p, nn, S);
        const int ye = out_offset(p, b, pd, ph, pw, rd, rh, rw);
        yoff[t] = ok ? ye : -1;
        const int k = (b * p.Nd + pd) * p.Nh + ph - rowid0;
        lrow[t] = k == 0 ? p.stride * (pw - pw0) : seg0 + (k - 1) * segw + p.stride * pw;
    }

    // ---- loop-invariant DMA source offsets: LDS row q of the A image <- input position src(q)
    const int npa = r_max >> 6;                               // pieces per wave (r_max % 64 == 0)
    int avoff[NPA_MAX];
#pragma unroll
    for (int q = 0; q < NPA_MAX; ++q) {
        const int lr = ((wave + 4 * q) << 4) + (lane >> 2);   // LDS row this lane fills in its q-th piece
        int k, off;
        if (lr < seg0) { k = 0; off = lr + p.stride * pw0; }
        else { k = 1 + (lr - seg0) / segw; off = (lr - seg0) - (k - 1) * segw; }      // (segw depends on kw: plain divide)
        int rowid = rowid0 + k;
        if (rowid > last_row) rowid = last_row;              // past the tensor: any valid address, never read
        const int b = p.dDH.div(rowid);
        int rem = rowid - b * (p.Nd * p.Nh);
        const int pd = p.dH.div(rem);
        const int ph = rem - pd * p.Nh;
        const int e = b * p.x_bs + p.x_org + (pd * p.x_ds + ph * p.x_hs) * p.stride + off * p.x_ws + cls_x;
        const int kg = (lane & 3) ^ swz<32>(lr);              // swizzle on the source side
        avoff[q] = e * 2 + kg * 16;
    }
    const int bvoff = lane * 16;

    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const size_t w_cls = (size_t)cls * T * (p.Cin / HKC) * p.n_tiles * 4096;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.w) + w_cls), 0,
        (int)((unsigned)T * (unsigned)(p.Cin / HKC) * (unsigned)p.n_tiles * 4096u), 0x00020000);

    int c_td = 0, c_th = 0, c_cc = kz * chunks, c_kt = kz * chunks * T;      // cursor of the NEXT group to fetch

    auto issue = [&](int buf) {
        char* st = smem + buf * stage_bytes;
        for (int tw = 0; tw < kw; ++tw)                                      // the group's kw weight tiles
            dma16(wrsrc, st + a_bytes + tw * 4096 + wave * 1024, bvoff,
                  ((c_kt + tw) * p.n_tiles + n_tile) * 4096 + wave * 1024);
        const int a_base = (c_cc * HKC + c_td * p.x_ds + c_th * p.x_hs) * 2;
#pragma unroll
        for (int q = 0; q < NPA_MAX; ++q)
            if (q < npa) dma16(xrsrc, st + ((wave + 4 * q) << 10), avoff[q], a_base);
        c_kt += kw;
        if (++c_th == p.kh) { c_th = 0; if (++c_td == p.kd) { c_td = 0; ++c_cc; } }
    };

    typename M::acc_t acc[NPT][NCT];
#pragma unroll
    for (int a = 0; a < NPT; ++a)
#pragma unroll
        for (int b = 0; b < NCT; ++b)
#pragma unroll
            for (int r = 0; r < M::NACC; ++r) acc[a][b][r] = 0.f;

    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                          // also publishes yoff / lrow

    int lr[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) lr[pt] = lrow[wave * 32 * TM + pt * MT + li];
    int b_off[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int row = ct * MT + li;
        b_off[ct] = row * 64 + ((lk ^ swz<32>(row)) << 4);
    }

    for (int g = 0; g < ngroups; ++g) {
        const int cur = g & 1;
        if (g + 1 < ngroups && !S3R_ABLH(p, 3)) issue(cur ^ 1);
        const char* a = smem + cur * stage_bytes;
        const char* b = a + a_bytes;
        for (int tw = 0; tw < kw; ++tw) {
            int a_off[NPT];
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
                const int row = lr[pt] + tw;
                a_off[pt] = (row << 6) + ((lk ^ swz<32>(row)) << 4);
            }
#pragma unroll
            for (int q = 0; q < NKS; ++q) {
                bf16x8 av[NPT], bv[NCT];
#pragma unroll
                for (int pt = 0; pt < NPT; ++pt) av[pt] = *reinterpret_cast<const bf16x8*>(a + (a_off[pt] ^ (q * M::NK * 16)));
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    bv[ct] = *reinterpret_cast<const bf16x8*>(b + tw * 4096 + (b_off[ct] ^ (q * M::NK * 16)));
#pragma unroll
                for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        acc[pt][ct] = mma<SH>(bv[ct], av[pt], acc[pt][ct]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    store_ep(epr, ep, tid);
    if (p.head_w) epilogue_h<SH, TM, true>(p, acc, yoff, ep, smem + wave * (32 * ST_ROW), wave, li, lk, m0, n0, cls, kz, BM);
    else epilogue_h<SH, TM, false>(p, acc, yoff, ep, smem + wave * (32 * ST_ROW), wave, li, lk, m0, n0, cls, kz, BM);
}

// LDS rows (64 B each) the row-reuse kernel's A image needs for a BM-position tile, rounded to whole pieces per wave
int rowreuse_rows(const ConvParamsH& p, int bm) {
    const int nrows = (bm + p.Nw - 2) / p.Nw + 1;
    const int r = p.stride * bm + nrows * p.kw;
    return (r + 63) / 64 * 64;
}

template <int SH, int TM>
static hipError_t launch_tm_rowreuse(ConvParamsH p, hipStream_t stream) {
    constexpr int BM = 128 * TM;
    p.m_tiles = (p.Ntotal + BM - 1) / BM;
    p.n_tiles = p.CoutPad / HBN;
    const int r_max = rowreuse_rows(p, BM);
    if (r_max > 64 * NPA_MAX) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * (r_max * 64 + p.kw * 4096) + 2 * BM * sizeof(int) + EP_BYTES;
    static LdsAttr lds_attr;                       // (per device: see LdsAttr)
    const hipError_t attr = lds_attr.ensure(reinterpret_cast<const void*>(&conv_bf16r_kernel<SH, TM>), 160 * 1024);
    if (attr != hipSuccess) return attr;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    dim3 grid(p.m_tiles * p.n_tiles * (p.transposed ? 8 : 1), 1, p.ksplit);
    hipLaunchKernelGGL((conv_bf16r_kernel<SH, TM>), grid, dim3(256), lds, stream, p, r_max);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? launch_finish_bf16(p, BM, stream) : e;
}

template <int SH>
static hipError_t launch_tap_sh(const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream) {
    if (t.family == BF16_ROWREUSE) return t.tm == 1 ? launch_tm_rowreuse<SH, 1>(p, stream) : launch_tm_rowreuse<SH, 2>(p, stream);
    if (t.nh == 2) return launch_tm<SH, 1, 2>(p, t.kc32, stream);            // 128 positions x 128 couts
    return t.tm == 1 ? launch_tm<SH, 1, 1>(p, t.kc32, stream)
         : t.tm == 2 ? launch_tm<SH, 2, 1>(p, t.kc32, stream) : launch_tm<SH, 4, 1>(p, t.kc32, stream);
}
hipError_t launch_bf16_tap(int sh, const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream) {
    return sh == 16 ? launch_tap_sh<16>(t, p, stream) : launch_tap_sh<32>(t, p, stream);
}

#ifdef S3R_ABLATE
int read_timeline_tap(unsigned long long* out, int nblocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(s3r_timeline_h), sizeof(unsigned long long) * 8 * (size_t)nblocks) == hipSuccess ? nblocks : -1;
}
#endif

}  // namespace s3r

