// bf16 MFMA path (BASELINE.json configs[2]): 2D/3D convolution and transposed convolution as an implicit
// GEMM on the bf16 matrix cores, bf16 activations in CHANNELS-LAST layout with a zero halo, fp32
// accumulation, folded-BN affine + activation + bf16 rounding fused into the epilogue.
//
//   D[pos][cout] = sum_{chunk, tap, c} X[b(pos)][in(pos) + tap][chunk*32 + c] * Wp[(chunk*T + tap)][cout][c]
//
//   GEMM M = B*Nd*Nh*Nw positions (A operand: gathered activations), N = Cout (B operand: weights),
//   K = Cin*T in K tiles of ONE tap x 32 channels = 64 contiguous bytes per position.
//
// Why channels-last here when the fp32 path is NCHW: the bf16 MFMA takes 8 consecutive k per lane, i.e. 16
// contiguous BYTES of one position's channel vector — one ds_read_b128 — whereas the fp32 MFMA takes one k
// per lane and wants position-contiguous rows.  The output falls out channels-last as well.
//
// Two matrix instructions, one code path (template parameter SH; MI355X_MICROARCH.md "DVFS give-back" item 7 and
// cdna_hip_programming.md rule 28: the chip can hold a higher clock on one shape than on the other, so both are
// built at the same per-wave output tile and the faster BY WALL ON RANDOM DATA is kept):
//   SH = 32: v_mfma_f32_32x32x16_bf16  lane = (row li = lane & 31, k group lk = lane >> 5), 16 acc registers
//   SH = 16: v_mfma_f32_16x16x32_bf16  lane = (row li = lane & 15, k group lk = lane >> 4),  4 acc registers
// A wave owns 32*TM positions x 64*NH couts as MFMA tiles of MT x MT (MT = SH).  The MFMA is issued with the
// WEIGHTS as its A operand, so D = [cout][position]: a lane owns ONE position per position tile, and the pack
// kernel permutes the weight rows so that the couts a lane holds are CONSECUTIVE (16 per 32 couts for SH = 32, 16 per
// 64 couts for SH = 16): 32 contiguous bytes of the channels-last output per group, one output offset per position,
// and the fused head's reduction over the couts stays inside the lane (+ one or two cross-lane exchanges).
//
// LDS images (per K tile): As[pos][slots x 16 B], Bs[cout row][slots x 16 B], slot = kgroup ^ swz(row).  A plain
// image makes every ds_read_b128 lane group hit the same 16-byte column of several rows; the XOR spreads them
// (swz below: conflict-free for BOTH instruction shapes' lane -> (row, k group) maps).  Both operands arrive by
// LDS-DMA (16 B per lane, lane-linear destination), so the swizzle is applied on the SOURCE side: a lane
// fetches channel group slot ^ swz(row) of its position; weights are stored pre-swizzled by the pack kernel.
//
// Workgroup: 4 waves along M.  Per-position input / output offsets are decoded once per workgroup into LDS.
//
// Four gathers of the A operand behind one epilogue (epilogue_h below), in two translation units.  This header holds what more
// than one unit needs: the MFMA interface, the epilogue, the LDS swizzle, the workgroup order and position decode of the tiled
// kernels, and the table of tile codes.
//   s3r_bf16_tap.hip     per-tap gather: conv_bf16_kernel (K tile = one tap x 32 or 64 channels), launch_tm;
//                        row reuse: conv_bf16r_kernel fetches a row group once per kw taps; rowreuse_rows, launch_tm_rowreuse
//   s3r_bf16_plane.hip   plane reuse (stride 1): conv_bf16p_kernel fetches a plane once per kh*kw taps; plane_rows, launch_tm_plane;
//                        row-persistent (e2 at large batches): conv_bf16w_kernel, rows_strips, launch_rows
//   s3r_conv_bf16.hip    the dispatch unit: tile and split-K choice, scratch size, launch_conv_bf16, the split-K finish kernel,
//                        the weight pack kernel
// Why the row kernels have no unit of their own: load_ep / store_ep take the workgroup's cout count as an argument, and in a
// code object where every caller passes 64 the compiler propagates the constant into them and emits a shorter prologue — other
// instructions than the ones that were measured.  Each row kernel therefore shares its unit with a kernel that also has 128-cout
// workgroups (NH = 2), as all four did in one file.
#pragma once
#include "s3r_kernels.h"

#ifndef S3R_PRIO_EDGE
#define S3R_PRIO_EDGE 3               // wave priority of the prologue / epilogue phases (the K loops run at 0)
#endif

namespace s3r {

#ifdef S3R_ABLATE   // diagnostic builds only: S3R_ABL=1 no epilogue stores, 2 one K tile only, 3 no DMA in the loop
#define S3R_ABLH(p, m) ((p).debug == (m))
#else
#define S3R_ABLH(p, m) false
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

#define S3R_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};      // one v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, v);
}

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds_dst, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, S3R_LDS_PTR(lds_dst), 16, voffset, soffset, 0, 0);
}

// ---- the two matrix instructions behind one interface
template <int SH> struct Mf;
template <> struct Mf<32> {
    static constexpr int MT = 32;      // rows / columns of one MFMA tile
    static constexpr int KS = 16;      // k per instruction
    static constexpr int NK = 2;       // k groups of 8 per instruction = lane groups
    typedef f32x16 acc_t;
    static constexpr int NACC = 16;
};
template <> struct Mf<16> {
    static constexpr int MT = 16;
    static constexpr int KS = 32;
    static constexpr int NK = 4;
    typedef f32x4 acc_t;
    static constexpr int NACC = 4;
};
template <int SH>
__device__ __forceinline__ typename Mf<SH>::acc_t mma(const bf16x8& w, const bf16x8& a, const typename Mf<SH>::acc_t& c) {
    if constexpr (SH == 32) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, a, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0);
}
// The 16 CONSECUTIVE couts a lane holds in one group: element r (0..15) of group gi of position tile `acc[..]`.
//   SH = 32: acc[gi = 32-cout tile][r]                 couts  gi*32 + 16*lk + r      (2 groups per 64 couts)
//   SH = 16: acc[r >> 2 = 16-cout tile][r & 3]         couts          16*lk + r      (1 group  per 64 couts)
template <int SH> constexpr int groups_per_64() { return SH == 32 ? 2 : 1; }
template <int SH> __device__ __forceinline__ int group_cout(int gi, int lk) { return SH == 32 ? gi * 32 + 16 * lk : 16 * lk; }
template <int SH>
__device__ __forceinline__ float acc_at(const typename Mf<SH>::acc_t (&t)[64 / Mf<SH>::MT], int gi, int r) {
    if constexpr (SH == 32) return t[gi][r]; else return t[r >> 2][r & 3];
}

constexpr int HKC = 32;    // channels per K tile
constexpr int HBN = 64;    // couts per workgroup

// element offset of output position (b, pd, ph, pw) [of parity class (rd, rh, rw) for a transposed conv] in p.y
__device__ __forceinline__ int out_offset(const ConvParamsH& p, int b, int pd, int ph, int pw, int rd, int rh, int rw) {
    const int ostep = p.transposed ? 2 : 1;
    int ye = b * p.y_bs + p.y_org + (pd * p.y_ds + ph * p.y_hs + pw * p.y_ws) * ostep;
    if (p.transposed) ye += rd * p.y_ds + rh * p.y_hs + rw * p.y_ws;
    return ye;
}

// Workgroup order of the tiled kernels: blockIdx.x -> (bid = tile index, cls = output-parity class).
// Convolutions: each XCD (blocks b, b+8, ... share one) walks a contiguous run of tiles.
// Transposed convolutions: the grid is 8 x as long and an XCD walks its run of tiles with the 8 output-parity classes
// of a tile BACK TO BACK — they read the same input tile, so seven of the eight reads are hits in that XCD's L2.
// With the class on blockIdx.y instead (all tiles of class 0, then of class 1, ...) every class streamed the whole
// input from HBM again once it outgrew the caches: d3 at B = 256 fetched 1.67 GB per launch for a 382 MB input.
__device__ __forceinline__ void wg_order(int transposed, int& bid, int& cls) {
    if (transposed) {
        const int nwg = gridDim.x >> 3;
        const int item = (bid & 7) * nwg + (bid >> 3);
        bid = item >> 3;
        cls = item & 7;
    } else {
        const int nwg = gridDim.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
}

// position n of the GEMM's M axis -> (batch, depth, row, column); S = p.Nd * p.Nh * p.Nw, computed by the caller
struct PosH { int b, pd, ph, pw; };
__device__ __forceinline__ PosH decode_pos(const ConvParamsH& p, int n, int S) {
    const int b = p.dS.div(n);
    int rem = n - b * S;
    const int pd = p.dHW.div(rem);
    rem -= pd * p.Nh * p.Nw;
    const int ph = p.dW.div(rem);
    return {b, pd, ph, rem - ph * p.Nw};
}

// Epilogue shared by the bf16 kernels.  D is [cout][position]: lane (li, lk) owns position row
// wave*32*TM + pt*MT + li of the tile for each position tile pt, and per 64-cout block the 16-cout groups of
// group_cout() (the pack kernel permutes the weight rows to make them consecutive).  A lane therefore stores 32
// contiguous bytes per group, needs one output offset per position, and the fused head's reduction over the couts
// stays inside the lane (then one exchange per lane-group bit).
// ep = LDS [3][64]: folded-BN scale, shift and head weight of the workgroup's 64 couts; yoff[row] = the
// position's output element offset (-1: past the end).
constexpr int EP_BYTES = 3 * 64 * 4;
constexpr int ST_ROW = 144;     // staging row: 128 payload bytes + 16 (rows 9 sixteen-byte slots apart: conflict-free b128 writes)

// The per-cout constants are LOADED first thing in the kernel (their latency hides behind the first operand
// fetch) and only written to LDS after the main loop: nothing before the epilogue waits for them.
struct EpRegs { float sc, sf, hw; };

__device__ __forceinline__ EpRegs load_ep(const ConvParamsH& p, int tid, int n0, int nco = 64) {
    EpRegs e = {1.f, 0.f, 0.f};
    if (tid < nco) {
        const int co = n0 + tid;
        const bool ok = co < p.Cout;
        e.sc = (ok && p.scale) ? p.scale[co] : 1.f;
        e.sf = (ok && p.shift) ? p.shift[co] : 0.f;
        e.hw = (ok && p.head_w) ? p.head_w[co] : 0.f;
    }
    return e;
}

__device__ __forceinline__ void store_ep(const EpRegs& e, float* ep, int tid, int nco = 64) {
    if (tid < nco) {                               // [64-cout half][scale | shift | head weight][64]
        float* q = ep + (tid >> 6) * 192 + (tid & 63);
        q[0] = e.sc;
        q[64] = e.sf;
        q[128] = e.hw;
    }
    __syncthreads();
}

// acc: the wave's accumulators of ONE 64-cout block: [position tile][cout tile of MT].
// NOSIG: the caller guarantees p.act != sigmoid (the per-element test of the wave-uniform flag compiles to a branch per
// value: 64 of them per unit)
template <int SH, int TM, bool HEAD, bool NOSIG = false>
__device__ __forceinline__ void epilogue_h(const ConvParamsH& p, typename Mf<SH>::acc_t (&acc)[32 * TM / Mf<SH>::MT][64 / Mf<SH>::MT],
                                           const int* yoff, const float* ep, char* stage, int wave, int li, int lk, int m0,
                                           int n0, int cls, int kz, int bm, int ybase = 0) {
    constexpr int MT = Mf<SH>::MT;
    constexpr int NPT = 32 * TM / MT;             // position tiles per wave
    constexpr int PPU = 32 / MT;                  // position tiles per 32-row staging unit (1 or 2)
    constexpr int GL = groups_per_64<SH>();       // 16-cout groups a lane holds per 64 couts
    // `stage`: this wave's 32 x ST_ROW bytes of the (now idle) operand buffers.  A lane holds 32 B (bf16) /
    // 64 B (fp32 slab) pieces of ONE position; stored as they stand, a wave instruction would touch 16-32 rows with
    // 16-byte pieces.  Staged through LDS, lanes 8r..8r+7 write the 128 contiguous bytes of row r: every store
    // instruction covers eight whole 128-byte lines.
    const int lane = threadIdx.x & 63;
    const int srow = lane >> 3, spiece = lane & 7;
    if (p.ksplit > 1) {
        // split-K: fp32 partial sums [cls][kz][position][CoutPad]; conv_finish_bf16 reduces in kz order.
        const int mpad = p.m_tiles * bm;
        if constexpr (SH == 32) {
            // one staging unit = 32 positions x 32 couts fp32 (128-byte rows): lane (li, lk) holds couts ch*32 + 16 lk + r
            float* __restrict__ slab = p.part + ((size_t)(cls * p.ksplit + kz) * mpad + m0) * p.CoutPad + n0 + 4 * spiece;
#pragma unroll
            for (int u = 0; u < TM; ++u)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 t = {acc[u][ch][4 * j], acc[u][ch][4 * j + 1], acc[u][ch][4 * j + 2], acc[u][ch][4 * j + 3]};
                        *reinterpret_cast<f32x4*>(stage + li * ST_ROW + lk * 64 + j * 16) = t;
                    }
                    if (S3R_ABLH(p, 1)) continue;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = i * 8 + srow;
                        const f32x4 t = *reinterpret_cast<const f32x4*>(stage + r * ST_ROW + spiece * 16);
                        *reinterpret_cast<f32x4*>(slab + (size_t)(wave * 32 * TM + u * 32 + r) * p.CoutPad + ch * 32) = t;
                    }
                }
        } else {
            // one staging unit = ONE position tile: 16 positions x 64 couts fp32 (256-byte rows + 16: 4352 B of the wave's
            // 4608).  EVERY lane writes (its 16 couts 16 lk + 4 ct + r of position li) — a unit in which only half the
            // lanes stage data would put the writes in a divergent branch, and nothing orders the other lanes' reads
            // behind it.  Read back as 4 rows x 256 contiguous bytes per store instruction.
            constexpr int SR = 272;
            float* __restrict__ slab = p.part + ((size_t)(cls * p.ksplit + kz) * mpad + m0) * p.CoutPad + n0 + 4 * (lane & 15);
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(stage + li * SR + lk * 64 + j * 16) = acc[pt][j];
                if (S3R_ABLH(p, 1)) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = i * 4 + (lane >> 4);
                    const f32x4 t = *reinterpret_cast<const f32x4*>(stage + r * SR + (lane & 15) * 16);
                    *reinterpret_cast<f32x4*>(slab + (size_t)(wave * 32 * TM + pt * MT + r) * p.CoutPad) = t;
                }
            }
        }
        return;
    }
    // ReLU / identity as ONE v_max against a wave-uniform floor; sigmoid (rare) behind a wave-uniform flag
    const float lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    const bool sig = !NOSIG && p.act == ACT_SIGMOID;
    if constexpr (HEAD) {
        int ye[NPT];
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) ye[pt] = yoff[wave * 32 * TM + pt * MT + li] + ybase;   // (-1 + 0: still 'none')
        // fused pointwise head (conv -> 1x1x1 conv to ONE channel + activation; the workgroup's 64-cout tile
        // is the whole channel axis): 16 * GL FMAs in the lane, an exchange per lane-group bit, one fp32 store per
        // position.  The conv's own bf16 output — the largest activation of the network — is never written.
        float t[NPT];
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) t[pt] = 0.f;
#pragma unroll
        for (int gi = 0; gi < GL; ++gi) {
            const float* e = ep + group_cout<SH>(gi, lk);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(e + 4 * q);
                const f32x4 sf = *reinterpret_cast<const f32x4*>(e + 64 + 4 * q);
                const f32x4 hw = *reinterpret_cast<const f32x4*>(e + 128 + 4 * q);
#pragma unroll
                for (int pt = 0; pt < NPT; ++pt) {
                    t[pt] = fmaf(fmaxf(fmaf(acc_at<SH>(acc[pt], gi, 4 * q + 0), sc.x, sf.x), lo), hw.x, t[pt]);
                    t[pt] = fmaf(fmaxf(fmaf(acc_at<SH>(acc[pt], gi, 4 * q + 1), sc.y, sf.y), lo), hw.y, t[pt]);
                    t[pt] = fmaf(fmaxf(fmaf(acc_at<SH>(acc[pt], gi, 4 * q + 2), sc.z, sf.z), lo), hw.z, t[pt]);
                    t[pt] = fmaf(fmaxf(fmaf(acc_at<SH>(acc[pt], gi, 4 * q + 3), sc.w, sf.w), lo), hw.w, t[pt]);
                }
            }
        }
        const float hsc = p.head_scale ? p.head_scale[0] : 1.f, hsf = p.head_shift ? p.head_shift[0] : 0.f;
        float* __restrict__ y = reinterpret_cast<float*>(p.y);
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            float v = t[pt] + __shfl_xor(t[pt], 32, 64);          // fixed order: (lk) + (lk ^ 2 | lk ^ 1 for SH = 32) ...
            if constexpr (SH == 16) v += __shfl_xor(v, 16, 64);
            if (lk == 0 && ye[pt] >= 0) {
                v = fmaf(v, hsc, hsf);
                if (p.head_act == ACT_RELU) v = fmaxf(v, 0.f);
                else if (p.head_act == ACT_SIGMOID) v = 1.f / (1.f + __expf(-v));
                y[ye[pt]] = v;
            }
        }
        return;
    }
    unsigned short* __restrict__ y = reinterpret_cast<unsigned short*>(p.y);
    const bool wide = (p.Cout & 7) == 0;          // 16-byte stores need the channel axis in whole groups of 8
#pragma unroll
    for (int u = 0; u < TM; ++u) {                // one staging unit = 32 positions x 64 couts bf16 (128-byte rows)
#pragma unroll
        for (int q = 0; q < PPU; ++q)
#pragma unroll
            for (int gi = 0; gi < GL; ++gi)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int cl = group_cout<SH>(gi, lk) + 8 * g;      // (tile-local) cout of element 8g of the group
                    const f32x4 sc0 = *reinterpret_cast<const f32x4*>(ep + cl);
                    const f32x4 sc1 = *reinterpret_cast<const f32x4*>(ep + cl + 4);
                    const f32x4 sf0 = *reinterpret_cast<const f32x4*>(ep + 64 + cl);
                    const f32x4 sf1 = *reinterpret_cast<const f32x4*>(ep + 64 + cl + 4);
                    const float sc[8] = {sc0.x, sc0.y, sc0.z, sc0.w, sc1.x, sc1.y, sc1.z, sc1.w};
                    const float sf[8] = {sf0.x, sf0.y, sf0.z, sf0.w, sf1.x, sf1.y, sf1.z, sf1.w};
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        v[r] = fmaf(acc_at<SH>(acc[u * PPU + q], gi, 8 * g + r), sc[r], sf[r]);
                        v[r] = sig ? __builtin_amdgcn_rcpf(1.f + __expf(-v[r])) : fmaxf(v[r], lo);
                    }
                    const uint4 pk = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]),
                                      pack_bf16(v[6], v[7])};
                    *reinterpret_cast<uint4*>(stage + (q * MT + li) * ST_ROW + cl * 2) = pk;
                }
        if (S3R_ABLH(p, 1)) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = i * 8 + srow;
            const int ye = yoff[wave * 32 * TM + u * 32 + r] + ybase;     // (ybase: a persistent kernel's per-step offset)
            const int co = n0 + 8 * spiece;
            const uint4 pk = *reinterpret_cast<const uint4*>(stage + r * ST_ROW + spiece * 16);
            if (ye < 0 || co >= p.Cout) continue;
            unsigned short* dst = y + (size_t)ye + co;
            if (wide) {
                *reinterpret_cast<uint4*>(dst) = pk;
            } else {
                const unsigned w[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (co + e < p.Cout) dst[e] = (unsigned short)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            }
        }
    }
}

// LDS rows are KC channels = KC*2 bytes = KC/8 sixteen-byte slots; slot = kgroup ^ swz(row) keeps every
// ds_read_b128 lane group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... of each 32) on 16 distinct 16-byte slots of
// the 256-byte bank row, for BOTH lane maps (SH = 32: 32 consecutive rows, one k group per lane half; SH = 16: 16
// consecutive rows x 4 k groups):
//   128-byte rows (2 rows per bank row): (row >> 1) & 7;
//   64-byte rows (4 rows per bank row): (-(row >> 2)) & 3 — for SH = 16 a lane group mixes k groups g and g + 1 on rows
//   {0-3, 12-15} and {4-11}: with t = (row >> 2) & 3 the four slots (g ^ f(0), g ^ f(3), (g+1) ^ f(1), (g+1) ^ f(2)) are
//   distinct for f = (0, 3, 2, 1) (the plain f(t) = t collides); any bijection serves SH = 32.
template <int KC>
__device__ __host__ __forceinline__ int swz(int row) { return KC == 64 ? (row >> 1) & 7 : (0 - (row >> 2)) & 3; }

constexpr int NPA_MAX = 10;    // row-reuse kernel: 16-position A pieces per wave per group, upper bound (registers)

// ---- the tile codes (s3r_conv_desc.tile; launch_conv_bf16's tm), one row each.  tm: 32 x tm positions per wave (128 x tm per
// workgroup of four waves); kc32: 32-channel K tiles even where 64 are possible (the plane family: instead of 64); nh: 64-cout
// halves per workgroup
enum Bf16Family { BF16_TAP, BF16_PLANE, BF16_ROWREUSE, BF16_ROWS };
struct Bf16Tile { int code, family, tm, kc32, nh; };
constexpr Bf16Tile kBf16Tiles[] = {
    {1, BF16_TAP, 1, 0, 1}, {2, BF16_TAP, 2, 0, 1}, {4, BF16_TAP, 4, 0, 1}, {3, BF16_TAP, 1, 0, 2},
    {17, BF16_TAP, 1, 1, 1}, {18, BF16_TAP, 2, 1, 1}, {20, BF16_TAP, 4, 1, 1}, {19, BF16_TAP, 1, 1, 2},
    {5, BF16_PLANE, 1, 0, 1}, {6, BF16_PLANE, 2, 0, 1}, {21, BF16_PLANE, 1, 1, 1}, {22, BF16_PLANE, 2, 1, 1}, {23, BF16_PLANE, 2, 1, 2},
    {9, BF16_ROWREUSE, 1, 1, 1}, {10, BF16_ROWREUSE, 2, 1, 1}, {40, BF16_ROWS, 2, 1, 1}};
inline const Bf16Tile* bf16_tile(int code) {      // null: no such code
    for (const Bf16Tile& t : kBf16Tiles)
        if (t.code == code) return &t;
    return nullptr;
}

// ---- the units' launchers (sh = 16 | 32: the matrix instruction; t: the tile's row; each unit picks its template instantiation
// from (sh, t.family, t.tm, t.kc32, t.nh)) and what conv_bf16_pick_tm asks them
hipError_t launch_bf16_tap(int sh, const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream);      // BF16_TAP, BF16_ROWREUSE
int rowreuse_rows(const ConvParamsH& p, int bm);
hipError_t launch_bf16_plane(int sh, const Bf16Tile& t, const ConvParamsH& p, hipStream_t stream);    // BF16_PLANE, BF16_ROWS
int plane_rows(const ConvParamsH& p, int bm, int kc);
int rows_strips(const ConvParamsH& p);
// split-K finish of a launch with bm-position tiles (s3r_conv_bf16.hip); a no-op for p.ksplit == 1
hipError_t launch_finish_bf16(const ConvParamsH& p, int bm, hipStream_t stream);
#ifdef S3R_ABLATE   // S3R_ABL=7: each timeline kernel's unit reads its own buffer; -> nblocks, -1 on error
int read_timeline_tap(unsigned long long* out, int nblocks);
int read_timeline_plane(unsigned long long* out, int nblocks);
#endif

}  // namespace s3r
