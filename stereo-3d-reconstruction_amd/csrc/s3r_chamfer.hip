// Chamfer distance forward and backward for Stereo2Point (the op the reference builds as extensions/chamfer_dist,
// /root/reference/README.md:64-65; its source is not in the mount).
//   dist1[b,i] = min_j |p[b,i] - q[b,j]|^2,  idx1[b,i] = argmin_j (first minimum)
//   dist2[b,j] = min_i |p[b,i] - q[b,j]|^2,  idx2[b,j] = argmin_i
// K = 3, so this is fp32 VALU work, not matrix-core work.  A workgroup owns 64*QPT query points; the other cloud is
// staged through LDS as (x, y, z, -) quads, 2048 points (32 KiB) per pass — the whole cloud at the BASELINE size, one
// barrier pair per launch — and every lane reads a candidate at the same address (LDS broadcast, one ds_read_b128
// per candidate per wave).  The four waves each scan a QUARTER of the staged candidates for the same queries (QPT
// independent chains per thread), and the four partial minima are merged through LDS with an explicit index
// comparison on ties, so the result keeps the first (lowest) index exactly as a sequential scan does.  The distance
// is ((dx*dx + dy*dy) + dz*dz) with contraction disabled: bit-identical to the oracle.  Both directions run in ONE
// launch (blockIdx.z): 1024 workgroups at the BASELINE size, 4 waves per SIMD (r01: two launches of 512, staging
// passes of 1024 with a barrier pair each, 25 "TFLOP/s" at 8 flops per pair).
//
// Instruction budget (the roof of this op is VALU issue: 78.6 T lane-instructions/s): a pair costs 3 sub + 3 mul +
// 2 add = 8 instructions for its distance — the floor of the oracle's formula; tracking (min, argmin) per pair would
// cost 3 more (v_cmp + 2 v_cndmask).  The candidates are taken in BLOCKS of 8: the block's minimum is 3 v_min3_f32 +
// 1 v_min (0.5 per pair) and the argmin is only looked for when the block minimum beats the running best (strictly:
// an equal distance later in the scan never replaces an earlier index) — a branch a wave takes ~ln(M) times per
// query, skipped by s_cbranch_execz otherwise: ~8.6 instructions per pair.  The file is built with
// -fno-slp-vectorize: plain -O3 packs the chains into v_pk_*_f32, which issue several times slower on gfx950.
// (Fetching the candidates by SCALAR loads instead — the range is wave-uniform — measured the same 66 us for 1, 2 and
// 4 queries per thread: every wave then waits out a scalar-cache miss per block, in lock-step with its neighbours.)
//
// Backward (chamfer_backward_kernel, s3r_chamfer_backward): d(sum g1 dist1 + sum g2 dist2) / d(p, q) as a GATHER with a fixed
// summation order — no atomics, no scratch, the same bits on every run, for every batch split and at every address:
//   grad_p[i] = a_i (p_i - q_idx1[i]) + sum_{j ascending, idx2[j] == i} c_j (p_i - q_j),   a = 2 g1, c = 2 g2 (exact)
//   grad_q[j] = c_j (q_j - p_idx2[j]) + sum_{i ascending, idx1[i] == j} a_i (q_j - p_i)
// per component: the difference is rounded, then the product, the accumulator starts as the own term and the scattered terms are
// added one at a time (contraction off, as in dist3).  A thread OWNS its target point (BQPT = 1 of them; coordinates and accumulators in
// registers) and sees every source in ascending order, so the four waves of a workgroup own DIFFERENT targets (256 * BQPT per
// workgroup) — slicing the sources over the waves, as the forward does, would turn the sequential sum into a tree.  The source side
// is staged through LDS in passes of 2048: the index array the sources scatter by (idx2 for grad_p, idx1 for grad_q), and (x, y, z,
// weight) quads.  The scan reads ONLY the indices — a wave-uniform address: LDS broadcast, one ds_read_b128 per four — and pays one
// v_cmp_eq per (owned target, source); the quad is fetched inside the match branch.  Every source scatters exactly one term, so a
// target receives one on average — but the branch is a WAVE's: a block of 8 sources holds one for some of a wave's 64 targets with
// probability 8 * 64 / 2048 = 1/4.  Every source on ONE target is still correct and in order, only slow.
#include "s3r_kernels.h"
#include <cstdlib>

namespace s3r {

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int CH_TILE = 2048;   // candidates staged per pass (4 slices of 512): 32 KiB
constexpr int QPT = 2;          // query points per thread
constexpr int CBLK = 8;         // candidates per block (one min tree, one rare argmin search)

__device__ __forceinline__ float dist3(float px, float py, float pz, const v4f& v) {
#pragma clang fp contract(off)   // (dx*dx + dy*dy) + dz*dz with three roundings each, as the oracle computes it
    const float dx = px - v[0], dy = py - v[1], dz = pz - v[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// direction 0: queries p (N points) against candidates q (M points) -> d1 / i1; direction 1: the roles swapped
__global__ __launch_bounds__(256) void chamfer_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                      float* __restrict__ d1, float* __restrict__ d2, int* __restrict__ i1,
                                                      int* __restrict__ i2, int N, int M) {
    __shared__ v4f qs[CH_TILE];
    __shared__ float rd[3][64 * QPT];
    __shared__ int ri[3][64 * QPT];
    const int dir = blockIdx.z;
    const int nq = dir ? M : N, nc = dir ? N : M;                 // queries / candidates of this direction
    if (blockIdx.x * 64 * QPT >= nq) return;                       // (the grid covers the larger cloud; block-uniform)
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i0 = (blockIdx.x * 64 + lane) * QPT;
    const float* __restrict__ pb = (dir ? q : p) + (size_t)b * nq * 3;
    const float* __restrict__ qb = (dir ? p : q) + (size_t)b * nc * 3;
    float* __restrict__ dist = dir ? d2 : d1;
    int* __restrict__ idx = dir ? i2 : i1;
    float px[QPT], py[QPT], pz[QPT], best[QPT];
    int besti[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int i = min(i0 + k, nq - 1);
        px[k] = pb[i * 3 + 0]; py[k] = pb[i * 3 + 1]; pz[k] = pb[i * 3 + 2];
        best[k] = __builtin_inff();
        besti[k] = 0;
    }
    for (int j0 = 0; j0 < nc; j0 += CH_TILE) {
        const int cnt = min(CH_TILE, nc - j0);
        if (j0) __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const float* s = qb + (size_t)(j0 + t) * 3;
            v4f v = {s[0], s[1], s[2], 0.f};
            qs[t] = v;
        }
        __syncthreads();
        // this wave's quarter of the staged candidates, in index order
        const int per = (cnt + 3) >> 2;
        const int t_begin = min(cnt, slice * per), t_end = min(cnt, t_begin + per);
        int t = t_begin;
        for (; t + CBLK <= t_end; t += CBLK) {
            float d[QPT][CBLK];
#pragma unroll
            for (int e = 0; e < CBLK; ++e) {
                const v4f v = qs[t + e];
#pragma unroll
                for (int k = 0; k < QPT; ++k) d[k][e] = dist3(px[k], py[k], pz[k], v);
            }
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const float m = __builtin_fminf(__builtin_fminf(__builtin_fminf(__builtin_fminf(d[k][0], d[k][1]), d[k][2]),
                                                                __builtin_fminf(__builtin_fminf(d[k][3], d[k][4]), d[k][5])),
                                                __builtin_fminf(d[k][6], d[k][7]));
                if (m < best[k]) {                 // rare: ~ln(M) times per query
                    int e_min = CBLK - 1;
#pragma unroll
                    for (int e = CBLK - 2; e >= 0; --e) e_min = d[k][e] == m ? e : e_min;    // the FIRST candidate at the minimum
                    best[k] = m;
                    besti[k] = j0 + t + e_min;
                }
            }
        }
        for (; t < t_end; ++t) {                   // the quarter's last < 8 candidates
            const v4f v = qs[t];
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const float dd = dist3(px[k], py[k], pz[k], v);
                if (dd < best[k]) { best[k] = dd; besti[k] = j0 + t; }
            }
        }
    }
    // merge the four slices' minima: strictly-smaller wins, equal distances keep the lowest candidate index
    // (within a staging pass the slices are in index order; across passes an earlier pass always has lower indices
    // but may sit in ANY slice, hence the explicit index comparison on ties)
    if (slice > 0) {
#pragma unroll
        for (int k = 0; k < QPT; ++k) { rd[slice - 1][lane * QPT + k] = best[k]; ri[slice - 1][lane * QPT + k] = besti[k]; }
    }
    __syncthreads();
    if (slice == 0) {
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            float d = best[k];
            int bi = besti[k];
#pragma unroll
            for (int s2 = 0; s2 < 3; ++s2) {
                const float od = rd[s2][lane * QPT + k];
                const int oi = ri[s2][lane * QPT + k];
                if (od < d || (od == d && oi < bi)) { d = od; bi = oi; }
            }
            if (i0 + k < nq) {
                dist[(size_t)b * nq + i0 + k] = d;
                idx[(size_t)b * nq + i0 + k] = bi;
            }
        }
    }
}

hipError_t launch_chamfer(const float* p, const float* q, float* d1, float* d2, int* i1, int* i2, int B, int N,
                          int M, hipStream_t s) {
    constexpr int PER_WG = 64 * QPT;
    const int big = N > M ? N : M;
    hipLaunchKernelGGL(chamfer_kernel, dim3((big + PER_WG - 1) / PER_WG, B, 2), dim3(256), 0, s, p, q, d1, d2, i1, i2, N, M);
    return hipGetLastError();
}

constexpr int BQPT = 1;         // target points per thread of the backward: the scan is bound by ONE wave's instruction issue (compare,
                                // mask OR, branch), not by throughput, so the fewest targets per wave — the most waves — wins:
                                // 50 us at 1, 83 at 2, 130 at 4 (B = 32, N = M = 2048; docs/LAB_NOTES.md)
constexpr int BW_BLK = 8;       // staged indices per block of the backward scan (two ds_read_b128, one match test per target)
typedef int v4i __attribute__((ext_vector_type(4)));

// w (t - s) per component: the difference rounded, then the product
__device__ __forceinline__ void bw_term(float tx, float ty, float tz, const v4f& s, float& ux, float& uy, float& uz) {
#pragma clang fp contract(off)
    const float dx = tx - s[0], dy = ty - s[1], dz = tz - s[2];
    ux = s[3] * dx; uy = s[3] * dy; uz = s[3] * dz;
}

__device__ __forceinline__ void bw_add(float& gx, float& gy, float& gz, float tx, float ty, float tz, const v4f& s) {
#pragma clang fp contract(off)
    float ux, uy, uz;
    bw_term(tx, ty, tz, s, ux, uy, uz);
    gx = gx + ux; gy = gy + uy; gz = gz + uz;
}

// direction 0: targets p (N points), sources q (M points): own index idx1, scattered by idx2 -> grad_p; direction 1: the roles swapped
__global__ __launch_bounds__(256) void chamfer_backward_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                               const int* __restrict__ i1, const int* __restrict__ i2,
                                                               const float* __restrict__ g1, const float* __restrict__ g2,
                                                               float* __restrict__ gp, float* __restrict__ gq, int N, int M) {
    __shared__ v4f ss[CH_TILE];                                    // a source's (x, y, z, weight)
    __shared__ __attribute__((aligned(16))) int si[CH_TILE + BW_BLK];      // ... and the target it scatters to (+ one block: the scan reads ahead)
    const int dir = blockIdx.z;
    float* __restrict__ out = dir ? gq : gp;
    if (!out) return;                                              // this direction is not asked for (block-uniform)
    const int nt = dir ? M : N, ns = dir ? N : M;                  // targets / sources of this direction
    if (blockIdx.x * 256 * BQPT >= nt) return;                      // (the grid covers the larger cloud; block-uniform)
    const size_t b = blockIdx.y;
    const float* __restrict__ tb = (dir ? q : p) + b * nt * 3;
    const float* __restrict__ sb = (dir ? p : q) + b * ns * 3;
    const int* __restrict__ own = (dir ? i2 : i1) + b * nt;        // a target's own nearest source
    const int* __restrict__ sct = (dir ? i1 : i2) + b * ns;        // a source's nearest target
    const float* __restrict__ gown = dir ? g2 : g1;                // NULL: all zeros (the same arithmetic with weight 0)
    const float* __restrict__ gsct = dir ? g1 : g2;
    if (gown) gown += b * nt;
    if (gsct) gsct += b * ns;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * BQPT;
    float tx[BQPT], ty[BQPT], tz[BQPT], ax[BQPT], ay[BQPT], az[BQPT];
    int tid[BQPT];
#pragma unroll
    for (int k = 0; k < BQPT; ++k) {
        tid[k] = i0 + k;                                           // (>= nt: no store; whatever it matches stays in registers)
        const int i = min(i0 + k, nt - 1);
        tx[k] = tb[i * 3 + 0]; ty[k] = tb[i * 3 + 1]; tz[k] = tb[i * 3 + 2];
        const int o = min(max(own[i], 0), ns - 1);                 // a garbage index never reads outside the cloud
        const v4f s = {sb[o * 3 + 0], sb[o * 3 + 1], sb[o * 3 + 2], gown ? 2.f * gown[i] : 0.f};
        bw_term(tx[k], ty[k], tz[k], s, ax[k], ay[k], az[k]);      // the accumulator starts as the own term
    }
    for (int j0 = 0; j0 < ns; j0 += CH_TILE) {
        const int cnt = min(CH_TILE, ns - j0);
        const int padded = (cnt + BW_BLK - 1) / BW_BLK * BW_BLK + BW_BLK;      // <= CH_TILE + BW_BLK: whole blocks, and the block read ahead
        if (j0) __syncthreads();
        for (int t = threadIdx.x; t < padded; t += 256) {
            if (t < cnt) {
                const float* s = sb + (size_t)(j0 + t) * 3;
                const v4f v = {s[0], s[1], s[2], gsct ? 2.f * gsct[j0 + t] : 0.f};
                ss[t] = v;
                si[t] = sct[j0 + t];
            } else {
                si[t] = -1;                                        // no target has a negative index
            }
        }
        __syncthreads();
        v4i na = *reinterpret_cast<const v4i*>(&si[0]), nb = *reinterpret_cast<const v4i*>(&si[4]);
        for (int t = 0; t < cnt; t += BW_BLK) {                    // every thread, every source, ascending
            const v4i ia = na, ib = nb;
            na = *reinterpret_cast<const v4i*>(&si[t + BW_BLK]);   // the next block's indices are in flight during this block's compares
            nb = *reinterpret_cast<const v4i*>(&si[t + BW_BLK + 4]);
            const int id[BW_BLK] = {ia[0], ia[1], ia[2], ia[3], ib[0], ib[1], ib[2], ib[3]};
#pragma unroll
            for (int k = 0; k < BQPT; ++k) {
                bool any = false;
#pragma unroll
                for (int e = 0; e < BW_BLK; ++e) any |= id[e] == tid[k];
                if (any) {                                         // about one scattered term per target: a quarter of a wave's blocks
#pragma unroll
                    for (int e = 0; e < BW_BLK; ++e)
                        if (id[e] == tid[k]) bw_add(ax[k], ay[k], az[k], tx[k], ty[k], tz[k], ss[t + e]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < BQPT; ++k) {
        if (i0 + k < nt) {
            float* g = out + (b * nt + i0 + k) * 3;
            g[0] = ax[k]; g[1] = ay[k]; g[2] = az[k];
        }
    }
}

hipError_t launch_chamfer_backward(const float* p, const float* q, const int* i1, const int* i2, const float* g1, const float* g2,
                                   float* gp, float* gq, int B, int N, int M, hipStream_t s) {
    constexpr int PER_WG = 256 * BQPT;
    const int big = N > M ? N : M;
    hipLaunchKernelGGL(chamfer_backward_kernel, dim3((big + PER_WG - 1) / PER_WG, B, 2), dim3(256), 0, s, p, q, i1, i2, g1, g2, gp,
                       gq, N, M);
    return hipGetLastError();
}

}  // namespace s3r
