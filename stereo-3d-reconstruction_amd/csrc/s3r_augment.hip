// The training-time augmentation of a stereo batch (s3r_augment_pair): 8-bit renders (RGB, or RGBA composited here over a drawn
// background) -> fp32 network inputs in [0, 1], with an integer shift shared by the two views and the disparity maps, a channel
// permutation, brightness / contrast / saturation jitter and per-view noise.  Every random number is Philox4x32-10 of (seed, sample id,
// purpose, index): a sample's bits depend on its id and its pixels only, and a captured call draws afresh from the ids in device memory.
//
// Everything is fp32 and every operation is rounded on its own (contraction off); the division is the correctly rounded one.  The
// order, one rounded operation per statement (include/s3r.h states it; tests/_augment64.py restates it):
//   source:      inside the image the render's code (RGBA: (c * a + bg * (255 - a) + 127) / 255 in integers), outside it bg[c]
//   scale:       v = (float)code / 255.f
//   brightness:  v = br * v;  clamp
//   contrast:    a = ct * v;  t = 1.f - ct;  b = t * m;  v = a + b;  clamp            (m: the pair's mean luma after brightness)
//   saturation:  a = st * v;  t = 1.f - st;  b = t * l;  v = a + b;  clamp            (l: the pixel's own luma after contrast)
//   noise:       s = u0 + u1;  s = s + u2;  s = s + u3;  s = s - 2.f;  s = s * 1.7320508f;  s = sigma * s;  v = v + s;  clamp
// The mean luma is summed in s3r_ordered.h's order with the two views as the B = 2 rows of one pair.
// Launches: [augment_luma_kernel + augment_mean_kernel, only with contrast] + augment_apply_kernel.  No LDS, no barrier, no atomics.
#include "s3r_ordered.h"
#include "s3r_philox.h"
#include "../../include/s3r.h"

namespace s3r {

struct AugArgs {
    const uint8_t* src[2];                   // left, right
    const float* disp[2];                    // NULL: no disparity maps
    float* out[2];
    float* odisp[2];
    const long long* ids;
    unsigned key0, key1;
    int channels, max_shift, flags, bg_lo, bg_hi;
    float br_lo, br_hi, ct_lo, ct_hi, st_lo, st_hi, sigma;
    int B, H, W;
    long long S;                             // H W
    long long nch;                           // chunks(S)
};

__device__ __forceinline__ float aug_range(float u, float lo, float hi) {
#pragma clang fp contract(off)
    float t = hi - lo;
    t = u * t;
    return lo + t;
}

__device__ __forceinline__ float aug_clamp(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float aug_luma(float v0, float v1, float v2) {
#pragma clang fp contract(off)
    const float a = 0.299f * v0;
    const float b = 0.587f * v1;
    const float c = 0.114f * v2;
    const float s = a + b;
    return s + c;
}

// what a pair's pixels share: the three draws of purpose 0 (made whether or not their op is on)
struct AugSample { int dy, dx, perm; float br, ct, st; unsigned bg[3]; unsigned id0, id1; };

__device__ __forceinline__ AugSample aug_sample(const AugArgs& a, int b) {
    AugSample s;
    const unsigned long long id = (unsigned long long)a.ids[b];
    s.id0 = (unsigned)id; s.id1 = (unsigned)(id >> 32);
    const Words g = philox(s.id0, s.id1, 0u, 0u, a.key0, a.key1);
    const unsigned span = 2u * (unsigned)a.max_shift + 1u;
    s.dy = (int)(g.w[0] % span) - a.max_shift;
    s.dx = (int)(g.w[1] % span) - a.max_shift;
    s.perm = (int)(g.w[2] % 6u);
    const Words j = philox(s.id0, s.id1, 0u, 1u, a.key0, a.key1);
    s.br = aug_range(aug_unit(j.w[0]), a.br_lo, a.br_hi);
    s.ct = aug_range(aug_unit(j.w[1]), a.ct_lo, a.ct_hi);
    s.st = aug_range(aug_unit(j.w[2]), a.st_lo, a.st_hi);
    const Words k = philox(s.id0, s.id1, 0u, 2u, a.key0, a.key1);
    const unsigned bspan = (unsigned)(a.bg_hi - a.bg_lo) + 1u;
#pragma unroll
    for (int c = 0; c < 3; ++c) s.bg[c] = (unsigned)a.bg_lo + k.w[c] % bspan;
    return s;
}

__device__ __forceinline__ bool aug_on(float lo, float hi) { return !(lo == 1.f && hi == 1.f); }

// (row, column) of position p — H W < 2^31, so ONE 32-bit division per run of consecutive positions — and the step to the next one
struct AugPos { int y, x; };
__device__ __forceinline__ AugPos aug_pos(unsigned p, int W) {
    const unsigned y = p / (unsigned)W;
    return AugPos{(int)y, (int)(p - y * (unsigned)W)};
}
__device__ __forceinline__ void aug_next(AugPos& q, int W) {
    if (++q.x == W) { q.x = 0; ++q.y; }
}

// steps 1 - 3 of output pixel (y, x) of one view of sample b: the three channels after brightness.  `inside` and `sp` (the source
// position) come back for the disparity copy
__device__ __forceinline__ void aug_pixel(const AugArgs& a, const AugSample& s, const uint8_t* __restrict__ img, int y, int x, float (&v)[3],
                                          bool& inside, long long& sp) {
#pragma clang fp contract(off)
    const int sy = y - s.dy, sx = x - s.dx;
    inside = sy >= 0 && sy < a.H && sx >= 0 && sx < a.W;
    sp = inside ? (long long)sy * a.W + sx : 0;
    unsigned code[3] = {s.bg[0], s.bg[1], s.bg[2]};
    if (inside) {
        if (a.channels == 4) {
            const unsigned al = img[3 * a.S + sp];
#pragma unroll
            for (int c = 0; c < 3; ++c) code[c] = ((unsigned)img[c * a.S + sp] * al + s.bg[c] * (255u - al) + 127u) / 255u;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) code[c] = img[c * a.S + sp];
        }
    }
    const bool bright = aug_on(a.br_lo, a.br_hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = (float)code[c] / 255.f;
        if (bright) {
            t = s.br * t;
            t = aug_clamp(t);
        }
        v[c] = t;
    }
}

// chunk sums of the luma after brightness: one wave per 512-position chunk of one view of one sample, s3r_ordered.h's lane order and
// tree.  part[(2 b + side) nch + chunk]
__global__ __launch_bounds__(256) void augment_luma_kernel(const AugArgs a, float* __restrict__ part) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const unsigned wv = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const unsigned nch = (unsigned)a.nch;
    if (wv >= 2u * (unsigned)a.B * nch) return;                          // (wave-uniform)
    const unsigned row = wv / nch, chunk = wv - row * nch;
    const int b = (int)(row >> 1), side = (int)(row & 1);
    const AugSample s = aug_sample(a, b);
    const uint8_t* __restrict__ img = a.src[side] + (size_t)b * a.channels * a.S;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const unsigned p0 = chunk * (unsigned)CHUNK + 256u * j + 4u * lane;      // (< S + 512 < 2^32)
        AugPos q = aug_pos(p0, a.W);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float l = 0.f;
            if ((long long)p0 + i < a.S) {
                float v[3]; bool in; long long sp;
                aug_pixel(a, s, img, q.y, q.x, v, in, sp);
                l = aug_luma(v[0], v[1], v[2]);
            }
            acc = acc + l;
            aug_next(q, a.W);
        }
    }
    acc = wave_tree(acc);
    if (lane == 0) part[wv] = acc;
}

// one wave per pair: the two views' chunk sums as the B = 2 rows of s3r_ordered.h's row_total, then m = total / (float)(2 S)
__global__ __launch_bounds__(64) void augment_mean_kernel(const float* __restrict__ part, float* __restrict__ mean, long long nch, long long S) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    const float total = row_total(part + (size_t)b * 2 * nch, 2, nch, threadIdx.x);
    if (threadIdx.x == 0) mean[b] = total / (float)(2 * S);
}

__device__ __forceinline__ float aug_pick(const float (&v)[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// A lane owns four consecutive positions of one view of one sample, all three channels: 16-byte stores through store4.  A workgroup of
// 256 takes 1024 positions; blockIdx.x = (2 b + side) nblk + block
__global__ __launch_bounds__(256) void augment_apply_kernel(const AugArgs a, const float* __restrict__ mean, unsigned nblk) {
#pragma clang fp contract(off)
    const unsigned row = blockIdx.x / nblk, blk = blockIdx.x - row * nblk;
    const int b = (int)(row >> 1), side = (int)(row & 1);
    const long long p0 = (long long)blk * 1024 + 4 * (long long)threadIdx.x;
    if (p0 >= a.S) return;
    const AugSample s = aug_sample(a, b);
    const uint8_t* __restrict__ img = a.src[side] + (size_t)b * a.channels * a.S;
    const bool contrast = aug_on(a.ct_lo, a.ct_hi), saturation = aug_on(a.st_lo, a.st_hi), noise = a.sigma != 0.f;
    const float m = contrast ? mean[b] : 0.f;
    const bool full = p0 + 4 <= a.S;
    const bool with_disp = a.disp[side] != nullptr;
    const float* __restrict__ dsrc = with_disp ? a.disp[side] + (size_t)b * a.S : nullptr;
    v4f o[3], od;
    AugPos q = aug_pos((unsigned)p0, a.W);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long p = p0 + i;
        float v[3] = {0.f, 0.f, 0.f};
        float dv = 0.f;
        if (p < a.S) {
            bool in; long long sp;
            aug_pixel(a, s, img, q.y, q.x, v, in, sp);
            aug_next(q, a.W);
            if (with_disp) dv = in ? dsrc[sp] : __builtin_inff();
            if (contrast) {
                const float t = 1.f - s.ct;
                const float bm = t * m;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float av = s.ct * v[c];
                    v[c] = aug_clamp(av + bm);
                }
            }
            if (saturation) {
                const float l = aug_luma(v[0], v[1], v[2]);
                const float t = 1.f - s.st;
                const float bl = t * l;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float av = s.st * v[c];
                    v[c] = aug_clamp(av + bl);
                }
            }
            if (noise) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const Words n = philox(s.id0, s.id1, (unsigned)(1 + 3 * side + c), (unsigned)p, a.key0, a.key1);
                    float z = aug_unit(n.w[0]) + aug_unit(n.w[1]);
                    z = z + aug_unit(n.w[2]);
                    z = z + aug_unit(n.w[3]);
                    z = z - 2.f;
                    z = z * 1.7320508f;
                    z = a.sigma * z;
                    v[c] = aug_clamp(v[c] + z);
                }
            }
        }
        od[i] = dv;
        if (a.flags & S3R_AUG_PERMUTE_RGB) {
            // the lexicographic permutations of (0, 1, 2): 012 021 102 120 201 210
            const int k0 = s.perm >> 1;
            const int lo = k0 == 0 ? 1 : 0, hi = k0 == 2 ? 1 : 2;      // the two channels left, ascending
            const int k1 = (s.perm & 1) ? hi : lo, k2 = (s.perm & 1) ? lo : hi;
            o[0][i] = aug_pick(v, k0); o[1][i] = aug_pick(v, k1); o[2][i] = aug_pick(v, k2);
        } else {
            o[0][i] = v[0]; o[1][i] = v[1]; o[2][i] = v[2];
        }
    }
    float* __restrict__ out = a.out[side] + (size_t)b * 3 * a.S;
#pragma unroll
    for (int c = 0; c < 3; ++c) store4(out + c * a.S, p0, a.S, o[c], full);
    if (with_disp) store4(a.odisp[side] + (size_t)b * a.S, p0, a.S, od, full);
}

static bool augment_contrast(const s3r_augment_desc* d) { return !(d->contrast_lo == 1.f && d->contrast_hi == 1.f); }

// the chunk sums of both views of every pair, then one mean per pair
long long augment_scratch(const s3r_augment_desc* d, int B, long long S) { return augment_contrast(d) ? 2ll * B * chunks(S) + B : 0; }

hipError_t launch_augment_pair(const s3r_augment_desc* d, const uint8_t* left, const uint8_t* right, const int64_t* ids, const float* disp_l,
                               const float* disp_r, float* out_l, float* out_r, float* out_dl, float* out_dr, int B, int H, int W,
                               float* scratch, hipStream_t s) {
    AugArgs a;
    a.src[0] = left; a.src[1] = right;
    a.disp[0] = disp_l; a.disp[1] = disp_r;
    a.out[0] = out_l; a.out[1] = out_r;
    a.odisp[0] = out_dl; a.odisp[1] = out_dr;
    a.ids = reinterpret_cast<const long long*>(ids);
    a.key0 = (unsigned)d->seed; a.key1 = (unsigned)(d->seed >> 32);
    a.channels = d->channels; a.max_shift = d->max_shift; a.flags = d->flags; a.bg_lo = d->bg_lo; a.bg_hi = d->bg_hi;
    a.br_lo = d->brightness_lo; a.br_hi = d->brightness_hi; a.ct_lo = d->contrast_lo; a.ct_hi = d->contrast_hi;
    a.st_lo = d->saturation_lo; a.st_hi = d->saturation_hi; a.sigma = d->noise_sigma;
    a.B = B; a.H = H; a.W = W;
    a.S = (long long)H * W;
    a.nch = chunks(a.S);
    float* mean = nullptr;
    if (augment_contrast(d)) {
        const long long waves = 2ll * B * a.nch;
        mean = scratch + waves;
        hipLaunchKernelGGL(augment_luma_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a, scratch);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(augment_mean_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float*)scratch, mean, a.nch, a.S);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const unsigned nblk = (unsigned)((a.S + 1023) / 1024);
    hipLaunchKernelGGL(augment_apply_kernel, dim3(2u * (unsigned)B * nblk), dim3(256), 0, s, a, (const float*)mean, nblk);
    return hipGetLastError();
}

}  // namespace s3r
