// Ground-truth point clouds drawn on the exposed faces of occupancy grids (s3r_voxel_surface_points): the Stereo2Point target made
// from what a StereoShapeNet tree holds.  include/s3r.h states the rule; tests/_surface64.py restates it.
//
// A sample's V = D H W voxels are cut into chunks of 64 consecutive linear indices v = (i0 H + i1) W + i2.  Face f = 2 axis + side of
// voxel v has number e = 6 v + f; the exposed ones are counted in ascending e.  Three launches, every node a kernel, no atomics:
//   surface_mask_kernel   one lane per voxel: the 6-bit exposure mask (bit f) as one byte, and per wave the chunk's face count
//   surface_scan_kernel   one workgroup per sample: the chunk counts become their exclusive prefix (in place); N goes to n_faces[b]
//   surface_draw_kernel   one lane per point: Philox, k = w0 N >> 32, the chunk by bisection of the prefix (staged in LDS up to
//                         LDS_CHUNKS chunks, read from global memory above), a walk over the chunk's 64 mask bytes to the face, the
//                         three coordinates.  Every search result is clamped to its range, so no scratch content can index past a buffer.
// Integers everywhere but the three rounded operations per coordinate (contraction off): any launch shape gives the same bits.
// scratch (as dwords): [B nch] counts -> prefix, [B] N, [B nch 16] mask bytes (64 per chunk, zero behind voxel V - 1).
#include "s3r_kernels.h"
#include "s3r_philox.h"
#include "../../include/s3r.h"

namespace s3r {

constexpr int SURFACE_PURPOSE = 0x100;       // the counter's third word (the augmentation owns purposes 0 .. 6)
constexpr int LDS_CHUNKS = 4096;             // prefix entries a draw workgroup stages (16 KiB): a 64^3 grid; 32^3 has 512

struct SurfaceArgs {
    const float* occ;
    const long long* ids;
    float* points;
    int* n_faces;                            // may be NULL
    int* prefix;                             // [B][nch]
    int* total;                              // [B]
    unsigned char* mask;                     // [B][nch * 64]
    float threshold;
    unsigned key0, key1;
    int D, H, W, V, nch, n_points;
    float inv[3];                            // 1.f / (float)size, correctly rounded on the host
};

__global__ __launch_bounds__(256) void surface_mask_kernel(const SurfaceArgs a, unsigned blocks_per_sample) {
    const int lane = threadIdx.x & 63;
    const unsigned b = blockIdx.x / blocks_per_sample;
    const int chunk = (int)(blockIdx.x - b * blocks_per_sample) * 4 + (int)(threadIdx.x >> 6);
    if (chunk >= a.nch) return;                                          // (wave-uniform)
    const int v = chunk * 64 + lane;
    unsigned m = 0;
    if (v < a.V) {
        const float* __restrict__ g = a.occ + (size_t)b * a.V;
        if (g[v] > a.threshold) {
            const int i2 = v % a.W, t = v / a.W;
            const int i1 = t % a.H, i0 = t / a.H;
            const int HW = a.H * a.W;
            // exposed: the neighbour is outside the grid or not occupied (a NaN compares false: empty)
            if (i0 == 0 || !(g[v - HW] > a.threshold)) m |= 1u;
            if (i0 == a.D - 1 || !(g[v + HW] > a.threshold)) m |= 2u;
            if (i1 == 0 || !(g[v - a.W] > a.threshold)) m |= 4u;
            if (i1 == a.H - 1 || !(g[v + a.W] > a.threshold)) m |= 8u;
            if (i2 == 0 || !(g[v - 1] > a.threshold)) m |= 16u;
            if (i2 == a.W - 1 || !(g[v + 1] > a.threshold)) m |= 32u;
        }
    }
    a.mask[((size_t)b * a.nch + chunk) * 64 + lane] = (unsigned char)m;
    int c = __popc(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0) a.prefix[(size_t)b * a.nch + chunk] = c;
}

// thread t owns the entries [t per, (t + 1) per): its sum, an exclusive scan of the 256 sums, then its entries' exclusive prefix
__global__ __launch_bounds__(256) void surface_scan_kernel(const SurfaceArgs a) {
    __shared__ int wave_sum[4];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int* __restrict__ p = a.prefix + (size_t)b * a.nch;
    const int per = (a.nch + 255) / 256;
    const int beg = min(t * per, a.nch), end = min(beg + per, a.nch);
    int s = 0;
    for (int i = beg; i < end; ++i) s += p[i];
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wave_sum[wv] = incl;
    __syncthreads();
    int base = incl - s;
    for (int w = 0; w < wv; ++w) base += wave_sum[w];
    for (int i = beg; i < end; ++i) {
        const int c = p[i];
        p[i] = base;
        base += c;
    }
    if (t == 255) {                                                      // (its `base` is now the sample's face count)
        a.total[b] = base;
        if (a.n_faces) a.n_faces[b] = base;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void surface_draw_kernel(const SurfaceArgs a, unsigned blocks_per_sample) {
#pragma clang fp contract(off)
    __shared__ int staged[STAGED ? LDS_CHUNKS : 1];
    const unsigned b = blockIdx.x / blocks_per_sample;
    const int j = (int)(blockIdx.x - b * blocks_per_sample) * 256 + (int)threadIdx.x;
    const int* __restrict__ gpre = a.prefix + (size_t)b * a.nch;
    if (STAGED) {
        for (int i = threadIdx.x; i < a.nch; i += 256) staged[i] = gpre[i];
        __syncthreads();
    }
    if (j >= a.n_points) return;
    float p[3] = {0.f, 0.f, 0.f};
    const int N = a.total[b];
    if (N > 0) {
        const unsigned long long id = (unsigned long long)a.ids[b];
        const Words w = philox((unsigned)id, (unsigned)(id >> 32), (unsigned)SURFACE_PURPOSE, (unsigned)j, a.key0, a.key1);
        const int k = (int)(((unsigned long long)w.w[0] * (unsigned long long)(unsigned)N) >> 32);
        // the last chunk whose prefix is <= k: lo stays in [0, nch)
        int lo = 0, hi = a.nch;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((STAGED ? staged[mid] : gpre[mid]) <= k) lo = mid; else hi = mid;
        }
        int r = k - (STAGED ? staged[lo] : gpre[lo]);
        // walk the chunk's 64 mask bytes, four at a time, to the voxel that holds the chunk's face r, then to the face
        const unsigned* __restrict__ mw = reinterpret_cast<const unsigned*>(a.mask + ((size_t)b * a.nch + lo) * 64);
        int q = 15;
        unsigned word = 0;
        for (int i = 0; i < 16; ++i) {
            word = mw[i] & 0x3F3F3F3Fu;
            const int c = __popc(word);
            if (r < c) { q = i; break; }
            if (i < 15) r -= c;
        }
        int byte = 3;
        for (int i = 0; i < 4; ++i) {
            const int c = __popc((word >> (8 * i)) & 0x3Fu);
            if (r < c) { byte = i; break; }
            if (i < 3) r -= c;
        }
        const unsigned m = (word >> (8 * byte)) & 0x3Fu;
        int f = 5;
        for (int i = 0; i < 6; ++i) {
            if ((m >> i) & 1u) {
                if (r == 0) { f = i; break; }
                --r;
            }
        }
        const int v = min(lo * 64 + q * 4 + byte, a.V - 1);
        const int i2 = v % a.W, t = v / a.W;
        const int idx[3] = {t / a.H, t % a.H, i2};
        const int axis = f >> 1, side = f & 1;
        const float u[2] = {aug_unit(w.w[1]), aug_unit(w.w[2])};
        int n = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float x;
            if (c == axis) {
                x = (float)(idx[c] + side);
            } else {
                x = (float)idx[c] + u[n];
                ++n;
            }
            x = x * a.inv[c];
            p[c] = x - 0.5f;
        }
    }
    float* __restrict__ o = a.points + ((size_t)b * a.n_points + j) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

long long surface_points_scratch(int B, long long V) { return (long long)B * (17 * ((V + 63) / 64) + 1); }

hipError_t launch_surface_points(const float* occ, float threshold, const int64_t* ids, uint64_t seed, float* points, int32_t* n_faces,
                                 int B, int D, int H, int W, int n_points, float* scratch, hipStream_t s) {
    SurfaceArgs a;
    a.occ = occ; a.ids = reinterpret_cast<const long long*>(ids); a.points = points; a.n_faces = n_faces;
    a.threshold = threshold;
    a.key0 = (unsigned)seed; a.key1 = (unsigned)(seed >> 32);
    a.D = D; a.H = H; a.W = W; a.V = D * H * W; a.nch = (a.V + 63) / 64; a.n_points = n_points;
    a.inv[0] = 1.f / (float)D; a.inv[1] = 1.f / (float)H; a.inv[2] = 1.f / (float)W;
    a.prefix = reinterpret_cast<int*>(scratch);
    a.total = a.prefix + (size_t)B * a.nch;
    a.mask = reinterpret_cast<unsigned char*>(a.total + B);
    const unsigned mask_blocks = (unsigned)((a.nch + 3) / 4), draw_blocks = (unsigned)((n_points + 255) / 256);
    hipLaunchKernelGGL(surface_mask_kernel, dim3((unsigned)B * mask_blocks), dim3(256), 0, s, a, mask_blocks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(surface_scan_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.nch <= LDS_CHUNKS)
        hipLaunchKernelGGL(surface_draw_kernel<true>, dim3((unsigned)B * draw_blocks), dim3(256), 0, s, a, draw_blocks);
    else
        hipLaunchKernelGGL(surface_draw_kernel<false>, dim3((unsigned)B * draw_blocks), dim3(256), 0, s, a, draw_blocks);
    return hipGetLastError();
}

}  // namespace s3r
