// The optimizer step (s3r_optim_step / s3r_optim_state_init): multi-tensor SGD and Adam / AdamW over a list of fp32 tensors, with an
// optional global gradient norm in s3r_ordered.h's order (a tensor in place of a row) for clipping and for skipping a non-finite step.
// The tensors' pointers and sizes travel BY VALUE in the kernel arguments, at most S3R_OPTIM_TENSORS_PER_LAUNCH per launch: there is no
// pointer table in device memory, so a captured call replays as long as the tensors stay where they were.  lr, the step count and the two
// running powers live in the eight dwords of `state` on the device; nothing here is read on the host.
//
// Everything is fp32 and every operation is rounded on its own (contraction off); division and square root are the correctly rounded
// ones.  The rules, one rounded operation per statement (include/s3r.h states them; tests/_optim64.py restates them):
//   clip:                g = g * clip_coef                                        (only with S3R_OPT_CLIP)
//   SGD   wd != 0:       t = wd * p;  g = g + t
//         mu != 0:       first step: m = g;  later: a = mu * m;  m = a + g
//                        nesterov: t = mu * m;  g = g + t;   otherwise g = m
//                        t = lr * g;  p = p - t
//   Adam  wd != 0:       decoupled: t = lr * wd (once);  s = t * p;  p = p - s;   coupled: t = wd * p;  g = g + t
//                        a = beta1 * m;  b = (1 - beta1) * g;  m = a + b
//                        a = beta2 * v;  q = g * g;  b = (1 - beta2) * q;  v = a + b
//                        mh = m / (1 - beta1_pow);  vh = v / (1 - beta2_pow);  r = sqrtf(vh);  d = r + eps;  u = mh / d
//                        t = lr * u;  p = p - t
// Launches: [optim_sumsq_kernel per 64 tensors] + optim_advance_kernel + optim_update_kernel per 64 tensors.  No LDS, no barrier, no atomics.
#include "s3r_ordered.h"
#include "../../include/s3r.h"

namespace s3r {

constexpr int OPT_TPL = S3R_OPTIM_TENSORS_PER_LAUNCH;
constexpr int OPT_WG = 4 * CHUNK;            // elements per workgroup of the update kernel: four waves, one chunk each

// the kernel arguments of one launch: `count` tensors by value, and the prefix table of their chunks (sumsq) or workgroups (update)
struct OptimSumsqArgs {
    const float* g[OPT_TPL];
    long long n[OPT_TPL];
    unsigned pre[OPT_TPL + 1];               // pre[k]: chunks of this launch's tensors 0 .. k - 1
    unsigned chunk0;                         // chunks of the list's tensors in front of this launch
    unsigned tensor0;                        // tensors of the list in front of this launch
    int count;
};

struct OptimUpdateArgs {
    float* p[OPT_TPL];
    const float* g[OPT_TPL];
    float* m[OPT_TPL];
    float* v[OPT_TPL];
    long long n[OPT_TPL];
    unsigned pre[OPT_TPL + 1];               // pre[k]: workgroups of this launch's tensors 0 .. k - 1
    int count;
};

struct OptimHyper { float beta1, beta2, eps, wd, max_norm; int flags; };

static_assert(sizeof(OptimUpdateArgs) + sizeof(OptimHyper) + sizeof(void*) <= 4096, "the argument block of a launch is 4 KB");

// the tensor of the launch that unit `u` (a chunk or a workgroup) belongs to: the largest k with pre[k] <= u.  u is wave-uniform.
__device__ __forceinline__ int optim_find(const unsigned* pre, int count, unsigned u) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool optim_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for NaN as well

// chunk sums of g * g: one wave per 512-element chunk of one tensor, s3r_ordered.h's lane order and tree.  scratch[chunk0 + c] receives
// chunk c of this launch; the wave of a tensor's chunk 0 also notes where that tensor's chunk sums start (a count, not an address).
__global__ __launch_bounds__(256) void optim_sumsq_kernel(const OptimSumsqArgs a, float* __restrict__ scratch,
                                                          unsigned* __restrict__ starts) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const unsigned c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (c >= a.pre[a.count]) return;                                     // (wave-uniform)
    const int k = optim_find(a.pre, a.count, c);
    const long long n = a.n[k];
    const float* __restrict__ g = a.g[k];
    const unsigned cin = c - a.pre[k];
    const long long e0 = (long long)cin * CHUNK;
    const bool full = e0 + CHUNK <= n;
    v4f gv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) gv[j] = load4(g, e0 + 256 * j + 4 * lane, n, full);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const long long e = e0 + 256 * j + 4 * lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = gv[j][i] * gv[j][i];
            s = s + (e + i < n ? t : 0.f);
        }
    }
    s = wave_tree(s);
    if (lane == 0) {
        scratch[a.chunk0 + c] = s;
        if (cin == 0) starts[a.tensor0 + k] = a.chunk0 + c;
    }
}

// the chunk sums scratch[b .. e) of ONE tensor added in ascending order into a partial that starts as scratch[b], by the whole wave: 64
// of them per load, the next 64 in flight, each lane doing the same serial adds on the values broadcast from their lanes (the value is
// wave-uniform).  The order, and so the bits, are optim_tensor_serial's.
__device__ __forceinline__ float optim_tensor_wave(const float* __restrict__ scratch, unsigned b, unsigned e, int lane) {
#pragma clang fp contract(off)
    float p = 0.f;
    float v = b + lane < e ? scratch[b + lane] : 0.f;
    for (unsigned z0 = b; z0 < e; z0 += 64) {
        const float nv = z0 + 64 + lane < e ? scratch[z0 + 64 + lane] : 0.f;
        const int iv = __float_as_int(v);
        if (e - z0 >= 64) {
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const float t = __int_as_float(__builtin_amdgcn_readlane(iv, l));
                p = (l == 0 && z0 == b) ? t : p + t;
            }
        } else {
            const int cnt = (int)(e - z0);
            for (int l = 0; l < cnt; ++l) {
                const float t = __shfl(v, l, 64);
                p = (l == 0 && z0 == b) ? t : p + t;
            }
        }
        v = nv;
    }
    return p;
}

// ... and by one lane on its own (the lanes of a wave take 64 tensors side by side): sixteen loads in flight, then the adds in order
__device__ __forceinline__ float optim_tensor_serial(const float* __restrict__ scratch, unsigned b, unsigned e) {
#pragma clang fp contract(off)
    float p = scratch[b];
    unsigned z = b + 1;
    for (; z + 16 <= e; z += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = scratch[z + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) p = p + t[u];
    }
    for (; z < e; ++z) p = p + scratch[z];
    return p;
}

constexpr unsigned OPT_WAVE_CHUNKS = 128;    // a tensor with more chunk sums than this is added by the whole wave (a choice of speed: no bit depends on it)

// One wave.  With the norm: the chunk sums of tensor t are added in ascending chunk order into a partial that starts as the tensor's
// chunk 0 (lane L takes tensor t0 + L; a large tensor is taken by the whole wave); the tensor totals are added into ONE accumulator in
// ascending tensor order, starting from tensor 0's.  Then
// norm = sqrtf(total), c = max_norm / (norm + 1e-6f), clip_coef = (c > 1) ? 1 : c (a NaN stays a NaN).  The step is skipped when
// S3R_OPT_SKIP_NONFINITE is set and the norm is not finite: `skipped` grows, nothing else advances.
__global__ __launch_bounds__(64) void optim_advance_kernel(float* state, const float* __restrict__ scratch,
                                                           const unsigned* __restrict__ starts, unsigned chunks, int n_tensors, int kind,
                                                           const OptimHyper h) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    bool skip = false;
    float norm = 0.f, coef = 1.f;
    const bool with_norm = (h.flags & (S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE)) != 0;
    if (with_norm) {
        float acc = 0.f;
        for (int t0 = 0; t0 < n_tensors; t0 += 64) {
            const int t = t0 + lane;
            float p = 0.f;
            unsigned b = 0, e = 0;
            if (t < n_tensors) {
                b = starts[t];
                e = t + 1 < n_tensors ? starts[t + 1] : chunks;
                if (e - b <= OPT_WAVE_CHUNKS) p = optim_tensor_serial(scratch, b, e);
            }
            const int cnt = n_tensors - t0 < 64 ? n_tensors - t0 : 64;
            for (int l = 0; l < cnt; ++l) {
                const unsigned bl = __shfl(b, l, 64), el = __shfl(e, l, 64);
                if (el - bl > OPT_WAVE_CHUNKS) {                             // (wave-uniform)
                    const float pw = optim_tensor_wave(scratch, bl, el, lane);
                    if (lane == l) p = pw;
                }
            }
            for (int l = 0; l < cnt; ++l) {
                const float v = __shfl(p, l, 64);
                acc = (t0 + l == 0) ? v : acc + v;
            }
        }
        norm = sqrtf(acc);
        if (h.flags & S3R_OPT_CLIP) {
            const float d = norm + 1e-6f;
            const float c = h.max_norm / d;
            coef = (c > 1.f) ? 1.f : c;
        }
        skip = (h.flags & S3R_OPT_SKIP_NONFINITE) && !optim_finite(norm);
    }
    if (lane != 0) return;
    int* istate = reinterpret_cast<int*>(state);
    if (with_norm) {
        state[4] = norm;
        state[5] = coef;
    }
    if (skip) {
        istate[6] = istate[6] + 1;
        return;
    }
    istate[0] = istate[0] + 1;
    if (kind == S3R_OPT_ADAM) {
        state[1] = state[1] * h.beta1;
        state[2] = state[2] * h.beta2;
    }
}

// what every element of a step shares: read from `state` once per thread, behind the advance launch
struct OptimStep { float lr, coef, bc1, bc2, omb1, omb2, lrwd; bool first; };

template <int KIND>
__device__ __forceinline__ void optim_elem(float& p, float g, float& m, float& v, const OptimHyper& h, const OptimStep& s) {
#pragma clang fp contract(off)
    if (h.flags & S3R_OPT_CLIP) g = g * s.coef;
    if (KIND == S3R_OPT_SGD) {
        if (h.wd != 0.f) {
            const float t = h.wd * p;
            g = g + t;
        }
        if (h.beta1 != 0.f) {
            if (s.first) {
                m = g;
            } else {
                const float a = h.beta1 * m;
                m = a + g;
            }
            if (h.flags & S3R_OPT_NESTEROV) {
                const float t = h.beta1 * m;
                g = g + t;
            } else {
                g = m;
            }
        }
        const float t = s.lr * g;
        p = p - t;
    } else {
        if (h.wd != 0.f) {
            if (h.flags & S3R_OPT_DECOUPLED_DECAY) {
                const float d = s.lrwd * p;
                p = p - d;
            } else {
                const float t = h.wd * p;
                g = g + t;
            }
        }
        const float a1 = h.beta1 * m;
        const float b1 = s.omb1 * g;
        m = a1 + b1;
        const float a2 = h.beta2 * v;
        const float q = g * g;
        const float b2 = s.omb2 * q;
        v = a2 + b2;
        const float mh = m / s.bc1;
        const float vh = v / s.bc2;
        const float r = sqrtf(vh);
        const float d = r + h.eps;
        const float u = mh / d;
        const float t = s.lr * u;
        p = p - t;
    }
}

// A workgroup of 256 owns 2048 consecutive elements of one tensor: wave w the chunk 512 w .. 512 w + 511 of them, lane L the positions
// 256 j + 4 L + i of that chunk (s3r_ordered.h's ownership: 16-byte accesses where the whole chunk lies inside the tensor).
template <int KIND>
__global__ __launch_bounds__(256) void optim_update_kernel(const OptimUpdateArgs a, const OptimHyper h, const float* __restrict__ state) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = optim_find(a.pre, a.count, blockIdx.x);
    const long long n = a.n[k];
    const long long e0 = (long long)(blockIdx.x - a.pre[k]) * OPT_WG + (long long)wave * CHUNK;
    if (e0 >= n) return;                                                 // (wave-uniform)
    const float norm = state[4];
    if ((h.flags & S3R_OPT_SKIP_NONFINITE) && !optim_finite(norm)) return;          // the advance launch counted it
    OptimStep s;
    s.first = reinterpret_cast<const int*>(state)[0] == 1;
    s.lr = state[3];
    s.coef = state[5];
    s.bc1 = 1.f - state[1];
    s.bc2 = 1.f - state[2];
    s.omb1 = 1.f - h.beta1;
    s.omb2 = 1.f - h.beta2;
    s.lrwd = s.lr * h.wd;
    float* __restrict__ P = a.p[k];
    const float* __restrict__ G = a.g[k];
    const bool has_m = KIND == S3R_OPT_ADAM || h.beta1 != 0.f;
    float* __restrict__ M = a.m[k];
    float* __restrict__ V = a.v[k];
    const bool full = e0 + CHUNK <= n;
    v4f pv[Q], gv[Q], mv[Q], vv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {                                        // every load in flight before the first division
        const long long e = e0 + 256 * j + 4 * lane;
        pv[j] = load4(P, e, n, full);
        gv[j] = load4(G, e, n, full);
        mv[j] = has_m ? load4(M, e, n, full) : v4f{0.f, 0.f, 0.f, 0.f};
        vv[j] = KIND == S3R_OPT_ADAM ? load4(V, e, n, full) : v4f{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const long long e = e0 + 256 * j + 4 * lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float p = pv[j][i], m = mv[j][i], v = vv[j][i];
            optim_elem<KIND>(p, gv[j][i], m, v, h, s);
            pv[j][i] = p; mv[j][i] = m; vv[j][i] = v;
        }
        store4(P, e, n, pv[j], full);
        if (has_m) store4(M, e, n, mv[j], full);
        if (KIND == S3R_OPT_ADAM) store4(V, e, n, vv[j], full);
    }
}

// the eight dwords of a fresh state: step 0, both powers 1, lr, norm 0, coefficient 1, skipped 0, reserved 0
__global__ __launch_bounds__(64) void optim_state_init_kernel(float* __restrict__ state, float lr) {
    const int i = threadIdx.x;
    if (i >= S3R_OPTIM_STATE_DWORDS) return;
    state[i] = i == 1 || i == 2 || i == 5 ? 1.f : (i == 3 ? lr : 0.f);
}

// one fp32 into state[3] (the learning rate of the next step), as a kernel so that it orders on the stream like the step
__global__ __launch_bounds__(64) void optim_set_lr_kernel(float* __restrict__ state, float lr) {
    if (threadIdx.x == 0) state[3] = lr;
}

hipError_t launch_optim_state_init(float* state, float lr, hipStream_t s) {
    hipLaunchKernelGGL(optim_state_init_kernel, dim3(1), dim3(64), 0, s, state, lr);
    return hipGetLastError();
}

hipError_t launch_optim_set_lr(float* state, float lr, hipStream_t s) {
    hipLaunchKernelGGL(optim_set_lr_kernel, dim3(1), dim3(64), 0, s, state, lr);
    return hipGetLastError();
}

long long optim_chunks(const s3r_optim_tensor* t, int n) {
    long long c = 0;
    for (int i = 0; i < n; ++i) c += chunks(t[i].elems);
    return c;
}

hipError_t launch_optim_step(int kind, int flags, float beta1, float beta2, float eps, float wd, float max_norm, const s3r_optim_tensor* t,
                             int n_tensors, float* state, float* scratch, hipStream_t s) {
    const OptimHyper h{beta1, beta2, eps, wd, max_norm, flags};
    const bool with_norm = (flags & (S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE)) != 0;
    const long long total_chunks = with_norm ? optim_chunks(t, n_tensors) : 0;
    unsigned* starts = with_norm ? reinterpret_cast<unsigned*>(scratch + total_chunks) : nullptr;
    if (with_norm) {
        long long c0 = 0;
        for (int t0 = 0; t0 < n_tensors; t0 += OPT_TPL) {
            OptimSumsqArgs a;
            a.count = n_tensors - t0 < OPT_TPL ? n_tensors - t0 : OPT_TPL;
            a.chunk0 = (unsigned)c0;
            a.tensor0 = (unsigned)t0;
            unsigned pre = 0;
            for (int k = 0; k < OPT_TPL; ++k) {
                const bool live = k < a.count;
                a.g[k] = live ? t[t0 + k].grad : nullptr;
                a.n[k] = live ? t[t0 + k].elems : 0;
                a.pre[k] = pre;
                if (live) pre += (unsigned)chunks(t[t0 + k].elems);
            }
            a.pre[OPT_TPL] = pre;
            hipLaunchKernelGGL(optim_sumsq_kernel, dim3((pre + 3) / 4), dim3(256), 0, s, a, scratch, starts);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            c0 += pre;
        }
    }
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(64), 0, s, state, (const float*)scratch, (const unsigned*)starts,
                       (unsigned)total_chunks, n_tensors, kind, h);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int t0 = 0; t0 < n_tensors; t0 += OPT_TPL) {
        OptimUpdateArgs a;
        a.count = n_tensors - t0 < OPT_TPL ? n_tensors - t0 : OPT_TPL;
        unsigned pre = 0;
        for (int k = 0; k < OPT_TPL; ++k) {
            const bool live = k < a.count;
            a.p[k] = live ? t[t0 + k].param : nullptr;
            a.g[k] = live ? t[t0 + k].grad : nullptr;
            a.m[k] = live ? t[t0 + k].m : nullptr;
            a.v[k] = live ? t[t0 + k].v : nullptr;
            a.n[k] = live ? t[t0 + k].elems : 0;
            a.pre[k] = pre;
            if (live) pre += (unsigned)((t[t0 + k].elems + OPT_WG - 1) / OPT_WG);
        }
        a.pre[OPT_TPL] = pre;
        if (kind == S3R_OPT_ADAM)
            hipLaunchKernelGGL(optim_update_kernel<S3R_OPT_ADAM>, dim3(pre), dim3(256), 0, s, a, h, (const float*)state);
        else
            hipLaunchKernelGGL(optim_update_kernel<S3R_OPT_SGD>, dim3(pre), dim3(256), 0, s, a, h, (const float*)state);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace s3r
