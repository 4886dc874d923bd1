// Host-side internals shared by the host translation units of libs3r_hip.so — s3r_prof.hip (event profiler), s3r_plan.hip (layer
// geometry, kernel policy, sizes, the packed weight image's layout, chain / arena planner), s3r_conv_forward.hip (one runner per
// kernel path, the dispatcher over them and their entry points) and s3r_api_layers.hip / s3r_api_tasks.hip (the other C-ABI entry
// points, by family); last, the argument checks those entry points share.  Not part of the ABI (include/s3r.h) and not seen by the
// kernel sources (those share s3r_kernels.h).
#pragma once
#include "../../include/s3r.h"
#include "s3r_kernels.h"

#include <cstdint>
#include <initializer_list>
#include <vector>

namespace s3rh {

constexpr int64_t kMaxElems = (int64_t)1 << 31;
constexpr int64_t kMaxBytes = (int64_t)1 << 32;
// padded output edges the two-axis Winograd finish kernels can stage in 64 KiB of LDS (include/s3r.h, s3r_algo): one fp32 plane of
// 128^2 (Conv2d), four slices of 64^2 (the semi-fused Conv3d form, which the plan offers up to an edge of 60)
constexpr int kWino2PlaneEdge = 128, kWino2SemiEdge = 64, kWino2SemiMaxEdge = 60;

// ---------------------------------------------------------------- errors (s3r_plan.hip): thread-local message behind s3r_last_error
const char* last_error();

// ---------------------------------------------------------------- profiler (s3r_prof.hip)
enum Family { F_MFMA = 0, F_STEM = 1, F_HEAD = 2, F_COSTVOL = 3, F_LINEAR = 4, F_CHAMFER = 5, F_IOU = 6, F_PACK = 7, F_PAD = 8, F_DISP = 9,
              F_AUX = 10 };    // F_AUX: a transform / difference / finish pass of a Winograd layer, nested inside its F_MFMA record

// One record: two events around everything enqueued while the scope lives.  A scope takes COPIES of its two event handles under
// the profiler's lock, so nothing of the pool is touched outside it; its stop record happens under the lock as well and is
// skipped when the pool was rebuilt meanwhile (s3r_profile_enable from another thread: the handles would be destroyed events).
// Events live on the device that was current at s3r_profile_enable: launches on another device are not profiled.
struct ProfScope {
    bool active = false;
    int slot = -1;
    unsigned gen = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int launches = 1;     // kernel launches inside the scope (a conv may be cut into bulk + remainder, + split-K finish)
    int algo = 0;         // what ran: 0 direct, 1 / 2 / 3 the Winograd serial / class-parallel / dual form, 4 the two-axis algorithm
    int form = 0;         // s3r_prof_record.launch_form: OR of ConvLaunchInfo::form over the scope's direct launches
    double exec = -1.0;   // MFMA FLOPs executed (< 0: the algorithmic count)
    int family, prev_tag = 0;
    hipStream_t stream;
    ProfScope(hipStream_t s, int family, int tag, double flops, double bytes);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};

// ---------------------------------------------------------------- geometry, policy, sizes, planner (s3r_plan.hip)
struct Geo {
    int nd;            // spatial dims
    int in, out;       // logical edge sizes
    int in_p, out_p;   // edge sizes of the halo-padded buffers
    int64_t in_sp, out_sp;         // logical voxels per channel
    int64_t x_elems, y_elems;      // elements of the (padded) buffers
    int64_t x_store, y_store;      // their storage in 4-byte units (bf16 buffers take half)
    int64_t w_elems;
    double flops, bytes;           // algorithmic (unpadded) work of the layer
};

enum Route { R_STEM, R_HEAD, R_MFMA, R_LINEAR };

enum { ALG_DIRECT = 0, ALG_WINO = 1, ALG_WINO2 = 2, ALG_WINO3 = 3 };      // (WINO3: the three-axis form of the transposed layers)

struct Wino2Geo { int ax, m, n, ncls, out, sg, wp, kw, bmax; int64_t w_elems, v_sample, pos_sample; };

struct WinoNeed { int64_t v, slab, total; };

struct LaunchH { int tm, ksplit; };

struct Launch { int cfg, vec, ksplit; };

struct Plan {
    std::vector<s3r_conv_desc> d;     // descriptors with planned halos
    std::vector<Route> r;
    std::vector<Geo> g;
    std::vector<int64_t> off;         // workspace offset of layer i's OUTPUT (-1: the caller's y)
    std::vector<char> fuse_head;      // layer i is an MFMA conv whose epilogue also runs layer i+1 (1x1 head)
    std::vector<int64_t> region;      // storage of layer i's output region where it is more than g[i].y_store (a 3D hand-off pair: the
                                      // larger of the plain output and the consumer's operand, whichever the launch forms pick), else 0
    bool stem_wino = false;           // the stem writes layer 1's Winograd-transformed planes (launch_stem_wino), not its activation
    bool pad_input = false;
    int64_t pad_off = 0;
    int64_t scratch_off = 0, scratch_elems = 0;   // split-K slabs, shared by all layers of the chain
    int64_t total = 0;
};

int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
int64_t ipow(int64_t b, int e);
int wino_r(const s3r_conv_desc*);
int out_size(const s3r_conv_desc* d);
int dil_of(const s3r_conv_desc* d);
bool staged_layer(const s3r_conv_desc* d);
struct StagedGeo { int cin_pad, step, pe, sp; int64_t elems; int bmax; };      // bmax > 0 (im2col): samples staged per pass
StagedGeo staged_geo(const s3r_conv_desc* d);
s3r::ConvParams make_params_staged(const s3r_conv_desc* d, const Geo& g);
// residue classes of a general ConvTranspose with dilation 1 (s3r_general.hip): class r of an axis = the outputs o with
// (o + pad) % stride == r; kr taps (0: none of that residue), ke >= 1 taps packed, positions q = qmin .. qmin + nq - 1 (nq <= 0: no output)
struct TClassAxis { int kr, ke, qmin, nq; };
bool im2col_layer(const s3r_conv_desc* d);      // a staged convolution with cin <= 8: unfolded to a 1 x 1 GEMM over cin k^nd rows
bool leaky_fused(const s3r_conv_desc* d);
bool needs_act_pass(const s3r_conv_desc* d);
bool tclass_layer(const s3r_conv_desc* d);
bool tclass_direct(const s3r_conv_desc* d);
// ... and a residue-class layer with k == stride, pad 0, out_pad 0 (every class is ONE tap on the same input element): one GEMM over
// cout x taps rows with a depth-to-space store instead of stride^ndim launches
bool tshuf_layer(const s3r_conv_desc* d);
s3r::ConvParams make_params_tshuf(const s3r_conv_desc* d, const Geo& g);
int want_halo(const s3r_conv_desc* d, Route r);
TClassAxis tclass_axis(const s3r_conv_desc* d, int r);
int tclass_halo(const s3r_conv_desc* d);
int64_t tclass_w_elems(const s3r_conv_desc* d);                      // the s^nd class slabs, in class order
// class (rd, rh, rw) as the direct kernel sees it: a stride-1 convolution over the staged tensor; false: the class has no output.
// *w_off = floats from the start of the packed image to the class's slab; *macs = its multiply-adds (CinPad channels)
bool make_params_tclass(const s3r_conv_desc* d, const Geo& g, int rd, int rh, int rw, s3r::ConvParams* q, int64_t* w_off, double* macs);
int geometry(const s3r_conv_desc* d, Geo* g);
int route(const s3r_conv_desc* d, Route* r);
int need_halo(const s3r_conv_desc* d, Route r);
int check_halos(const s3r_conv_desc* d, Route r);
int cout_pad(int cout);
int wino_mode();
bool wino_layer(const s3r_conv_desc* d);
bool dwino_layer(const s3r_conv_desc* d);
bool dwino3_layer(const s3r_conv_desc* d);
bool dwino3_desc_ok(const s3r_conv_desc* d);
// The packed image of an fp32 MFMA layer that is not staged, the ONE description packing, sizing and the runners share: convolution
// [direct | one-axis | two-axis], transposed [direct (8 classes x 8 taps) | two-axis classes | three-axis].  Floats; -1: no such slab
struct PackedLayout { int64_t direct, wino, dwino, wino2, dwino3, total; };
PackedLayout packed_layout(const s3r_conv_desc* d, const Geo& g);
// the divisors of the conv kernels' position decode, from the positions per sample (Nd, Nh, Nw)
inline void set_divs(s3r::ConvParams& p) {
    p.dS = s3r::FastDiv((unsigned)(p.Nd * p.Nh * p.Nw));
    p.dHW = s3r::FastDiv((unsigned)(p.Nh * p.Nw));
    p.dW = s3r::FastDiv((unsigned)p.Nw);
}
struct Dwino3Need { int64_t diff, total; bool split; };
Dwino3Need dwino3_need(const s3r_conv_desc* d, int form);
bool wino_desc_ok(const s3r_conv_desc* d);
int wino2_ax(const s3r_conv_desc* d);
bool wino2_desc_ok(const s3r_conv_desc* d);
bool wino2_plane_fits(const s3r_conv_desc* d);
bool wino2_semi_fits(const s3r_conv_desc* d);
int wino2_max_edge();
int resolve_algo(const s3r_conv_desc* d, int* alg, int* form);
bool resolves_to_wino(const s3r_conv_desc* d);
Wino2Geo wino2_geo(const s3r_conv_desc* d);
int64_t wino_w_elems(const s3r_conv_desc* d);
int64_t wino_v_elems(const s3r_conv_desc* d);
int wino_bmax(const s3r_conv_desc* d);
int64_t dwino_w_elems(const s3r_conv_desc* d);
bool dwino_materialise(const s3r_conv_desc* d);
int64_t dwino_d_elems(const s3r_conv_desc* d);
int wino_kind(const s3r_conv_desc* d);
int wino_kcls(const s3r_conv_desc* d);
int64_t wino_positions(const s3r_conv_desc* d, int nb);
WinoNeed wino_need(const s3r_conv_desc* d, int form, bool head);
double wino_exec_flops(const s3r_conv_desc* d, const Geo& g);
int wino2_form_of(const s3r_conv_desc* d, int ntotal, int forced);
WinoNeed wino2_need(const s3r_conv_desc* d, int form);
double wino2_exec_flops(const s3r_conv_desc* d);
int cout_pad_h(int cout);
s3r::ConvParamsH make_params_h(const s3r_conv_desc* d, const Geo& g);
int resolve_launch_h(const s3r_conv_desc* d, s3r::ConvParamsH* p, LaunchH* L);
s3r::ConvParams make_params(const s3r_conv_desc* d, const Geo& g);
int resolve_launch(const s3r_conv_desc* d, s3r::ConvParams* p, Launch* L);
int64_t align_up(int64_t v, int64_t a);
int plan_chain(const s3r_layer* layers, int n, Plan* pl);

// ---------------------------------------------------------------- argument checks shared by the entry points
// Each states one rule of include/s3r.h once; all run on the host, before anything is enqueued.  A check returns S3R_OK or fail(...).
inline int null_tensor() { return fail(S3R_ERR_INVALID, "null tensor pointer"); }
// bf16 tensors (channels-last activations, and the scratch / workspace that holds them) are read and written with 16-byte accesses
// whose addresses are base + a multiple of 16 bytes: the base must be 16-byte aligned (include/s3r.h, Conventions).  fp32 and int32
// tensors need their natural 4 bytes only
inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline int bf16_align_fail(const char* what, const void* p) {
    return fail(S3R_ERR_INVALID, "%s must be 16-byte aligned (got %p): bf16 tensors are accessed 16 bytes at a time", what, p);
}
// the stems fetch render rows by 16-byte vector loads / LDS-DMA from base + row * width (fp32 and 8-bit renders alike)
inline int check_renders_aligned(const void* left, const void* right) {
    if (!misaligned16(left) && !misaligned16(right)) return S3R_OK;
    return fail(S3R_ERR_INVALID, "render tensors must be 16-byte aligned (got %p, %p)", left, right);
}
// scratch NULL or smaller than the need; `who`: the entry's words in front of "needs", `query`: the size query to name
inline int need_scratch(int code, const char* who, int64_t need, const char* query, const void* scratch, int64_t scratch_elems) {
    if (scratch && scratch_elems >= need) return S3R_OK;
    return fail(code, "%s needs %lld floats of scratch (%s), got %lld", who, (long long)need, query, (long long)(scratch ? scratch_elems : 0));
}
// the end of an entry point: what its launch answered
inline int launched(hipError_t e, const char* what) { return e == hipSuccess ? S3R_OK : hip_fail(e, what); }
// the epilogues of the backward kernels know none / ReLU / sigmoid, and read y only where the activation's derivative needs it
inline int check_act(int act, const char* who) {
    if (act >= S3R_ACT_NONE && act <= S3R_ACT_SIGMOID) return S3R_OK;
    return fail(S3R_ERR_INVALID, "%s takes none / relu / sigmoid (act %d)", who, act);
}
inline int check_y(int act, const void* y, const char* who) {
    if (act == S3R_ACT_NONE || y) return S3R_OK;
    return fail(S3R_ERR_INVALID, "%s: y is NULL (it may be only when act is none)", who);
}
// The header's limits on one tensor (< 2^31 elements, < 4 GiB): true when the product of the first 1, 2, ... extents has 2^31 elements
// or more, or the whole tensor 4 GiB or more at `elem_bytes` bytes an element (1: the element limit is the tighter one).  Factor by
// factor, so no int64 product overflows whatever the extents.  An extent of 0 (an empty batch) makes every later product 0: list it
// FIRST where an empty call is never too large, LAST where its per-sample extents are still checked
inline bool too_large(std::initializer_list<int64_t> extents, int elem_bytes) {
    int64_t n = 1;
    for (int64_t e : extents) {
        if (e > 0 && n > (kMaxElems - 1) / e) return true;
        n *= e;
    }
    return elem_bytes * n >= kMaxBytes;
}
inline int too_large_fail() { return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the batch"); }
// tensors of a call that must not share memory (NULL: absent): byte spans, and the outputs against each other and the inputs
struct Span { const void* p; int64_t bytes; const char* name; };
inline bool overlap(const Span& a, const Span& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + (uintptr_t)b.bytes && y < x + (uintptr_t)a.bytes;
}
inline int check_overlaps(const char* who, const Span* outs, int n_outs, const Span* ins, int n_ins) {
    for (int i = 0; i < n_outs; ++i) {
        for (int j = i + 1; j < n_outs; ++j)
            if (overlap(outs[i], outs[j])) return fail(S3R_ERR_INVALID, "%s: %s and %s overlap", who, outs[i].name, outs[j].name);
        for (int j = 0; j < n_ins; ++j)
            if (overlap(outs[i], ins[j])) return fail(S3R_ERR_INVALID, "%s: %s overlaps the input %s", who, outs[i].name, ins[j].name);
    }
    return S3R_OK;
}

}  // namespace s3rh
