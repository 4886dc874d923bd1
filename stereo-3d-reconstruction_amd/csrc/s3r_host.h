// Host-side internals shared by the host translation units of libs3r_hip.so — s3r_prof.hip (event profiler), the planner's four
// units s3r_plan_geometry.hip / s3r_plan_algo.hip / s3r_plan_params.hip / s3r_plan_chain.hip (layer geometry; kernel policy and the
// sizes that follow; kernel parameter blocks; chain / arena planner), s3r_conv_forward.hip (one runner per kernel path, the
// dispatcher over them and their entry points) and s3r_api_layers.hip / s3r_api_tasks.hip (the other C-ABI entry points, by
// family); last, the argument checks those entry points share.  Not part of the ABI (include/s3r.h) and not seen by the kernel
// sources (those share s3r_kernels.h).  A planner helper's comment sits HERE, at its declaration, under the unit that defines it.
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

// ---------------------------------------------------------------- the plan's types
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

// the staged copy of a parameter-general layer's input; bmax > 0 (im2col): samples staged per pass; too_large: the copy would not fit
// one call's limits (then elems is 0: the int64 product may not exist)
struct StagedGeo { int cin_pad, step, pe, sp; int64_t elems; int bmax; bool too_large; };
// residue classes of a general ConvTranspose with dilation 1 (s3r_general.hip): class r of an axis = the outputs o with
// (o + pad) % stride == r; kr taps (0: none of that residue), ke >= 1 taps packed, positions q = qmin .. qmin + nq - 1 (nq <= 0: no output)
struct TClassAxis { int kr, ke, qmin, nq; };

struct Wino2Geo { int ax, m, n, ncls, out, sg, wp, kw, bmax; int64_t w_elems, v_sample, pos_sample; };
struct WinoNeed { int64_t v, slab, total; };
struct Dwino3Need { int64_t diff, total; bool split; };
// The packed image of an fp32 MFMA layer that is not staged, the ONE description packing, sizing and the runners share: convolution
// [direct | one-axis | two-axis], transposed [direct (8 classes x 8 taps) | two-axis classes | three-axis].  Floats; -1: no such slab
struct PackedLayout { int64_t direct, wino, dwino, wino2, dwino3, total; };
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

// membership in a constexpr table (the layout whitelists)
template <int N> inline bool one_of(int v, const int (&table)[N]) {
    for (int t : table)
        if (t == v) return true;
    return false;
}

// ---------------------------------------------------------------- s3r_plan_geometry.hip: errors, shapes, geometry, route, halos
int fail(int code, const char* fmt, ...);      // sets the thread-local message behind s3r_last_error, returns code
int hip_fail(hipError_t e, const char* what);
const char* last_error();
int64_t ipow(int64_t b, int e);
int64_t align_up(int64_t v, int64_t a);
int dil_of(const s3r_conv_desc* d);            // (a zero-initialised ABI-7 descriptor: 1)
int out_size(const s3r_conv_desc* d);
int cout_pad(int cout);                        // fp32 packed images: couts in whole 128-row tiles
int cout_pad_h(int cout);                      // bf16: 64
int cin_pad16(int k_rows);                     // K rows (channels; unfolded: channels x taps) in whole 16-row K tiles
// the transposed layer the tuned kernels serve (8 output-parity classes of 2 x 2 x 2 taps; Winograd forms)
bool deconv_fast(const s3r_conv_desc* d);
// Parameter-general layers (ABI 8, s3r_general.hip): an fp32 convolution whose channel count is not a multiple of 16, or any
// transposed convolution but the tuned one, runs the direct kernel over a STAGED copy of its input (channels zero-padded, the
// padding as a halo, transposed: zero-stuffed at the stride).  Correct first; the network's own shapes never take this path.
bool staged_layer(const s3r_conv_desc* d);
// A staged ConvTranspose with dilation 1 runs as stride^ndim residue classes over the halo-padded (not stuffed) input
bool tclass_layer(const s3r_conv_desc* d);
// ... and WITHOUT the staged copy when its input already carries the halo the classes read and whole 16-channel K tiles: what
// s3r_chain_forward plans for such a layer behind another one (want_halo), or a caller states with in_halo
bool tclass_direct(const s3r_conv_desc* d);
// ... and a residue-class layer with k == stride, pad 0, out_pad 0 (every class is ONE tap on the same input element): one GEMM over
// cout x taps rows with a depth-to-space store instead of stride^ndim launches
bool tshuf_layer(const s3r_conv_desc* d);
TClassAxis tclass_axis(const s3r_conv_desc* d, int r);
int tclass_halo(const s3r_conv_desc* d);                             // the widest border any class reads
int64_t tclass_w_elems(const s3r_conv_desc* d);                      // the s^nd class slabs, in class order
// a staged convolution with cin <= 8: unfolded to a 1 x 1 GEMM over cin k^nd rows.  Decided from the layer's PER-SAMPLE geometry only:
// the packed weights have the unfolded layout, and they are packed once for every batch; a batch whose unfolded copy would pass 1 GiB
// goes through in sub-batches
bool im2col_layer(const s3r_conv_desc* d);
StagedGeo staged_geo(const s3r_conv_desc* d);
// the staged tensor as a residue-class layer's kernel reads it: the staged copy, or (tclass_direct) the layer's own input in place,
// whose halo is the classes' border
StagedGeo tclass_input_geo(const s3r_conv_desc* d);
// LeakyReLU with a slope in [0, 1] is max(t, slope t): the direct kernel's epilogue and its split-K finish apply it themselves (r06: a
// DispNet-style network has it behind every convolution; as a pass of its own it cost every layer a round trip of its output)
bool leaky_fused(const s3r_conv_desc* d);
bool needs_act_pass(const s3r_conv_desc* d);
// validates the descriptor and fills g; a staged layer builds its own halo of any width — what bounds it is the size of the staged
// copy, checked HERE so that planning and the forward agree
int geometry(const s3r_conv_desc* d, Geo* g);
int route(const s3r_conv_desc* d, Route* r);           // which kernel serves a layer shape (halos are checked separately, by check_halos)
// input halo the layer's kernel needs (the MFMA gather reads its zero padding from memory; a staged layer builds its own padded copy)
int need_halo(const s3r_conv_desc* d, Route r);
// the halo a chain gives the layer's input when it can choose (>= need_halo): a residue-class ConvTranspose with whole K tiles reads
// its border from the producer's zero halo instead of staging a padded copy
int want_halo(const s3r_conv_desc* d, Route r);
int check_halos(const s3r_conv_desc* d, Route r);

// ---------------------------------------------------------------- s3r_plan_algo.hip: which algorithm and launch form, and every size that follows
// Winograd along H (s3r_wino_axis1.hip, s3r_wino_gemm.hip) for the fp32 3 x 3 [x 3] stride-1 pad-1 convolutions (F(4,3): 1/2 of the matrix work, F(2,3):
// 2/3) and the transposed convolutions (F(2,2) along D and H inside the parity classes: 9/16): another summation order than the direct
// kernels' — same fp32 accuracy, other bits.  Such a layer's packed weights hold BOTH forms (the direct slab, then the class
// slabs); which kernel a call runs is the descriptor's `algo` (include/s3r.h): AUTO resolves from the layer's per-sample
// geometry (and the descriptor's own tile / split-K / layout fields) alone — never from the scratch a caller offers or the
// batch — under the process-level policy S3R_WINO, read once:
//   unset / 1: every layer that has the form (e2, e4, e6, e7, v1, v3, v5, d1, d2, d3 of this network: each measured faster on it at
//   B = 32, and — with the class-parallel launch form on sparse grids — at every smaller batch);  0: never.
int wino_mode();
// outputs per Winograd group along H of an fp32 3 x 3 [x 3] stride-1 convolution: F(4,3), half the direct form's multiplications.
// Edges that are not a multiple of 4 compute a partial last group (v3: 16 rows for 14, v5: 8 for 7) and still beat F(2,3), which
// r03 used for them (v3 0.505 -> 0.431 ms, v5 0.304 -> 0.251 alone at B = 32): one group size, one class kernel.
int wino_r(const s3r_conv_desc*);
// structural: the layer has a Winograd form (decides the packed layout; independent of any switch)
bool wino_layer(const s3r_conv_desc* d);
bool dwino_layer(const s3r_conv_desc* d);
// the three-axis form of a transposed layer (s3r_deconv_wino3.hip): whole padded rows per 64-position tile
bool dwino3_layer(const s3r_conv_desc* d);
bool dwino3_desc_ok(const s3r_conv_desc* d);
bool wino_desc_ok(const s3r_conv_desc* d);             // the descriptor can run its layer's (one-axis / transposed) Winograd form
// Two-axis class-parallel Winograd (s3r_wino_axis2.hip): the stride-1 layers with a small edge — Conv3d k3 p1 as F(4,3) x F(4,3)
// over D and H (returns 0), Conv3d k4 p0 as F(2,4) x F(2,4) (returns 1), Conv2d k3 p1 as F(4,3) x F(4,3) over H and W (returns 2);
// -1: the layer has no such form
int wino2_ax(const s3r_conv_desc* d);
bool wino2_desc_ok(const s3r_conv_desc* d);
// The LDS rule of the two-axis finish kernels (s3r_wino_axis2.hip, launch_conv_wino2: it keeps its own checks).  Both stage PADDED
// output planes in 64 KiB: the Conv2d finish one plane, (out + 2 out_halo)^2 floats, hence a padded edge <= 128 (a layer writing
// its consumer's plane sets stages the halo-1 plane: always inside, the edge stops at 124); the semi-fused Conv3d finish four
// slices, hence a padded edge <= 64.  The class-parallel Conv3d form stages nothing.  Part of the PLAN: a descriptor outside the
// rule is refused by resolve_algo (or planned in the class-parallel form), never by the launcher behind an enqueued transform
bool wino2_plane_fits(const s3r_conv_desc* d);
bool wino2_semi_fits(const s3r_conv_desc* d);
// library policy: the two-axis form where the output is small enough for its class slabs (ncls / m^2 x the output) to be cheap
// or, in its semi-fused launch form (6 / 4 x the output), worth the halved matrix work — v1 (edge 28), v3 (14), v5, v6 (7) of this
// network: every 3D stride-1 layer; S3R_WINO2_MAX_EDGE (read once) moves the bound for experiments
int wino2_max_edge();
// the algorithm a descriptor resolves to; *form = the forced launch form of the one-axis kernel, or -1
int resolve_algo(const s3r_conv_desc* d, int* alg, int* form);
bool resolves_to_wino(const s3r_conv_desc* d);
// Element count of a transformed operand of `nb` samples, stated once.  The plane sets of a two-axis kernel of form `ax` over C
// channels, `out` = the consumer's OUTPUT edge (groups per axis: ceil(out / m)), `wp` its padded input edge; ax 2: [36][C][positions of
// the nb samples rounded up to whole GEMM tiles] ...
int64_t wino2_operand_elems(int ax, int C, int out, int wp, int64_t nb);
// ... and any S3R_LAYOUT_WINO_* operand of the consumer `c` (WINO_H: [R + 2][nb][Cin][Dp][ceil(H / R)][Wp])
int64_t operand_elems(const s3r_conv_desc* c, int layout, int64_t nb);
// samples per call: one call's transformed input stays below 2 GiB (32-bit byte offsets); never more than the batch
int call_samples(int64_t per_sample_elems, int batch);
Wino2Geo wino2_geo(const s3r_conv_desc* d);
int wino_bmax(const s3r_conv_desc* d);                 // call_samples of the one-axis form
// the whole batch's operand of `alg` (ALG_WINO / ALG_WINO2) fits ONE call: what a producer-written operand needs
bool fits_one_call(const s3r_conv_desc* d, int alg);
// Inputs too large for 32-bit byte offsets go through in sub-batches of bmax samples (a sample's result does not depend on the batch
// it is computed in, so neither does it on this split): the samples of the sub-batch that starts at b0
inline int sub_batch(int batch, int b0, int bmax) { return batch - b0 < bmax ? batch - b0 : bmax; }
int64_t wino_w_elems(const s3r_conv_desc* d);          // the R + 2 class slabs behind the direct slab
int64_t dwino_w_elems(const s3r_conv_desc* d);         // (parity class, class) x 2 taps
PackedLayout packed_layout(const s3r_conv_desc* d, const Geo& g);
// The depth differences of the transposed Winograd form are materialised (two more tensors behind the row differences) while
// the four tensors stay in the Infinity Cache, and formed inside the class kernel otherwise: same bits either way, so this
// may follow the batch (s3r_wino_gemm.hip).
bool dwino_materialise(const s3r_conv_desc* d);
int64_t dwino_d_elems(const s3r_conv_desc* d);
int wino_kind(const s3r_conv_desc* d);
int wino_kcls(const s3r_conv_desc* d);                 // K per class: Cin x (depth taps x column taps)
int64_t wino_positions(const s3r_conv_desc* d, int nb);      // GEMM positions (groups of R output rows) of nb samples
// Scratch of a Winograd call: [transformed input V (a convolution fed with plain input) | the difference tensors (transposed) ] then
// the class-parallel slabs of the launch form the library plans for this batch (every form gives the same bits, so the form
// — unlike the algorithm — may follow the batch).  form < 0, the library's pick: sized for the class-parallel form, the largest — the
// pick counts workgroups against the current device's compute units, and a size query must not depend on the device
WinoNeed wino_need(const s3r_conv_desc* d, int form, bool head);
// the launch form of a two-axis call (0 class-parallel, 1 semi-fused): the library's plan unless forced; a 3D layer whose four padded
// output slices do not fit the semi-fused finish kernel's LDS WITH THIS out_halo (wino2_semi_fits) stays class-parallel
int wino2_form_of(const s3r_conv_desc* d, int ntotal, int forced);
// scratch of a two-axis call: [V of one sub-batch (unless the producer wrote it) | slabs of the launch form planned for the batch]
WinoNeed wino2_need(const s3r_conv_desc* d, int form);
// scratch of the three-axis form: [Dh | Dd | Ddh] then, class-parallel form only, the slabs
Dwino3Need dwino3_need(const s3r_conv_desc* d, int form);
double wino_exec_flops(const s3r_conv_desc* d, const Geo& g);      // MFMA FLOPs the Winograd form executes for the whole batch
double wino2_exec_flops(const s3r_conv_desc* d);

// ---------------------------------------------------------------- s3r_plan_params.hip: kernel parameter blocks and launch forms
// the divisors of the conv kernels' position decode, from the positions per sample (Nd, Nh, Nw)
inline void set_divs(s3r::ConvParams& p) {
    p.dS = s3r::FastDiv((unsigned)(p.Nd * p.Nh * p.Nw));
    p.dHW = s3r::FastDiv((unsigned)(p.Nh * p.Nw));
    p.dW = s3r::FastDiv((unsigned)p.Nw);
}
s3r::ConvParams make_params(const s3r_conv_desc* d, const Geo& g);
// bf16 channels-last twin of make_params: strides are in elements of (B, Dp, Hp, Wp, C)
s3r::ConvParamsH make_params_h(const s3r_conv_desc* d, const Geo& g);
// a staged layer as the direct kernel sees it: a convolution (stride 1 if the layer is transposed) over the staged tensor, whose
// halo is exactly the effective padding
s3r::ConvParams make_params_staged(const s3r_conv_desc* d, const Geo& g);
s3r::ConvParams make_params_tshuf(const s3r_conv_desc* d, const Geo& g);
// class (rd, rh, rw) as the direct kernel sees it: a stride-1 convolution over the staged tensor; false: the class has no output.
// *w_off = floats from the start of the packed image to the class's slab; *macs = its multiply-adds (CinPad channels)
bool make_params_tclass(const s3r_conv_desc* d, const Geo& g, int rd, int rh, int rw, s3r::ConvParams* q, int64_t* w_off, double* macs);
// (tile cfg, gather width, split-K) of an MFMA-route layer: the caller's forced values or the heuristics
int resolve_launch(const s3r_conv_desc* d, s3r::ConvParams* p, Launch* L);
// (position-tile multiplier TM, split-K) of a bf16 MFMA layer
int resolve_launch_h(const s3r_conv_desc* d, s3r::ConvParamsH* p, LaunchH* L);
// the direct kernel of the WHOLE layer as planned: make_params[_h] + resolve_launch[_h] ...
int plan_direct(const s3r_conv_desc* d, const Geo& g, s3r::ConvParams* p, Launch* L);
int plan_direct_h(const s3r_conv_desc* d, const Geo& g, s3r::ConvParamsH* p, LaunchH* L);
// ... and whether it splits K, fp32 or bf16 (split-K follows the per-sample geometry alone)
int direct_ksplit(const s3r_conv_desc* d, const Geo& g, int* ksplit);

// ---------------------------------------------------------------- s3r_plan_chain.hip: hand-offs, head fusion, the arena
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
