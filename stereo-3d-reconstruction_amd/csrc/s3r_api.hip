// C-ABI of libs3r_hip.so (declared in include/s3r.h).  Top to bottom: what every forward convolution shares (ConvCall, the scratch /
// launch / activation helpers), ONE runner per kernel path (run_*), the dispatcher over them (conv_forward_impl: validation and a
// switch, no launch), the fused conv + head launch and the chain walker; then ONE extern "C" block of entry points.  Planning (geometry,
// kernel policy, sizes, the packed image's layout, the arena) lives in s3r_plan.hip, the profiler in s3r_prof.hip.  Host code only.
#include "s3r_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>

using namespace s3rh;

namespace {

// bf16 tensors (channels-last activations, and the scratch / workspace that holds them) are read and written with 16-byte accesses
// whose addresses are base + a multiple of 16 bytes: the base must be 16-byte aligned (include/s3r.h, Conventions).  fp32 and int32
// tensors need their natural 4 bytes only.  Checked on the host, before anything is enqueued
inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
int bf16_align_fail(const char* what, const void* p) {
    return fail(S3R_ERR_INVALID, "%s must be 16-byte aligned (got %p): bf16 tensors are accessed 16 bytes at a time", what, p);
}

// ---------------------------------------------------------------- one forward call, and what its runners share
// x2 != NULL (stem only): images [0, nsplit) are read from x, images [nsplit, batch) from x2 (left / right renders of a stereo batch:
// no concatenation copy); x_u8 != 0 (stem only): x / x2 are 8-bit renders, scaled by 1/255 inside the stem kernel
struct ConvCall {
    const s3r_conv_desc* d;
    Geo g;
    const void* x; const void* x2; int nsplit, x_u8;
    const void* w; const float* scale; const float* shift;      // w: the packed image (s3r_conv_pack_weights)
    void* y;
    float* scratch; int64_t scratch_elems;
    hipStream_t s;
    const float* xf() const { return static_cast<const float*>(x); }
    const float* wf() const { return static_cast<const float*>(w); }
    float* yf() const { return static_cast<float*>(y); }
};

// what a fused 1x1 head adds to its layer's profiler record (bytes: the head's output in place of the layer's)
struct HeadWork { double flops, bytes; };
constexpr HeadWork kNoHead = {0.0, 0.0};
s3r::ConvParams bind(const ConvCall& c, s3r::ConvParams p) {
    p.x = c.xf(); p.w = c.wf(); p.scale = c.scale; p.shift = c.shift; p.y = c.yf();
    return p;
}

// scratch NULL or too small is S3R_ERR_WORKSPACE, never another kernel; `who`: the path's own words in front of the need
int check_scratch(const ConvCall& c, int64_t need, const char* who) {
    if (c.scratch && c.scratch_elems >= need) return S3R_OK;
    return fail(S3R_ERR_WORKSPACE, "%s %lld floats of scratch (s3r_conv_scratch_elems), got %lld", who, (long long)need,
                (long long)(c.scratch ? c.scratch_elems : 0));
}
int check_splitk_scratch(const ConvCall& c, int ksplit, int64_t need) {      // (never answered unsplit: another summation order is other bits)
    char who[32];
    snprintf(who, sizeof(who), "ksplit=%d needs", ksplit);
    return check_scratch(c, need, who);
}

// the stems fetch render rows by 16-byte vector loads / LDS-DMA from base + row * width (fp32 and 8-bit renders alike)
int check_stem_input(const s3r_conv_desc* d, const void* x, const void* x2, int nsplit) {
    if (x2 && (nsplit <= 0 || nsplit >= d->batch)) return fail(S3R_ERR_INVALID, "split %d outside (0, batch=%d)", nsplit, d->batch);
    if (misaligned16(x) || misaligned16(x2)) return fail(S3R_ERR_INVALID, "render tensors must be 16-byte aligned (got %p, %p)", x, x2);
    return S3R_OK;
}

int launched(const ConvCall& c, hipError_t e) {
    return e == hipSuccess ? S3R_OK : hip_fail(e, c.d->dtype == S3R_BF16 ? "conv forward launch (bf16)" : "conv forward launch");
}

// the direct kernel on the tile / gather width resolve_launch picked; its launches and launch form go into the layer's record
int launch_direct(const s3r::ConvParams& p, const Launch& L, hipStream_t s, ProfScope& ps, const char* what) {
    s3r::ConvLaunchInfo info;
    const hipError_t e = s3r::launch_conv_mfma(p, L.cfg + 16 * L.vec, s, &info);
    ps.launches += info.launches; ps.form |= info.form;
    return e == hipSuccess ? S3R_OK : hip_fail(e, what);
}

// ELU / Tanh / LeakyReLU with a slope outside [0, 1]: a pass behind the kernel, which ran with ACT_NONE (make_params)
int act_pass(const ConvCall& c, ProfScope& ps, const char* what) {
    s3r::AuxScope aux(c.s, 8.0 * (double)c.g.y_elems);
    const hipError_t e = s3r::launch_act(c.yf(), c.g.y_elems, c.d->act, c.d->act_param, c.s);
    if (e != hipSuccess) return hip_fail(e, what);
    ps.launches += 1;
    return S3R_OK;
}

// Inputs too large for 32-bit byte offsets go through in sub-batches (a sample's result does not depend on the batch it is computed
// in, so neither does it on this split): samples [b0, b0 + nb) of the call, x_sample floats of (staged / transformed) input each
inline int sub_batch(int batch, int b0, int bmax) { return batch - b0 < bmax ? batch - b0 : bmax; }
void set_sub_batch(s3r::ConvParams& p, float* y, int b0, int nb, int64_t x_sample) {
    p.B = nb; p.Ntotal = nb * p.Nd * p.Nh * p.Nw;
    p.x_bytes = (unsigned)(4 * (int64_t)nb * x_sample);
    p.y = y + (int64_t)b0 * p.y_bs;
    p.y_bytes = (unsigned)(4 * (int64_t)nb * p.y_bs);
}

// ---------------------------------------------------------------- stem, head, linear, bf16 MFMA
int run_stem(const ConvCall& c) {
    const s3r_conv_desc* d = c.d; const Geo& g = c.g;
    if (!c.scale || !c.shift) return fail(S3R_ERR_INVALID, "stem needs scale and shift");
    const double u8_saved = c.x_u8 ? 3.0 * d->batch * d->cin * (double)g.in_sp : 0.0;      // algorithmic bytes: 1 instead of 4 per sample
    ProfScope ps(c.s, F_STEM, d->tag, g.flops, g.bytes - u8_saved);
    if (d->dtype == S3R_BF16)      // (channels-last: the 32 couts are the innermost stride)
        return launched(c, s3r::launch_stem_bf16(c.x, c.x2, c.x_u8, c.nsplit, c.wf(), c.scale, c.shift, c.y, d->batch, g.in, g.in, g.out, g.out,
                                                 g.out_p * g.out_p * 32, g.out_p * 32, d->out_halo * (g.out_p + 1) * 32, c.s));
    return launched(c, s3r::launch_stem(c.x, c.x2, c.x_u8, c.nsplit, c.wf(), c.scale, c.shift, c.yf(), d->batch, g.in, g.in, g.out, g.out,
                                        g.out_p * g.out_p, g.out_p, d->out_halo * (g.out_p + 1), c.s));
}

int run_head(const ConvCall& c) {
    const s3r_conv_desc* d = c.d;
    ProfScope ps(c.s, F_HEAD, d->tag, c.g.flops, c.g.bytes);
    if (d->dtype == S3R_BF16)
        return launched(c, s3r::launch_head_bf16(c.x, c.wf(), c.scale, c.shift, c.yf(), d->cin, (int64_t)d->batch * c.g.in_sp, d->act, c.s));
    return launched(c, s3r::launch_head(c.xf(), c.wf(), c.scale, c.shift, c.yf(), d->batch, d->cin, c.g.in_sp, d->act, c.s));
}

int run_linear(const ConvCall& c) {
    const s3r_conv_desc* d = c.d;
    int rc = check_scratch(c, s3r::linear_scratch_elems(d->batch, d->cin, d->cout), "linear layer needs");
    if (rc) return rc;
    ProfScope ps(c.s, F_LINEAR, d->tag, c.g.flops, c.g.bytes);
    // (the linear epilogue knows none / ReLU / sigmoid; LeakyReLU / ELU / Tanh are a pass behind it, as on the convolutions)
    const bool pass = d->act > S3R_ACT_SIGMOID;
    hipError_t e = s3r::launch_linear(c.xf(), c.wf(), c.scale, c.shift, c.yf(), d->batch, d->cin, d->cout, pass ? S3R_ACT_NONE : d->act,
                                      c.scratch, c.s);
    if (e == hipSuccess && pass) e = s3r::launch_act(c.yf(), c.g.y_elems, d->act, d->act_param, c.s);
    return launched(c, e);
}

int run_mfma_bf16(const ConvCall& c) {
    s3r::ConvParamsH p = make_params_h(c.d, c.g);
    p.x = c.x; p.w = c.w; p.scale = c.scale; p.shift = c.shift; p.y = c.y;
    LaunchH L;
    int rc = resolve_launch_h(c.d, &p, &L);
    if (rc) return rc;
    if (L.ksplit > 1) {
        if ((rc = check_splitk_scratch(c, L.ksplit, s3r::conv_bf16_scratch_elems(p, L.tm)))) return rc;
        p.part = c.scratch;
    }
    ProfScope ps(c.s, F_MFMA, c.d->tag, c.g.flops, c.g.bytes);
    return launched(c, s3r::launch_conv_bf16(p, L.tm, c.s));
}

// ---------------------------------------------------------------- parameter-general layers: the direct kernel behind a staged copy
// `xs`: the staged copy, or the layer's own input where it already carries the halo (tclass_direct).  None of them splits K
// cin <= 8: unfold (sub-batches of sg.bmax samples) -> a 1 x 1 GEMM per pass
int run_unfolded(const ConvCall& c, const StagedGeo& sg, ProfScope& ps) {
    const s3r_conv_desc* d = c.d; const Geo& g = c.g;
    s3r::ConvParams q = bind(c, make_params_staged(d, g));
    q.x = c.scratch;
    s3r_conv_desc di = *d; di.ksplit = 1;
    const int64_t x_sample = g.x_elems / d->batch, s_sample = sg.elems / (d->batch < sg.bmax ? d->batch : sg.bmax);
    for (int b0 = 0; b0 < d->batch; b0 += sg.bmax) {
        const int nb = sub_batch(d->batch, b0, sg.bmax);
        hipError_t e;
        {
            s3r::AuxScope aux(c.s, 4.0 * ((double)nb * x_sample + (double)nb * s_sample));
            e = s3r::launch_stage_im2col(c.xf() + (int64_t)b0 * x_sample, c.scratch, nb, d->cin, sg.cin_pad, g.nd, d->in_size, d->in_halo,
                                         sg.sp, d->k, d->stride, d->pad, dil_of(d), c.s);
        }
        if (e != hipSuccess) return hip_fail(e, "unfolding launch");
        s3r::ConvParams p = q;
        set_sub_batch(p, c.yf(), b0, nb, s_sample);
        Launch L;
        int rc = resolve_launch(&di, &p, &L);
        if (rc || (rc = launch_direct(p, L, c.s, ps, "conv forward launch (unfolded)"))) return rc;
        ps.launches += 1;      // (the unfolding pass)
    }
    ps.exec = 2.0 * d->batch * (double)d->cout * (double)g.out_sp * sg.cin_pad;
    return S3R_OK;
}

// ConvTranspose with k == stride: ONE 1 x 1 GEMM over (cout, tap) rows, depth-to-space store
int run_depth_to_space(const ConvCall& c, const float* xs, ProfScope& ps) {
    s3r::ConvParams p = bind(c, make_params_tshuf(c.d, c.g));
    p.x = xs;
    s3r_conv_desc dd = *c.d; dd.ksplit = 1; dd.tile = -1; dd.cout = p.Cout;
    Launch L;
    int rc = resolve_launch(&dd, &p, &L);
    if (rc || (rc = launch_direct(p, L, c.s, ps, "conv forward launch (depth-to-space)"))) return rc;
    ps.exec = 2.0 * (double)p.Ntotal * p.Cin * (double)p.Cout;
    return S3R_OK;
}

// ConvTranspose, dilation 1: the residue classes of the output, each a stride-1 convolution — ONE launch over a class table (up to
// kTClsMax classes), one launch per class beyond that
int run_classes(const ConvCall& c, const float* xs, ProfScope& ps) {
    const s3r_conv_desc* d = c.d;
    s3r_conv_desc dd = *d; dd.ksplit = 1; dd.tile = -1;
    const int ncls = (int)ipow(d->stride, c.g.nd);
    s3r::TClsTable tab; tab.n = 0;
    s3r::ConvParams base;
    int64_t w_first = 0;
    double macs_all = 0.0;
    for (int cls = 0; cls < ncls; ++cls) {
        const int rw = cls % d->stride, rh = (cls / d->stride) % d->stride, rd = c.g.nd == 3 ? cls / (d->stride * d->stride) : 0;
        s3r::ConvParams p; int64_t w_off; double macs;
        if (!make_params_tclass(d, c.g, rd, rh, rw, &p, &w_off, &macs)) continue;      // (a class with no output)
        p = bind(c, p);
        p.x = xs; p.w = c.wf() + w_off;
        macs_all += macs;
        if (ncls <= s3r::kTClsMax) {
            if (tab.n == 0) { base = p; w_first = w_off; }
            s3r::TClsEntry& t = tab.e[tab.n++];
            t.Nd = p.Nd; t.Nh = p.Nh; t.Nw = p.Nw; t.kd = p.kd; t.kh = p.kh; t.kw = p.kw; t.T = p.T;
            t.x_org = p.x_org; t.y_org = p.y_org; t.Ntotal = p.Ntotal; t.wg_begin = 0; t.w_off = (int)(w_off - w_first);
            t.dS = p.dS; t.dHW = p.dHW; t.dW = p.dW;
            continue;
        }
        Launch L;
        int rc = resolve_launch(&dd, &p, &L);
        if (rc || (rc = launch_direct(p, L, c.s, ps, "conv forward launch (transposed class)"))) return rc;
    }
    if (tab.n > 0) {
        const hipError_t e = s3r::launch_conv_tcls(base, tab, c.s);
        if (e != hipSuccess) return hip_fail(e, "conv forward launch (transposed classes)");
        ps.launches += 1;
    }
    ps.exec = 2.0 * macs_all;
    return S3R_OK;
}

// staged copy -> one of the forms above, or the direct kernel as it is -> [activation pass]
int run_staged(const ConvCall& c) {
    const s3r_conv_desc* d = c.d; const Geo& g = c.g;
    ProfScope ps(c.s, F_MFMA, d->tag, g.flops, g.bytes);
    ps.launches = 0;
    const bool in_place = tclass_direct(d);
    const StagedGeo sg = staged_geo(d);
    int rc = in_place ? S3R_OK : check_scratch(c, (sg.elems + 255) / 256 * 256, "a parameter-general layer stages its input in");
    if (rc) return rc;
    if (im2col_layer(d)) {
        rc = run_unfolded(c, sg, ps);
    } else {
        if (!in_place) {
            s3r::AuxScope aux(c.s, 4.0 * ((double)g.x_elems + (double)sg.elems));
            const hipError_t e = s3r::launch_stage(c.xf(), c.scratch, d->batch, d->cin, sg.cin_pad, g.nd, d->in_size, d->in_halo, sg.sp, sg.pe,
                                                   sg.step, c.s);
            ps.launches += 2;
            if (e != hipSuccess) return hip_fail(e, "staging launch");
        }
        const float* xs = in_place ? c.xf() : c.scratch;
        if (tshuf_layer(d)) {
            rc = run_depth_to_space(c, xs, ps);
        } else if (tclass_layer(d)) {
            rc = run_classes(c, xs, ps);
        } else {
            s3r::ConvParams q = bind(c, make_params_staged(d, g));
            q.x = xs;
            s3r_conv_desc dd = *d; dd.ksplit = 1;
            Launch L;
            ps.exec = 2.0 * d->batch * (double)d->cout * (double)g.out_sp * sg.cin_pad * (double)ipow(d->k, g.nd);
            if (!(rc = resolve_launch(&dd, &q, &L))) rc = launch_direct(q, L, c.s, ps, "conv forward launch");
        }
    }
    if (rc) return rc;
    return needs_act_pass(d) ? act_pass(c, ps, "activation launch") : S3R_OK;
}

// ---------------------------------------------------------------- Winograd: one runner per form, each with its layer's record
// All four re-aim the layer's ConvParams (make_params, bound; with the head's fields where one rides along) at their form's operand
// and slab of the packed image (packed_layout)

// exec / algo of a Winograd layer's record (the runners refine algo by the launch form that ran)
void wino_prof(ProfScope& ps, const ConvCall& c, int alg, const HeadWork& head) {
    if (alg == ALG_WINO2) { ps.exec = wino2_exec_flops(c.d); ps.algo = 4; }
    else if (alg == ALG_WINO3) { ps.exec = c.g.flops * (27.0 / 64.0) + head.flops; ps.algo = 5; }
    else ps.exec = wino_exec_flops(c.d, c.g) + head.flops;
}

// one axis, F(R, 3) along H: input transform + class kernel, in sub-batches
int run_wino1(const ConvCall& c, s3r::ConvParams p, int form, const HeadWork& head) {
    const s3r_conv_desc* d = c.d; const Geo& g = c.g;
    const bool pre = d->in_layout == S3R_LAYOUT_WINO_H;      // the producer wrote the transformed planes
    const int R = wino_r(d), is3 = d->ndim == 3, n = d->in_size, wp = n + 2, h2 = (n + R - 1) / R, dp = is3 ? n + 2 : 1;
    const int bmax = wino_bmax(d);
    if (bmax <= 0 || (pre && bmax < d->batch))
        return fail(S3R_ERR_INVALID, "a Winograd-transformed input takes at most %d samples per call here "
                    "(s3r_conv_wino_input_elems)", bmax);
    const WinoNeed need = wino_need(d, form, false);
    int rc = need.total > 0 ? check_scratch(c, need.total, "the Winograd form of this layer needs") : S3R_OK;
    if (rc) return rc;
    const int64_t v_sample = wino_v_elems(d) / d->batch, x_sample = g.x_elems / d->batch;
    ProfScope ps(c.s, F_MFMA, d->tag, g.flops + head.flops, g.bytes + head.bytes);
    wino_prof(ps, c, ALG_WINO, head);
    ps.launches = 0;
    p.w = c.wf() + packed_layout(d, g).wino;
    p.x = pre ? c.xf() : c.scratch;
    p.part = c.scratch ? c.scratch + need.v : nullptr;
    p.Nh = h2; p.T = p.kd * p.kw;
    p.x_hs = wp; p.x_ds = is3 ? h2 * wp : 0; p.x_cs = dp * h2 * wp;
    p.x_org = 0;
    set_divs(p);
    p.Hout = n;
    p.ksplit = 1;
    for (int b0 = 0; b0 < d->batch; b0 += bmax) {
        const int nb = sub_batch(d->batch, b0, bmax);
        hipError_t e;
        if (!pre) {
            s3r::AuxScope aux(c.s, 4.0 * ((double)nb * x_sample + (double)nb * v_sample));
            e = s3r::launch_wino_input(c.xf() + (int64_t)b0 * x_sample, c.scratch, (long long)nb * d->cin * dp, n + 2, wp, h2, R, c.s);
            if (e != hipSuccess) return hip_fail(e, "Winograd input transform launch");
            ps.launches += 1;
        }
        set_sub_batch(p, c.yf(), b0, nb, v_sample);
        p.x_cls = nb * d->cin * p.x_cs;
        const s3r::WinoLaunch WL = s3r::wino_plan(wino_kind(d), d->cout, wino_kcls(d), p.Ntotal, false, form);
        int nl = 0;
        e = s3r::launch_conv_wino(p, WL, c.s, &nl);
        if (e != hipSuccess) return hip_fail(e, "Winograd conv launch");
        ps.launches += nl;
        ps.algo = 1 + WL.mode;
    }
    return S3R_OK;
}

// two axes: input transform + class kernel + finish, in sub-batches
int run_wino2(const ConvCall& c, s3r::ConvParams p, int form, const HeadWork& head) {
    const s3r_conv_desc* d = c.d; const Geo& g = c.g;
    ProfScope ps(c.s, F_MFMA, d->tag, g.flops + head.flops, g.bytes + head.bytes);
    wino_prof(ps, c, ALG_WINO2, head);
    const Wino2Geo g2 = wino2_geo(d);
    const WinoNeed need = wino2_need(d, form);
    const bool pre = d->in_layout == S3R_LAYOUT_WINO_DH || d->in_layout == S3R_LAYOUT_WINO_HW ||
                     d->in_layout == S3R_LAYOUT_WINO_3D;             // the producer wrote the plane sets
    const bool to_v = d->out_layout == S3R_LAYOUT_WINO_HW;           // ... and this layer writes its consumer's
    // ... or (3D) its consumer's operand from ONE pass in place of the finish pass: ConvParams::out_mode
    p.out_mode = d->out_layout == S3R_LAYOUT_WINO_3D ? (d->out_halo ? 1 : 2) : d->out_layout == S3R_LAYOUT_DIFF ? 3 : 0;
    if (p.out_mode && (g2.ax > 1 || wino2_form_of(d, (int)(g2.pos_sample * d->batch), form) != 0))
        return fail(S3R_ERR_INVALID, "a consumer's operand is written from the class-parallel launch form of a 3D two-axis layer only (the semi-fused "
                    "form of this batch keeps the plain output: s3r_chain_forward plans that itself)");
    if (g2.bmax <= 0 || ((pre || to_v || p.out_mode) && g2.bmax < d->batch))
        return fail(S3R_ERR_INVALID, "two-axis Winograd form: the transformed input of this batch exceeds 2 GiB (at most %d samples per "
                    "call with a producer-written input: s3r_conv_wino_input_elems)", g2.bmax);
    int rc = check_scratch(c, need.total, "the two-axis Winograd form of this layer needs");
    if (rc) return rc;
    p.w = c.wf() + packed_layout(d, g).wino2;
    p.x = pre ? c.xf() : c.scratch;
    p.part = c.scratch + need.v;
    p.Nd = g2.sg; p.Nh = g2.sg; p.Nw = g2.out;
    p.kd = 1; p.kh = 1; p.kw = g2.kw; p.T = g2.kw;
    p.x_hs = g2.wp; p.x_ds = g2.sg * g2.wp; p.x_cs = g2.sg * g2.sg * g2.wp;
    p.x_org = 0;
    set_divs(p);
    if (g2.ax == 2) {                                     // (the finish kernel's view; launch_conv_wino2 derives the class GEMM's)
        p.Nd = 1; p.Nw = g2.sg;
        p.dS = s3r::FastDiv((unsigned)(g2.sg * g2.sg));
        p.dW = s3r::FastDiv((unsigned)g2.sg);
    }
    p.Hout = g2.out; p.Dout = g2.out;
    p.ncls = g2.ncls;
    p.ksplit = 1;
    // S3R_LAYOUT_WINO_DH is what s3r_cost_volume_forward_wino2 wrote, column outside the row group (include/s3r.h): launch_conv_wino2
    // re-aims the class GEMM at that order and leaves out the K tiles that hold the volume's structural zeros
    p.cv_n = d->in_layout == S3R_LAYOUT_WINO_DH ? g2.out : 0;
    const int64_t x_sample = g.x_elems / d->batch;
    ps.launches = 0;
    for (int b0 = 0; b0 < d->batch; b0 += g2.bmax) {
        const int nb = sub_batch(d->batch, b0, g2.bmax);
        hipError_t e = hipSuccess;
        if (!pre) {
            // (aux pass: reads the padded input once, writes its ncls plane sets)
            s3r::AuxScope aux(c.s, 4.0 * ((double)nb * x_sample + (double)(g2.ax == 2 ? g2.ncls * d->cin * s3r::wino2_npad(g2.pos_sample * nb) : g2.v_sample * nb)));
            if (g2.ax == 2)
                e = s3r::launch_wino2p_input(c.xf() + (int64_t)b0 * x_sample, c.scratch, nb, d->cin, g2.wp, g2.wp, g2.sg, g2.sg,
                                             s3r::wino2_npad(g2.pos_sample * nb), c.s);
            else
                e = s3r::launch_wino2_input(c.xf() + (int64_t)b0 * x_sample, c.scratch, g2.ax, (long long)nb * d->cin, g2.wp, g2.wp, g2.wp, g2.sg,
                                            g2.sg, c.s);
            if (e != hipSuccess) return hip_fail(e, "two-axis Winograd input transform launch");
            ps.launches += 1;
        }
        set_sub_batch(p, c.yf(), b0, nb, g2.v_sample);
        p.x_cls = nb * d->cin * p.x_cs;
        int nl = 0;
        e = s3r::launch_conv_wino2(p, g2.ax, wino2_form_of(d, p.Ntotal, form), to_v, c.s, &nl);
        if (e != hipSuccess) return hip_fail(e, "two-axis Winograd conv launch");
        ps.launches += nl;
    }
    return S3R_OK;
}

// transposed, F(2, 2) along D and H inside the parity classes: difference tensors + class kernel
int run_dwino(const ConvCall& c, s3r::ConvParams p, int form, const HeadWork& head) {
    const s3r_conv_desc* d = c.d;
    ProfScope ps(c.s, F_MFMA, d->tag, c.g.flops + head.flops, c.g.bytes + head.bytes);
    wino_prof(ps, c, ALG_WINO, head);
    const WinoNeed need = wino_need(d, form, p.head_w != nullptr);
    int rc = check_scratch(c, need.total, "the Winograd form of this transposed convolution needs");
    if (rc) return rc;
    const int n = d->in_size;
    const bool pre = d->in_layout == S3R_LAYOUT_DIFF;                 // the producer wrote [x | Dh | Dd | Ddh]
    const int64_t x_plain = (int64_t)d->batch * d->cin * ipow(n + 2, 3);
    p.xd_mode = pre || dwino_materialise(d) ? 1 : 0;
    hipError_t e = hipSuccess;
    if (!pre) {
        s3r::AuxScope aux(c.s, 4.0 * (double)x_plain * (p.xd_mode ? 4.0 : 2.0));      // (reads x, writes Dh [, Dd, Ddh])
        e = s3r::launch_wino_diff(c.xf(), c.scratch, (long long)d->batch * d->cin, n + 2, n + 2, n + 2, p.xd_mode, c.s);
    }
    if (e != hipSuccess) return hip_fail(e, "Winograd difference-tensor launch");
    p.xd = pre ? c.xf() + x_plain : c.scratch;
    p.x_bytes = (unsigned)(4 * x_plain);                              // (one tensor: the class kernel steps from Dh to Dd to Ddh by it)
    p.out_mode = d->out_layout == S3R_LAYOUT_DIFF ? 3 : 0;            // ... and this layer's finish pass writes its consumer's
    p.part = c.scratch + need.v;
    p.w = c.wf() + packed_layout(d, c.g).dwino;
    p.Nd = n / 2; p.Nh = n / 2;
    p.Ntotal = p.B * p.Nd * p.Nh * p.Nw;
    p.n_begin = 0; p.n_end = p.Ntotal;
    set_divs(p);
    p.ksplit = 1;
    const s3r::WinoLaunch L = s3r::wino_plan(2, d->cout, wino_kcls(d), p.Ntotal, p.head_w != nullptr, form);
    if (p.out_mode && (L.mode != s3r::WINO_CP || p.head_w))
        return fail(S3R_ERR_INVALID, "a consumer's difference tensors are written from the class-parallel launch form of the transposed Winograd "
                    "layer only (the form of this batch keeps the plain output: s3r_chain_forward plans that itself)");
    int nl = 0;
    e = s3r::launch_deconv_wino(p, L, c.s, &nl);
    if (e != hipSuccess) return hip_fail(e, "Winograd transposed-conv launch");
    ps.launches = (pre ? 0 : 1) + nl;
    ps.algo = 1 + L.mode;
    return S3R_OK;
}

// transposed, three axes: difference tensors (all three materialised) + the class kernel (serial, or class-parallel over the depth
// class with a finish kernel: same bits)
int run_dwino3(const ConvCall& c, s3r::ConvParams p, int form, const HeadWork& head) {
    const s3r_conv_desc* d = c.d;
    ProfScope ps(c.s, F_MFMA, d->tag, c.g.flops + head.flops, c.g.bytes + head.bytes);
    wino_prof(ps, c, ALG_WINO3, head);
    const int n = d->in_size;
    const Dwino3Need nd = dwino3_need(d, form);
    int rc = check_scratch(c, nd.total, "the three-axis Winograd form of this transposed convolution needs");
    if (rc) return rc;
    hipError_t e;
    {
        s3r::AuxScope aux(c.s, 4.0 * 4.0 * (double)d->batch * d->cin * (double)ipow(n + 2, 3));
        e = s3r::launch_wino_diff(c.xf(), c.scratch, (long long)d->batch * d->cin, n + 2, n + 2, n + 2, 1, c.s);
    }
    if (e != hipSuccess) return hip_fail(e, "Winograd difference-tensor launch");
    p.xd = c.scratch;
    p.w = c.wf() + packed_layout(d, c.g).dwino3;
    p.Nd = p.Nh = p.Nw = n / 2;
    p.Ntotal = p.B * p.Nd * p.Nh * p.Nw;
    set_divs(p);
    p.ksplit = 1;
    p.part = nd.split ? c.scratch + nd.diff : nullptr;
    e = s3r::launch_deconv_wino3(p, nd.split, c.s);
    if (e != hipSuccess) return hip_fail(e, "three-axis Winograd transposed-conv launch");
    ps.launches = nd.split ? 3 : 2;
    ps.algo = nd.split ? 6 : 5;
    return S3R_OK;
}

int run_wino(const ConvCall& c, const s3r::ConvParams& p, int alg, int form, const HeadWork& head) {
    if (alg == ALG_WINO2) return run_wino2(c, p, form, head);
    if (alg == ALG_WINO3) return run_dwino3(c, p, form, head);
    return c.d->op == S3R_OP_DECONV ? run_dwino(c, p, form, head) : run_wino1(c, p, form, head);
}

// ---------------------------------------------------------------- the direct kernel: split-K and hand-off rules
int run_direct(const ConvCall& c, s3r::ConvParams p) {
    const s3r_conv_desc* d = c.d;
    Launch L;
    int rc = resolve_launch(d, &p, &L);
    if (rc) return rc;
    if (d->in_layout != S3R_LAYOUT_PLAIN || d->out_layout == S3R_LAYOUT_DIFF || d->out_layout == S3R_LAYOUT_WINO_HW)
        return fail(S3R_ERR_INVALID, "the direct kernel reads a plain input and writes a plain output or (split-K) its consumer's two-axis plane sets");
    if (d->out_layout == S3R_LAYOUT_WINO_3D) {      // the split-K finish pass writes the consumer's plane sets
        if (L.ksplit <= 1 || d->op != S3R_OP_CONV || needs_act_pass(d) || p.act == S3R_ACT_SIGMOID)
            return fail(S3R_ERR_INVALID, "a direct layer writes its consumer's plane sets from its split-K finish pass only (convolution, "
                        "ksplit > 1, no activation pass behind it)");
        p.out_mode = d->out_halo ? 1 : 2;
    }
    if (L.ksplit > 1) {
        if ((rc = check_splitk_scratch(c, L.ksplit, s3r::conv_scratch_elems(p, L.cfg)))) return rc;
        p.part = c.scratch;
    }
    ProfScope ps(c.s, F_MFMA, d->tag, c.g.flops, c.g.bytes);
    ps.launches = 0;
    if ((rc = launch_direct(p, L, c.s, ps, "conv forward launch"))) return rc;
    if (needs_act_pass(d) && (rc = act_pass(c, ps, "conv forward launch"))) ps.launches += 1;      // (counted even when it failed: ADVICE.md)
    return rc;
}

// ---------------------------------------------------------------- every forward convolution: validation, then the path's runner
int conv_forward_impl(ConvCall c) {
    const s3r_conv_desc* d = c.d;
    Route r;
    int rc = geometry(d, &c.g);
    if (rc) return rc;
    if ((rc = route(d, &r))) return rc;
    if ((rc = check_halos(d, r))) return rc;
    if (!c.x || !c.w || !c.y) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (c.x2 && r != R_STEM) return fail(S3R_ERR_INVALID, "only the stem convolution takes a second input tensor");
    if (c.x_u8 && r != R_STEM) return fail(S3R_ERR_INVALID, "only the stem convolution reads 8-bit renders");
    if (r == R_STEM && (rc = check_stem_input(d, c.x, c.x2, c.nsplit))) return rc;
    if (d->dtype == S3R_BF16) {
        if (r != R_STEM && misaligned16(c.x)) return bf16_align_fail("the bf16 input of an S3R_BF16 layer", c.x);
        if (r != R_HEAD && misaligned16(c.y)) return bf16_align_fail("the bf16 output of an S3R_BF16 layer", c.y);
        if (c.scratch && misaligned16(c.scratch)) return bf16_align_fail("the scratch of an S3R_BF16 layer", c.scratch);
        if (c.g.x_elems * 2 >= ((int64_t)1 << 31) || c.g.y_elems * 2 >= ((int64_t)1 << 31))
            return fail(S3R_ERR_INVALID, "bf16 path: tensors must be < 2 GiB per call: split the batch");
        if (r == R_LINEAR) return fail(S3R_ERR_INVALID, "layer not available on the bf16 path");
    }
    switch (r) {
        case R_STEM: return run_stem(c);
        case R_HEAD: return run_head(c);
        case R_LINEAR: return run_linear(c);
        case R_MFMA: break;
    }
    if (d->dtype == S3R_BF16) return run_mfma_bf16(c);
    int alg, form;
    if ((rc = resolve_algo(d, &alg, &form))) return rc;
    if (staged_layer(d)) return run_staged(c);
    const s3r::ConvParams p = bind(c, make_params(d, c.g));
    return alg == ALG_DIRECT ? run_direct(c, p) : run_wino(c, p, alg, form, kNoHead);
}

// MFMA conv with the following 1x1 single-channel head folded into its epilogue (plan_chain decides)
int conv_head_fused(const s3r_conv_desc* d, const Geo& g, const s3r_conv_desc* hd, const Geo& hg, const float* x,
                    const s3r_layer& L, const s3r_layer& H, float* out, float* scratch, int64_t scratch_elems, hipStream_t s) {
    const ConvCall c = {d, g, x, nullptr, 0, 0, L.packed_w, L.scale, L.shift, out, scratch, scratch_elems, s};
    s3r::ConvParams p = bind(c, make_params(d, g));
    // y_* now describe the head's (B, 1, n[, n], n) output
    const bool is3 = hd->ndim == 3;
    p.y_hs = hg.out_p; p.y_ds = is3 ? hg.out_p * hg.out_p : 0; p.y_cs = (int)ipow(hg.out_p, hg.nd);
    p.y_bs = p.y_cs;
    p.y_org = hd->out_halo * (p.y_ds + p.y_hs + 1);
    p.y_bytes = (unsigned)(hg.y_elems * 4);
    p.head_w = static_cast<const float*>(H.packed_w); p.head_scale = H.scale; p.head_shift = H.shift; p.head_act = hd->act;
    const HeadWork head = {hg.flops, 4.0 * d->batch * (double)hg.out_sp - 4.0 * d->batch * d->cout * (double)g.out_sp};
    int alg, form;
    int rc = resolve_algo(d, &alg, &form);
    if (rc) return rc;
    if (alg != ALG_DIRECT) {
        if (!(alg == ALG_WINO3 || (alg == ALG_WINO && d->op == S3R_OP_DECONV)) || d->cout > 64)
            return fail(S3R_ERR_INVALID, "the fused head rides on the transposed Winograd kernel with <= 64 couts only");
        return run_wino(c, p, alg, form, head);
    }
    Launch Ln;
    if ((rc = resolve_launch(d, &p, &Ln))) return rc;
    if (!(Ln.cfg == 1 || Ln.cfg == 2 || Ln.cfg == 7) || (Ln.cfg == 2 && d->cout > 32)) {
        // the heuristic's tile splits the couts over waves: take the widest one-wave-tall tile that fills the chip
        int bm, bn;
        s3r::conv_tile_dims(1, &bm, &bn);
        const long wg1 = (long)((p.Ntotal + bn - 1) / bn) * (p.transposed ? 8 : 1);
        Ln.cfg = d->cout <= 32 ? 2 : (wg1 >= 2000 ? 1 : 7);
    }
    ProfScope ps(s, F_MFMA, d->tag, g.flops + head.flops, g.bytes + head.bytes);
    ps.launches = 0;
    return launch_direct(p, Ln, s, ps, "fused conv+head launch");
}

// the same on the bf16 channels-last path: the conv's 64-cout tile is the whole channel axis of its positions
int conv_head_fused_h(const s3r_conv_desc* d, const Geo& g, const s3r_conv_desc* hd, const Geo& hg, const void* x,
                      const s3r_layer& L, const s3r_layer& H, float* out, hipStream_t s) {
    s3r::ConvParamsH p = make_params_h(d, g);
    p.x = x; p.w = L.packed_w; p.scale = L.scale; p.shift = L.shift; p.y = out;
    const bool is3 = hd->ndim == 3;
    p.y_ws = 1; p.y_hs = hg.out_p; p.y_ds = is3 ? hg.out_p * hg.out_p : 0; p.y_bs = (int)ipow(hg.out_p, hg.nd);
    p.y_org = hd->out_halo * (p.y_ds + p.y_hs + 1);
    p.head_w = static_cast<const float*>(H.packed_w); p.head_scale = H.scale; p.head_shift = H.shift; p.head_act = hd->act;
    LaunchH Ln;
    int rc = resolve_launch_h(d, &p, &Ln);
    if (rc) return rc;
    ProfScope ps(s, F_MFMA, d->tag, g.flops + hg.flops, g.bytes - 2.0 * d->batch * d->cout * (double)g.out_sp +
                 4.0 * d->batch * (double)hg.out_sp);
    hipError_t e = s3r::launch_conv_bf16(p, Ln.tm, s);
    if (e != hipSuccess) return hip_fail(e, "fused conv+head launch (bf16)");
    return S3R_OK;
}

int chain_forward_impl(const s3r_layer* layers, int n_layers, const void* x, const void* x2, int nsplit, int x_u8, void* y,
                       float* ws, int64_t ws_elems, int ws_fresh, void* stream) {
    Plan pl;
    int rc = plan_chain(layers, n_layers, &pl);
    if (rc) return rc;
    if (!x || !y) return fail(S3R_ERR_INVALID, "null tensor pointer");
    {   // bf16 hand-off points and the workspace that holds bf16 intermediates (the first layer's renders are checked below)
        const int last = n_layers - 1;
        bool any_bf16 = false;
        for (int i = 0; i < n_layers; ++i) any_bf16 = any_bf16 || pl.d[i].dtype == S3R_BF16;
        if (pl.d[0].dtype == S3R_BF16 && pl.r[0] != R_STEM && misaligned16(x)) return bf16_align_fail("the bf16 input of an S3R_BF16 chain", x);
        if (pl.d[last].dtype == S3R_BF16 && pl.r[last] != R_HEAD && misaligned16(y))
            return bf16_align_fail("the bf16 output of an S3R_BF16 chain", y);
        if (any_bf16 && pl.total > 0 && ws && misaligned16(ws)) return bf16_align_fail("the workspace of a chain with S3R_BF16 layers", ws);
    }
    if (pl.total > 0 && (!ws || ws_elems < pl.total))
        return fail(S3R_ERR_WORKSPACE, "chain needs a workspace of %lld floats, got %lld", (long long)pl.total,
                    (long long)ws_elems);
    hipStream_t s = (hipStream_t)stream;
    if (ws_fresh && pl.total > 0) {   // zero halos (and everything else) once; later calls write interiors only
        hipError_t e = s3r::launch_zero_fill(ws, (long long)pl.total, s);
        if (e != hipSuccess) return hip_fail(e, "workspace zero fill");
    }
    const void* cur = x;
    if ((x2 || x_u8) && (pl.pad_input || pl.r[0] != R_STEM))
        return fail(S3R_ERR_INVALID, "a second input tensor / 8-bit renders need a chain that starts with the stem convolution");
    // checked HERE: every entry that can reach a stem (s3r_encoder_forward[_u8], s3r_chain_forward over a tower prefix) shares it
    if (pl.r[0] == R_STEM && (rc = check_stem_input(&pl.d[0], x, x2, nsplit))) return rc;
    if (pl.pad_input) {
        const s3r_conv_desc& d0 = pl.d[0];
        const int hl = d0.in_halo, is3 = d0.ndim == 3;
        ProfScope ps(s, F_PAD, d0.tag, 0.0, 8.0 * d0.batch * d0.cin * (double)pl.g[0].in_sp);
        hipError_t e;
        if (d0.dtype == S3R_BF16) {
            // channels-last bf16 (B, [D,] H, W, C): rows of W*C bf16 = W*C/2 floats, planes = samples
            const int wc = d0.in_size * d0.cin / 2, hwc = hl * d0.cin / 2;
            e = s3r::launch_pad_copy(static_cast<const float*>(x), ws + pl.pad_off, d0.batch, is3 ? d0.in_size : 1,
                                     d0.in_size, wc, is3 ? hl : 0, hl, hwc, s);
        } else {
            e = s3r::launch_pad_copy(static_cast<const float*>(x), ws + pl.pad_off, (int64_t)d0.batch * d0.cin,
                                     is3 ? d0.in_size : 1, d0.in_size, d0.in_size, is3 ? hl : 0, hl, hl, s);
        }
        if (e != hipSuccess) return hip_fail(e, "pad copy launch");
        cur = ws + pl.pad_off;
    }
    float* const scratch = pl.scratch_elems ? ws + pl.scratch_off : nullptr;      // split-K slabs / Winograd operands, shared by the layers
    for (int i = 0; i < n_layers; ++i) {
        const s3r_layer& L = layers[i];
        if (pl.fuse_head[i]) {
            const s3r_layer& H = layers[i + 1];
            void* out = (i + 1 == n_layers - 1) ? y : static_cast<void*>(ws + pl.off[i + 1]);
            if (pl.d[i].dtype == S3R_BF16)
                rc = conv_head_fused_h(&pl.d[i], pl.g[i], &pl.d[i + 1], pl.g[i + 1], cur, L, H, static_cast<float*>(out), s);
            else
                rc = conv_head_fused(&pl.d[i], pl.g[i], &pl.d[i + 1], pl.g[i + 1], static_cast<const float*>(cur), L, H,
                                     static_cast<float*>(out), scratch, pl.scratch_elems, s);
            if (rc) return rc;
            cur = out;
            ++i;
            continue;
        }
        void* out = (i == n_layers - 1) ? y : static_cast<void*>(ws + pl.off[i]);
        if (i == 0 && pl.stem_wino) {
            const s3r_conv_desc& d0 = pl.d[0];
            const Geo& g0 = pl.g[0];
            if (!L.packed_w || !L.scale || !L.shift) return fail(S3R_ERR_INVALID, "stem needs packed weights, scale and shift");
            // bytes: the renders in (1 byte a sample when 8-bit), layer 1's six plane sets out
            ProfScope ps(s, F_STEM, d0.tag, g0.flops, (x_u8 ? 1.0 : 4.0) * d0.batch * d0.cin * (double)g0.in_sp + 4.0 * (double)pl.g[1].x_elems);
            hipError_t e = s3r::launch_stem_wino(cur, x2, x_u8, nsplit, static_cast<const float*>(L.packed_w), L.scale, L.shift,
                                                 static_cast<float*>(out), d0.batch, g0.in, g0.in, g0.out, g0.out, s);
            if (e != hipSuccess) return hip_fail(e, "stem (Winograd layout) launch");
            cur = out;
            continue;
        }
        rc = conv_forward_impl({&pl.d[i], Geo(), cur, i == 0 ? x2 : nullptr, nsplit, i == 0 ? x_u8 : 0, L.packed_w, L.scale, L.shift, out,
                                scratch, pl.scratch_elems, s});
        if (rc) return rc;
        cur = out;
    }
    return S3R_OK;
}

int encoder_forward(const s3r_layer* layers, int n_layers, const void* images_left, const void* images_right, int u8,
                    void* features, float* ws, int64_t ws_elems, int ws_fresh, void* stream) {
    if (!layers || n_layers <= 0) return fail(S3R_ERR_INVALID, "empty encoder");
    const s3r_conv_desc& f = layers[0].desc;
    if (f.op != S3R_OP_CONV || f.ndim != 2 || f.cin != 3)
        return fail(S3R_ERR_INVALID, "encoder must start with a 2D convolution over 3-channel renders");
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].desc.op != S3R_OP_CONV || layers[i].desc.ndim != 2)
            return fail(S3R_ERR_INVALID, "encoder layer %d is not a 2D convolution", i);
    if (images_right && (f.batch < 2 || (f.batch & 1)))
        return fail(S3R_ERR_INVALID, "a (left, right) pair of tensors needs an even image count N = 2B (got %d)", f.batch);
    return chain_forward_impl(layers, n_layers, images_left, images_right, f.batch / 2, u8, features, ws, ws_elems, ws_fresh,
                              stream);
}

}  // namespace

extern "C" {

int s3r_abi_version(void) { return S3R_ABI_VERSION; }

const char* s3r_last_error(void) { return last_error(); }

int s3r_conv_pack_weights(const s3r_conv_desc* d, const float* w, void* packedv, void* stream) {
    float* packed = static_cast<float*>(packedv);
    Geo g; Route r;
    int rc = geometry(d, &g);
    if (rc) return rc;
    if ((rc = route(d, &r))) return rc;
    if (!w || !packed) return fail(S3R_ERR_INVALID, "null weight pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_PACK, d->tag, 0.0, 8.0 * g.w_elems);
    hipError_t e = hipSuccess;
    switch (r) {
        case R_STEM: e = s3r::launch_pack_stem(w, packed, s); break;
        case R_HEAD: e = hipMemcpyAsync(packed, w, sizeof(float) * d->cin, hipMemcpyDeviceToDevice, s); break;
        case R_LINEAR: e = hipMemcpyAsync(packed, w, sizeof(float) * g.w_elems, hipMemcpyDeviceToDevice, s); break;
        case R_MFMA:
            if (d->dtype == S3R_BF16)
                e = s3r::launch_pack_bf16(w, packed, d->cin, d->cout, cout_pad_h(d->cout),
                                          d->op == S3R_OP_DECONV ? 8 : (int)ipow(d->k, g.nd), d->op == S3R_OP_DECONV, s);
            else if (tshuf_layer(d)) {      // w[Cin][Cout][k^nd] IS [Cin][cout x taps]: pad the rows to 16 and the columns to the tile
                const int rows = d->cout * (int)ipow(d->stride, g.nd);
                e = s3r::launch_pack_general(w, packed, d->cin, staged_geo(d).cin_pad, rows, cout_pad(rows), 1, 1, s);
            } else if (tclass_layer(d)) {
                for (int cls = 0; cls < (int)ipow(d->stride, g.nd) && e == hipSuccess; ++cls) {
                    const int rw = cls % d->stride, rh = (cls / d->stride) % d->stride, rd = g.nd == 3 ? cls / (d->stride * d->stride) : 0;
                    s3r::ConvParams q; int64_t w_off; double macs;
                    (void)make_params_tclass(d, g, rd, rh, rw, &q, &w_off, &macs);      // (the slab is packed whether or not this size uses it)
                    e = s3r::launch_pack_tclass(w, packed + w_off, d->cin, staged_geo(d).cin_pad, d->cout, cout_pad(d->cout), g.nd, d->k,
                                                d->stride, rd, rh, rw, s);
                }
            } else if (im2col_layer(d)) {      // w[Cout][Cin][k^nd] IS [Cout][cin x taps]: the K rows of the unfolded GEMM
                e = s3r::launch_pack_general(w, packed, d->cin * (int)ipow(d->k, g.nd), staged_geo(d).cin_pad, d->cout, cout_pad(d->cout), 1, 0, s);
            } else if (staged_layer(d)) {
                e = s3r::launch_pack_general(w, packed, d->cin, staged_geo(d).cin_pad, d->cout, cout_pad(d->cout), (int)ipow(d->k, g.nd),
                                             d->op == S3R_OP_DECONV, s);
            } else {      // the direct slab, then the slab of every Winograd form the layer has (packed_layout)
                const PackedLayout at = packed_layout(d, g);
                const int cp = cout_pad(d->cout);
                e = s3r::launch_pack_conv(w, packed + at.direct, d->cin, d->cout, cp, d->op == S3R_OP_DECONV ? 8 : (int)ipow(d->k, g.nd),
                                          d->op == S3R_OP_DECONV, s);
                if (e == hipSuccess && at.wino >= 0)
                    e = s3r::launch_pack_wino(w, packed + at.wino, d->cin, d->cout, cp, g.nd == 3 ? 3 : 1, 3, wino_r(d), s);
                if (e == hipSuccess && at.dwino >= 0) e = s3r::launch_pack_wino_deconv(w, packed + at.dwino, d->cin, d->cout, cp, s);
                if (e == hipSuccess && at.dwino3 >= 0) e = s3r::launch_pack_dwino3(w, packed + at.dwino3, d->cin, d->cout, s);
                if (e == hipSuccess && at.wino2 >= 0) e = s3r::launch_pack_wino2(w, packed + at.wino2, wino2_ax(d), d->cin, d->cout, cp, s);
            }
            break;
    }
    if (e != hipSuccess) return hip_fail(e, "pack weights");
    return S3R_OK;
}

int s3r_conv_forward(const s3r_conv_desc* d, const void* xv, const void* packed_wv, const float* scale,
                     const float* shift, void* yv, float* scratch, int64_t scratch_elems, void* stream) {
    return conv_forward_impl({d, Geo(), xv, nullptr, 0, 0, packed_wv, scale, shift, yv, scratch, scratch_elems, (hipStream_t)stream});
}

int s3r_chain_forward(const s3r_layer* layers, int n_layers, const void* x, void* y, float* ws, int64_t ws_elems,
                      int ws_fresh, void* stream) {
    return chain_forward_impl(layers, n_layers, x, nullptr, 0, 0, y, ws, ws_elems, ws_fresh, stream);
}

int s3r_encoder_forward(const s3r_layer* layers, int n_layers, const float* images_left, const float* images_right,
                        void* features, float* ws, int64_t ws_elems, int ws_fresh, void* stream) {
    return encoder_forward(layers, n_layers, images_left, images_right, 0, features, ws, ws_elems, ws_fresh, stream);
}

int s3r_encoder_forward_u8(const s3r_layer* layers, int n_layers, const uint8_t* images_left, const uint8_t* images_right,
                           void* features, float* ws, int64_t ws_elems, int ws_fresh, void* stream) {
    return encoder_forward(layers, n_layers, images_left, images_right, 1, features, ws, ws_elems, ws_fresh, stream);
}

int s3r_channels_last_to_f32(const void* x, float* y, int batch, int channels, int64_t positions, void* stream) {
    if (!x || !y) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (misaligned16(x)) return bf16_align_fail("the bf16 channels-last tensor", x);
    if (batch <= 0 || channels <= 0 || positions <= 0) return fail(S3R_ERR_INVALID, "dims must be positive");
    if (batch > 65535 || (int64_t)channels * positions >= kMaxElems)
        return fail(S3R_ERR_INVALID, "tensor too large for one call: split the batch");
    hipStream_t s = (hipStream_t)stream;
    const double n = (double)batch * channels * (double)positions;
    ProfScope ps(s, F_PAD, 1, 0.0, 6.0 * n);
    hipError_t e = s3r::launch_cl_bf16_to_f32(x, y, batch, positions, channels, s);
    if (e != hipSuccess) return hip_fail(e, "channels-last to fp32 launch");
    return S3R_OK;
}

int s3r_decoder_forward(const s3r_layer* layers, int n_layers, const void* volume, float* occupancy, float* ws,
                        int64_t ws_elems, int ws_fresh, void* stream) {
    if (!layers || n_layers <= 0) return fail(S3R_ERR_INVALID, "empty decoder");
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].desc.op == S3R_OP_LINEAR || layers[i].desc.ndim != 3)
            return fail(S3R_ERR_INVALID, "decoder layer %d is not a 3D (transposed) convolution", i);
    return s3r_chain_forward(layers, n_layers, volume, occupancy, ws, ws_elems, ws_fresh, stream);
}

int s3r_cost_volume_forward(const float* fl, const float* fr, float* vol, int batch, int channels, int max_disp,
                            int height, int width, int out_halo, void* stream) {
    if (!fl || !fr || !vol) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || channels <= 0 || max_disp <= 0 || height <= 0 || width <= 0)
        return fail(S3R_ERR_INVALID, "cost volume dims must be positive");
    const int64_t hw = (int64_t)height * width;
    if (2 * hw * 4 > 64 * 1024) return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the LDS staging", height, width);
    if (out_halo < 0 || out_halo > 8) return fail(S3R_ERR_INVALID, "halo must be in [0, 8]");
    const int64_t out = (int64_t)batch * 2 * channels * max_disp * hw;
    const int64_t out_p = (int64_t)batch * 2 * channels * (max_disp + 2 * out_halo) * (height + 2 * out_halo) *
                          (width + 2 * out_halo);
    if (out_p >= kMaxElems) return fail(S3R_ERR_INVALID, "cost volume too large for one call: split the batch");
    hipStream_t s = (hipStream_t)stream;
    const double bytes = 4.0 * (2.0 * batch * channels * hw + (double)out);
    ProfScope ps(s, F_COSTVOL, 0, (double)out, bytes);
    hipError_t e = s3r::launch_cost_volume(fl, fr, vol, batch, channels, max_disp, height, width, out_halo, s);
    if (e != hipSuccess) return hip_fail(e, "cost volume launch");
    return S3R_OK;
}

int s3r_cost_volume_forward_wino(const float* fl, const float* fr, float* planes, int batch, int channels, int max_disp,
                                 int height, int width, void* stream) {
    if (!fl || !fr || !planes) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || channels <= 0 || max_disp <= 0 || height < 4 || width <= 0 || (height & 3))
        return fail(S3R_ERR_INVALID, "bad cost-volume shape for the Winograd layout (height a multiple of 4: F(4,3) groups)");
    if (max_disp > width) return fail(S3R_ERR_INVALID, "max_disp %d exceeds the feature width %d", max_disp, width);
    if ((size_t)2 * height * width * sizeof(float) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the kernel's 64 KiB of LDS", height, width);
    const int64_t elems = 6 * (int64_t)batch * 2 * channels * (max_disp + 2) * (height / 4) * (width + 2);
    if (elems * 4 >= ((int64_t)1 << 31)) return fail(S3R_ERR_INVALID, "Winograd planes of %lld floats exceed 2 GiB: split the batch", (long long)elems);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, 2.0 * batch * channels * (double)max_disp * height * width,
                 4.0 * batch * channels * (2.0 * height * width) + 4.0 * (double)elems);
    hipError_t e = s3r::launch_cost_volume_wino(fl, fr, planes, batch, channels, max_disp, height, width, 4, s);
    if (e != hipSuccess) return hip_fail(e, "cost volume (Winograd layout) launch");
    return S3R_OK;
}

int s3r_cost_volume_forward_wino2(const float* fl, const float* fr, float* planes, int batch, int channels, int max_disp,
                                  int height, int width, void* stream) {
    if (!fl || !fr || !planes) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || channels <= 0 || max_disp < 4 || height < 4 || width <= 0 || (height & 3) || (max_disp & 3))
        return fail(S3R_ERR_INVALID, "bad cost-volume shape for the two-axis Winograd layout (height and max_disp multiples of 4: F(4,3) groups)");
    if (max_disp > width) return fail(S3R_ERR_INVALID, "max_disp %d exceeds the feature width %d", max_disp, width);
    if ((size_t)2 * height * width * sizeof(float) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the kernel's 64 KiB of LDS", height, width);
    const int64_t elems = 36 * (int64_t)batch * 2 * channels * (max_disp / 4) * (height / 4) * (width + 2);
    if (elems * 4 >= ((int64_t)1 << 31)) return fail(S3R_ERR_INVALID, "two-axis Winograd planes of %lld floats exceed 2 GiB: split the batch", (long long)elems);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, 2.0 * batch * channels * (double)max_disp * height * width,
                 4.0 * batch * channels * (2.0 * height * width) + 4.0 * (double)elems);
    hipError_t e = s3r::launch_cost_volume_wino2(fl, fr, planes, batch, channels, max_disp, height, width, s);
    if (e != hipSuccess) return hip_fail(e, "cost volume (two-axis Winograd layout) launch");
    return S3R_OK;
}

int s3r_cost_volume_forward_bf16(const void* fl, const void* fr, void* vol, int batch, int channels, int max_disp,
                                 int height, int width, int out_halo, void* stream) {
    if (!fl || !fr || !vol) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (misaligned16(fl)) return bf16_align_fail("the left bf16 features", fl);
    if (misaligned16(fr)) return bf16_align_fail("the right bf16 features", fr);
    if (misaligned16(vol)) return bf16_align_fail("the bf16 cost volume", vol);
    if (batch <= 0 || channels <= 0 || max_disp <= 0 || height <= 0 || width <= 0)
        return fail(S3R_ERR_INVALID, "cost volume dims must be positive");
    if (channels % 8 != 0) return fail(S3R_ERR_INVALID, "bf16 cost volume needs channels %% 8 == 0");
    if (out_halo < 0 || out_halo > 8) return fail(S3R_ERR_INVALID, "halo must be in [0, 8]");
    const int64_t hw = (int64_t)height * width;
    const int64_t out = (int64_t)batch * 2 * channels * max_disp * hw;
    const int64_t out_p = (int64_t)batch * 2 * channels * (max_disp + 2 * out_halo) * (height + 2 * out_halo) *
                          (width + 2 * out_halo);
    if (out_p >= kMaxElems) return fail(S3R_ERR_INVALID, "cost volume too large for one call: split the batch");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, (double)out, 2.0 * (2.0 * batch * channels * hw + (double)out));
    hipError_t e = s3r::launch_cost_volume_bf16(fl, fr, vol, batch, channels, max_disp, height, width, out_halo, s);
    if (e != hipSuccess) return hip_fail(e, "cost volume launch (bf16)");
    return S3R_OK;
}

int s3r_cost_volume_backward(const float* grad_volume, float* grad_left, float* grad_right, int batch, int channels, int max_disp,
                             int height, int width, void* hip_stream) {
    if (!grad_left && !grad_right)
        return fail(S3R_ERR_INVALID, "cost volume backward: grad_left and grad_right are both NULL (either may be: it is not computed)");
    if (batch < 0 || channels <= 0 || max_disp <= 0 || height <= 0 || width <= 0)
        return fail(S3R_ERR_INVALID, "cost volume backward dims must be positive (batch >= 0)");
    const int64_t hw = (int64_t)height * width;
    if (2 * hw * 4 > 64 * 1024)      // the forward's domain: a gradient exists for the volumes the forward can write
        return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the forward's LDS staging", height, width);
    const int64_t vol = (int64_t)batch * 2 * channels * max_disp * hw;
    if (vol >= kMaxElems) return fail(S3R_ERR_INVALID, "cost volume gradient too large for one call: split the batch");
    if (batch == 0) return S3R_OK;
    if (!grad_volume) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const double dn = max_disp < width ? max_disp : width;
    const double terms = dn * (dn + 1.0) / 2.0 + (width - dn) * dn;      // sum over w of n_L(w) = sum over w of n_R(w)
    const double sides = (grad_left ? 1.0 : 0.0) + (grad_right ? 1.0 : 0.0);
    const double rows = (double)batch * channels * height;
    ProfScope ps(s, F_COSTVOL, 1, 2.0 * sides * rows * terms, 4.0 * ((double)vol + sides * rows * width));
    hipError_t e = s3r::launch_cost_volume_backward(grad_volume, grad_left, grad_right, batch, channels, max_disp, height, width, s);
    if (e != hipSuccess) return hip_fail(e, "cost volume backward launch");
    return S3R_OK;
}

int64_t s3r_linear_scratch_elems(int batch, int cin, int cout) {
    if (batch <= 0 || cin <= 0 || cout <= 0) return fail(S3R_ERR_INVALID, "linear dims must be positive");
    return s3r::linear_scratch_elems(batch, cin, cout);
}

int s3r_linear_forward(const float* x, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                       int act, float* scratch, int64_t scratch_elems, void* stream) {
    if (!x || !w || !y) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || cin <= 0 || cout <= 0) return fail(S3R_ERR_INVALID, "linear dims must be positive");
    if (act < S3R_ACT_NONE || act > S3R_ACT_SIGMOID)
        return fail(S3R_ERR_INVALID, "s3r_linear_forward takes none / relu / sigmoid (act %d): LeakyReLU / ELU / Tanh carry a parameter — "
                    "run the layer as an S3R_OP_LINEAR descriptor through s3r_conv_forward / s3r_chain_forward", act);
    if (!scratch || scratch_elems < s3r::linear_scratch_elems(batch, cin, cout))
        return fail(S3R_ERR_WORKSPACE, "linear needs %lld floats of scratch (s3r_linear_scratch_elems)",
                    (long long)s3r::linear_scratch_elems(batch, cin, cout));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_LINEAR, 0, 2.0 * batch * (double)cin * cout, 4.0 * ((double)cin * cout + (double)batch * (cin + cout)));
    hipError_t e = s3r::launch_linear(x, w, nullptr, bias, y, batch, cin, cout, act, scratch, s);
    if (e != hipSuccess) return hip_fail(e, "linear launch");
    return S3R_OK;
}

// every tensor of a linear-backward call within the header's limits (< 2^31 elements, < 4 GiB)
static bool linbwd_too_large(int batch, int cin, int cout) {
    const int64_t a = (int64_t)batch * cin, b = (int64_t)batch * cout, c = (int64_t)cin * cout;
    const int64_t m = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return m >= kMaxElems || 4 * m >= kMaxBytes;
}

int64_t s3r_linear_backward_scratch_elems(int batch, int cin, int cout) {
    if (batch <= 0 || cin <= 0 || cout <= 0) return fail(S3R_ERR_INVALID, "linear dims must be positive");
    if (linbwd_too_large(batch, cin, cout)) return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the batch");
    return s3r::linear_backward_scratch_elems(batch, cin, cout);
}

int s3r_linear_backward(const float* x, const float* w, const float* y, const float* grad_y, float* grad_x, float* grad_w,
                        float* grad_bias, int batch, int cin, int cout, int act, float* scratch, int64_t scratch_elems, void* stream) {
    if (!grad_x && !grad_w && !grad_bias)
        return fail(S3R_ERR_INVALID, "linear backward: grad_x, grad_w and grad_bias are all NULL (each may be: it is not computed)");
    if (act < S3R_ACT_NONE || act > S3R_ACT_SIGMOID)
        return fail(S3R_ERR_INVALID, "s3r_linear_backward takes none / relu / sigmoid (act %d)", act);
    if (!grad_y || (grad_w && !x) || (grad_x && !w)) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (act != S3R_ACT_NONE && !y) return fail(S3R_ERR_INVALID, "linear backward: y is NULL (it may be only when act is none)");
    if (batch <= 0 || cin <= 0 || cout <= 0) return fail(S3R_ERR_INVALID, "linear dims must be positive");
    if (linbwd_too_large(batch, cin, cout)) return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the batch");
    const int64_t need = s3r::linear_backward_scratch_elems(batch, cin, cout);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "linear backward needs %lld floats of scratch (s3r_linear_backward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)stream;
    const double B = batch, I = cin, O = cout;
    const double flops = 2.0 * B * I * O * ((grad_w ? 1.0 : 0.0) + (grad_x ? 1.0 : 0.0));
    const double elems = B * O * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (grad_w ? B * I + I * O : 0.0) + (grad_x ? I * O + B * I : 0.0) +
                         (grad_bias ? O : 0.0);
    ProfScope ps(s, F_LINEAR, 1, flops, 4.0 * elems);
    hipError_t e = s3r::launch_linear_backward(x, w, y, grad_y, grad_x, grad_w, grad_bias, batch, cin, cout, act, scratch, s, &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "linear backward launch");
    return S3R_OK;
}

int s3r_chamfer_forward(const float* p, const float* q, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                        int batch, int n, int m, void* stream) {
    if (!p || !q || !dist1 || !dist2 || !idx1 || !idx2) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || n <= 0 || m <= 0) return fail(S3R_ERR_INVALID, "chamfer needs non-empty clouds (batch=%d n=%d m=%d)", batch, n, m);
    if (batch > 65535) return fail(S3R_ERR_INVALID, "batch > 65535: split the call");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_CHAMFER, 0, 2.0 * 8.0 * batch * (double)n * m, 4.0 * batch * (5.0 * n + 5.0 * m));
    hipError_t e = s3r::launch_chamfer(p, q, dist1, dist2, idx1, idx2, batch, n, m, s);
    if (e != hipSuccess) return hip_fail(e, "chamfer launch");
    return S3R_OK;
}

int s3r_chamfer_backward(const float* p, const float* q, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                         const float* grad_dist2, float* grad_p, float* grad_q, int batch, int n, int m, void* stream) {
    if (!p || !q || !idx1 || !idx2) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (!grad_dist1 && !grad_dist2) return fail(S3R_ERR_INVALID, "chamfer backward: grad_dist1 and grad_dist2 are both NULL (one may be: it means zeros)");
    if (!grad_p && !grad_q) return fail(S3R_ERR_INVALID, "chamfer backward: grad_p and grad_q are both NULL (one may be: it is not computed)");
    if (batch <= 0 || n <= 0 || m <= 0) return fail(S3R_ERR_INVALID, "chamfer needs non-empty clouds (batch=%d n=%d m=%d)", batch, n, m);
    if (batch > 65535) return fail(S3R_ERR_INVALID, "batch > 65535: split the call");
    if (3 * (int64_t)batch * (n > m ? n : m) >= kMaxElems) return fail(S3R_ERR_INVALID, "tensor of 2^31 elements or more: split the batch");
    hipStream_t s = (hipStream_t)stream;
    // per computed direction: 7 per target (one doubling, 3 differences, 3 products: the own term) + 10 per source (one doubling, 3
    // differences, 3 products, 3 adds: every source scatters one term); the index compares of the scan are not counted
    const double B = batch, N = n, M = m;
    const double flops = B * ((grad_p ? 7.0 * N + 10.0 * M : 0.0) + (grad_q ? 7.0 * M + 10.0 * N : 0.0));
    const double elems = 3.0 * (N + M) + (N + M) + (grad_dist1 ? N : 0.0) + (grad_dist2 ? M : 0.0) + (grad_p ? 3.0 * N : 0.0) +
                         (grad_q ? 3.0 * M : 0.0);
    ProfScope ps(s, F_CHAMFER, 1, flops, 4.0 * B * elems);
    hipError_t e = s3r::launch_chamfer_backward(p, q, idx1, idx2, grad_dist1, grad_dist2, grad_p, grad_q, batch, n, m, s);
    if (e != hipSuccess) return hip_fail(e, "chamfer backward launch");
    return S3R_OK;
}

int s3r_voxel_iou(const float* pred, const float* gt, float threshold, float* iou, int batch, int64_t voxels,
                  void* stream) {
    if (!pred || !gt || !iou) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || voxels <= 0) return fail(S3R_ERR_INVALID, "iou dims must be positive");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_IOU, 0, 0.0, 8.0 * batch * (double)voxels);
    hipError_t e = s3r::launch_iou(pred, gt, threshold, iou, batch, voxels, s);
    if (e != hipSuccess) return hip_fail(e, "iou launch");
    return S3R_OK;
}

// (B V) of a BCE call within the header's limits (< 2^31 elements, < 4 GiB)
static int bce_dims(int batch, int64_t voxels) {
    if (batch < 0 || voxels <= 0) return fail(S3R_ERR_INVALID, "voxel BCE dims: batch >= 0 and voxels > 0 (batch %d, voxels %lld)", batch, (long long)voxels);
    if (voxels >= kMaxElems || (int64_t)batch * voxels >= kMaxElems || 4 * (int64_t)batch * voxels >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the batch");
    return S3R_OK;
}

int s3r_voxel_bce_forward(const float* pred, const float* target, float* loss_sum, float* loss_elem, int batch, int64_t voxels,
                          void* stream) {
    if (!loss_sum && !loss_elem)
        return fail(S3R_ERR_INVALID, "voxel BCE: loss_sum and loss_elem are both NULL (one may be: it is not written)");
    int rc = bce_dims(batch, voxels);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !target) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)stream;
    const double n = (double)batch * (double)voxels;
    ProfScope ps(s, F_IOU, 1, 0.0, 4.0 * (n * (loss_elem ? 3.0 : 2.0) + (loss_sum ? batch : 0)));
    hipError_t e = s3r::launch_voxel_bce(pred, target, loss_sum, loss_elem, batch, voxels, s);
    if (e != hipSuccess) return hip_fail(e, "voxel BCE launch");
    return S3R_OK;
}

int s3r_voxel_bce_backward(const float* pred, const float* target, const float* grad_scale, float* grad_pred, int batch,
                           int64_t voxels, void* stream) {
    int rc = bce_dims(batch, voxels);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !target || !grad_scale || !grad_pred) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_IOU, 2, 0.0, 4.0 * (3.0 * batch * (double)voxels + batch));
    hipError_t e = s3r::launch_voxel_bce_backward(pred, target, grad_scale, grad_pred, batch, voxels, s);
    if (e != hipSuccess) return hip_fail(e, "voxel BCE backward launch");
    return S3R_OK;
}

// x / grad_x of a head-backward call within the header's limits (< 2^31 elements, < 4 GiB); they are its largest tensors
static int headbwd_dims(int batch, int channels, int64_t voxels) {
    if (batch < 0 || channels <= 0 || voxels <= 0)
        return fail(S3R_ERR_INVALID, "head backward dims: batch >= 0, channels > 0 and voxels > 0 (batch %d, channels %d, voxels %lld)", batch,
                    channels, (long long)voxels);
    if (voxels >= kMaxElems || (int64_t)channels * voxels >= kMaxElems || (int64_t)batch * channels * voxels >= kMaxElems ||
        4 * (int64_t)batch * channels * voxels >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the batch");
    return S3R_OK;
}

int64_t s3r_head_backward_scratch_elems(int batch, int channels, int64_t voxels) {
    int rc = headbwd_dims(batch, channels, voxels);
    if (rc) return rc;
    return s3r::head_backward_scratch_elems(batch, channels, voxels);
}

int s3r_head_backward(const float* x, const float* w, const float* scale, const float* y, const float* grad_y, float* grad_x,
                      float* grad_w, float* grad_shift, int batch, int channels, int64_t voxels, int act, float* scratch,
                      int64_t scratch_elems, void* stream) {
    if (!grad_x && !grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "head backward: grad_x, grad_w and grad_shift are all NULL (each may be: it is not computed)");
    if (act < S3R_ACT_NONE || act > S3R_ACT_SIGMOID)
        return fail(S3R_ERR_INVALID, "s3r_head_backward takes none / relu / sigmoid (act %d)", act);
    int rc = headbwd_dims(batch, channels, voxels);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if (!grad_y || (grad_w && !x) || (grad_x && !w)) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (act != S3R_ACT_NONE && !y) return fail(S3R_ERR_INVALID, "head backward: y is NULL (it may be only when act is none)");
    const int64_t need = s3r::head_backward_scratch_elems(batch, channels, voxels);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "head backward needs %lld floats of scratch (s3r_head_backward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)stream;
    const double B = batch, C = channels, S = (double)voxels;
    const double flops = (grad_w ? 2.0 * B * C * S : 0.0) + (grad_x ? B * C * S : 0.0);
    const double elems = B * S * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale ? 1.0 : 0.0) + (grad_w ? B * C * S + C : 0.0) +
                         (grad_x ? C + B * C * S : 0.0) + (grad_shift ? 1.0 : 0.0);
    ProfScope ps(s, F_HEAD, 1, flops, 4.0 * elems);
    hipError_t e = s3r::launch_head_backward(x, w, scale, y, grad_y, grad_x, grad_w, grad_shift, batch, channels, voxels, act, scratch, s,
                                             &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "head backward launch");
    return S3R_OK;
}

// what the conv-backward entry points take: an fp32 Conv / ConvTranspose, dilation 1, plain tensors without halos, none / relu / sigmoid.
// `batch_min` 0: s3r_conv_backward and its scratch query accept an empty batch.  Fills the geometry (of batch max(batch, 1)) and tiling
static int convbwd_check(const s3r_conv_desc* d, const char* who, int batch_min, Geo* g, s3r::ConvBwdGeo* cg) {
    if (!d) return fail(S3R_ERR_INVALID, "%s: null descriptor", who);
    if (d->dtype != S3R_F32) return fail(S3R_ERR_INVALID, "%s: fp32 layers only (dtype %d)", who, d->dtype);
    if (d->op != S3R_OP_CONV && d->op != S3R_OP_DECONV)
        return fail(S3R_ERR_INVALID, "%s: Conv / ConvTranspose layers only (op %d; linear layers have s3r_linear_backward)", who, d->op);
    if (dil_of(d) != 1) return fail(S3R_ERR_INVALID, "%s: dilation 1 only (got %d)", who, d->dilation);
    if (d->in_layout != S3R_LAYOUT_PLAIN || d->out_layout != S3R_LAYOUT_PLAIN || d->in_halo != 0 || d->out_halo != 0)
        return fail(S3R_ERR_INVALID, "%s: plain tensors only (layouts PLAIN, halos 0)", who);
    if (d->act < S3R_ACT_NONE || d->act > S3R_ACT_SIGMOID) return fail(S3R_ERR_INVALID, "%s takes none / relu / sigmoid (act %d)", who, d->act);
    if (d->batch < batch_min) return fail(S3R_ERR_INVALID, "%s: batch must be >= %d (got %d)", who, batch_min, d->batch);
    s3r_conv_desc one = *d;
    if (one.batch == 0) one.batch = 1;
    int rc = geometry(&one, g);
    if (rc) return rc;
    if (g->w_elems >= kMaxElems) return fail(S3R_ERR_INVALID, "%s: weight of 2^31 elements or more", who);
    if (!s3r::convbwd_geo(d->op == S3R_OP_DECONV, d->ndim, d->cin, d->cout, g->in, g->out, d->k, d->stride, d->pad, cg))
        return fail(S3R_ERR_INVALID, "%s: no tiling of the weight-gradient GEMM fits this kernel size / stride (k %d, stride %d)", who, d->k,
                    d->stride);
    if ((int64_t)d->batch * cg->nsl * cg->tiles >= kMaxElems) return fail(S3R_ERR_INVALID, "%s: too many workgroups: split the batch", who);
    return S3R_OK;
}

int s3r_conv_adjoint_desc(const s3r_conv_desc* d, s3r_conv_desc* adj) {
    Geo g, ga;
    s3r::ConvBwdGeo cg;
    if (!adj) return fail(S3R_ERR_INVALID, "s3r_conv_adjoint_desc: null output descriptor");
    int rc = convbwd_check(d, "s3r_conv_adjoint_desc", 1, &g, &cg);
    if (rc) return rc;
    s3r_conv_desc a;
    memset(&a, 0, sizeof(a));
    a.op = d->op == S3R_OP_CONV ? S3R_OP_DECONV : S3R_OP_CONV;
    a.ndim = d->ndim; a.batch = d->batch; a.tag = d->tag;
    a.cin = d->cout; a.cout = d->cin;
    a.in_size = g.out;
    a.k = d->k; a.stride = d->stride; a.pad = d->pad;
    a.act = S3R_ACT_NONE; a.tile = -1; a.dtype = S3R_F32; a.algo = S3R_ALGO_AUTO; a.dilation = 1;
    a.out_pad = d->op == S3R_OP_CONV ? (d->in_size + 2 * d->pad - d->k) % d->stride : 0;
    rc = geometry(&a, &ga);                                              // (a Conv with pad > k - 1 has no ConvTranspose this library runs)
    if (rc) return rc;
    if (ga.out != d->in_size) return fail(S3R_ERR_INVALID, "s3r_conv_adjoint_desc: internal: adjoint output edge %d != input edge %d", ga.out, d->in_size);
    *adj = a;
    return S3R_OK;
}

int64_t s3r_conv_backward_scratch_elems(const s3r_conv_desc* d) {
    Geo g;
    s3r::ConvBwdGeo cg;
    int rc = convbwd_check(d, "s3r_conv_backward_scratch_elems", 0, &g, &cg);
    if (rc) return rc;
    if (d->batch == 0) return 0;
    return s3r::conv_backward_scratch_elems(cg, d->batch, d->cout, g.out_sp);
}

int s3r_conv_backward(const s3r_conv_desc* d, const float* x, const float* y, const float* grad_y, const float* scale, float* gs,
                      float* grad_w, float* grad_shift, float* scratch, int64_t scratch_elems, void* hip_stream) {
    if (!gs && !grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "conv backward: gs, grad_w and grad_shift are all NULL (each may be: it is not computed)");
    Geo g;
    s3r::ConvBwdGeo cg;
    int rc = convbwd_check(d, "s3r_conv_backward", 0, &g, &cg);
    if (rc) return rc;
    if (d->batch == 0) return S3R_OK;
    if (!grad_y || (grad_w && !x)) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (d->act != S3R_ACT_NONE && !y) return fail(S3R_ERR_INVALID, "conv backward: y is NULL (it may be only when act is none)");
    const int64_t need = s3r::conv_backward_scratch_elems(cg, d->batch, d->cout, g.out_sp);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "conv backward needs %lld floats of scratch (s3r_conv_backward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)hip_stream;
    const double B = d->batch, Y = B * d->cout * (double)g.out_sp, X = B * d->cin * (double)g.in_sp;
    const double flops = grad_w ? 2.0 * B * (double)cg.Q * cg.Ca * cg.Cf * cg.T : 0.0;
    const double elems = Y * (d->act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale ? d->cout : 0.0) + (gs ? Y : 0.0) +
                         (grad_w ? X + (double)g.w_elems : 0.0) + (grad_shift ? d->cout : 0.0);
    ProfScope ps(s, F_MFMA, S3R_CONV_BACKWARD_TAG + d->tag, flops, 4.0 * elems);
    hipError_t e = s3r::launch_conv_backward(cg, d->op == S3R_OP_DECONV, x, y, grad_y, scale, gs, grad_w, grad_shift, d->batch, d->cout,
                                             g.out_sp, d->act, scratch, s, &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "conv backward launch");
    return S3R_OK;
}

// the stem backward's shape: in_size >= 1, n_images >= 0, y / grad_y (n_images,32,m,m) within the header's limits; fills m
static int stembwd_dims(int n_images, int in_size, const char* who, int* m_out) {
    if (n_images < 0 || in_size < 1)
        return fail(S3R_ERR_INVALID, "%s: n_images >= 0 and in_size >= 1 (n_images %d, in_size %d)", who, n_images, in_size);
    const int64_t m = (in_size - 1) / 2 + 1;
    const int64_t Y = (int64_t)n_images * 32 * m * m;
    if (32 * m * m >= kMaxElems || Y >= kMaxElems || 4 * Y >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "%s: tensor of 2^31 elements / 4 GiB or more: split the batch", who);
    *m_out = (int)m;
    return S3R_OK;
}

int64_t s3r_stem_backward_scratch_elems(int n_images, int in_size) {
    int m = 0;
    int rc = stembwd_dims(n_images, in_size, "s3r_stem_backward_scratch_elems", &m);
    if (rc) return rc;
    return s3r::stem_backward_scratch_elems(n_images, m);
}

int s3r_stem_backward(const void* images_left, const void* images_right, int n_left, int renders_u8, const float* y, const float* grad_y,
                      const float* scale, float* grad_w, float* grad_shift, int n_images, int in_size, int act, float* scratch,
                      int64_t scratch_elems, void* hip_stream) {
    if (!grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "stem backward: grad_w and grad_shift are both NULL (each may be: it is not computed)");
    if (act != S3R_ACT_NONE && act != S3R_ACT_RELU) return fail(S3R_ERR_INVALID, "s3r_stem_backward takes none / relu (act %d)", act);
    int m = 0;
    int rc = stembwd_dims(n_images, in_size, "s3r_stem_backward", &m);
    if (rc) return rc;
    if (n_images == 0) return S3R_OK;
    if (images_right ? (n_left < 1 || n_left > n_images) : n_left != n_images)
        return fail(S3R_ERR_INVALID, "stem backward: n_left must lie in [1, n_images] with two render tensors and equal n_images with one "
                                     "(n_left %d, n_images %d)", n_left, n_images);
    if (!images_left || !grad_y) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (act != S3R_ACT_NONE && !y) return fail(S3R_ERR_INVALID, "stem backward: y is NULL (it may be only when act is none)");
    if ((((uintptr_t)images_left) | ((uintptr_t)images_right)) & 15)
        return fail(S3R_ERR_INVALID, "render tensors must be 16-byte aligned (got %p, %p)", images_left, images_right);
    const int64_t P = (int64_t)in_size * in_size;
    const int64_t big = 3 * P * (n_left > n_images - n_left ? n_left : n_images - n_left);
    if (big >= kMaxElems || (renders_u8 ? 1 : 4) * big >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "stem backward: render tensor of 2^31 elements / 4 GiB or more: split the batch");
    const int64_t need = s3r::stem_backward_scratch_elems(n_images, m);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "stem backward needs %lld floats of scratch (s3r_stem_backward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)hip_stream;
    const double B = n_images, Y = B * 32.0 * (double)m * m;
    const double flops = grad_w ? 2.0 * B * (double)m * m * 32.0 * 27.0 : 0.0;
    const double bytes = 4.0 * (Y * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale && grad_w ? 32.0 : 0.0) + (grad_w ? 864.0 : 0.0) +
                                (grad_shift ? 32.0 : 0.0)) + (grad_w ? (renders_u8 ? 1.0 : 4.0) * B * 3.0 * (double)P : 0.0);
    ProfScope ps(s, F_STEM, 1, flops, bytes);
    hipError_t e = s3r::launch_stem_backward(images_left, images_right, n_left, renders_u8 != 0, y, grad_y, scale, grad_w, grad_shift,
                                             n_images, in_size, m, act, scratch, s, &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "stem backward launch");
    return S3R_OK;
}

// z / y / grad_z of a train-mode BatchNorm call within the header's limits (< 2^31 elements, < 4 GiB)
static int bn_dims(int batch, int channels, int64_t positions) {
    if (batch < 0 || channels <= 0 || positions <= 0)
        return fail(S3R_ERR_INVALID, "batchnorm dims: batch >= 0, channels > 0 and positions > 0 (batch %d, channels %d, positions %lld)", batch,
                    channels, (long long)positions);
    if (positions >= kMaxElems || (int64_t)channels * positions >= kMaxElems || (int64_t)batch * channels * positions >= kMaxElems ||
        4 * (int64_t)batch * channels * positions >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the channels");
    return S3R_OK;
}

static int bn_act_ok(int act, const char* who) {
    if (act < S3R_ACT_NONE || act > S3R_ACT_SIGMOID) return fail(S3R_ERR_INVALID, "%s takes none / relu / sigmoid (act %d)", who, act);
    return S3R_OK;
}

int64_t s3r_batchnorm_train_forward_scratch_elems(int batch, int channels, int64_t positions) {
    int rc = bn_dims(batch, channels, positions);
    if (rc) return rc;
    return s3r::batchnorm_forward_scratch_elems(batch, channels, positions);
}

int64_t s3r_batchnorm_train_backward_scratch_elems(int batch, int channels, int64_t positions) {
    int rc = bn_dims(batch, channels, positions);
    if (rc) return rc;
    return s3r::batchnorm_backward_scratch_elems(batch, channels, positions);
}

int s3r_batchnorm_train_forward(const float* z, const float* gamma, const float* beta, float eps, int act, float* y, float* save_mean,
                                float* save_var, float* save_invstd, int batch, int channels, int64_t positions, float* scratch,
                                int64_t scratch_elems, void* hip_stream) {
    int rc = bn_act_ok(act, "s3r_batchnorm_train_forward");
    if (rc) return rc;
    rc = bn_dims(batch, channels, positions);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if ((int64_t)batch * positions < 2)
        return fail(S3R_ERR_INVALID, "batchnorm: batch statistics need more than one value per channel (batch * positions = 1)");
    if (!z || !gamma || !beta || !y || !save_mean || !save_var || !save_invstd) return fail(S3R_ERR_INVALID, "null tensor pointer");
    const int64_t need = s3r::batchnorm_forward_scratch_elems(batch, channels, positions);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "batchnorm forward needs %lld floats of scratch (s3r_batchnorm_train_forward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)hip_stream;
    const double T = (double)batch * channels * (double)positions;
    ProfScope ps(s, F_HEAD, 2, 0.0, 4.0 * (4.0 * T + 5.0 * channels));
    hipError_t e = s3r::launch_batchnorm_train_forward(z, gamma, beta, eps, act, y, save_mean, save_var, save_invstd, batch, channels,
                                                       positions, scratch, s, &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "batchnorm forward launch");
    return S3R_OK;
}

int s3r_batchnorm_train_backward(const float* z, const float* y, const float* grad_y, const float* gamma, const float* save_mean,
                                 const float* save_invstd, int act, float* grad_z, float* grad_gamma, float* grad_beta, int batch,
                                 int channels, int64_t positions, float* scratch, int64_t scratch_elems, void* hip_stream) {
    if (!grad_z && !grad_gamma && !grad_beta)
        return fail(S3R_ERR_INVALID, "batchnorm backward: grad_z, grad_gamma and grad_beta are all NULL (each may be: it is not computed)");
    int rc = bn_act_ok(act, "s3r_batchnorm_train_backward");
    if (rc) return rc;
    rc = bn_dims(batch, channels, positions);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if ((int64_t)batch * positions < 2)
        return fail(S3R_ERR_INVALID, "batchnorm: batch statistics need more than one value per channel (batch * positions = 1)");
    const bool gg = grad_gamma || grad_z;
    if (!grad_y || (gg && (!z || !save_mean || !save_invstd)) || (grad_z && !gamma)) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (act != S3R_ACT_NONE && !y) return fail(S3R_ERR_INVALID, "batchnorm backward: y is NULL (it may be only when act is none)");
    const int64_t need = s3r::batchnorm_backward_scratch_elems(batch, channels, positions);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_WORKSPACE, "batchnorm backward needs %lld floats of scratch (s3r_batchnorm_train_backward_scratch_elems), got %lld",
                    (long long)need, (long long)(scratch ? scratch_elems : 0));
    hipStream_t s = (hipStream_t)hip_stream;
    const double T = (double)batch * channels * (double)positions;
    const double reads = 1.0 + (act != S3R_ACT_NONE ? 1.0 : 0.0) + (gg ? 1.0 : 0.0);
    ProfScope ps(s, F_HEAD, 3, 0.0, 4.0 * (T * (grad_z ? 2.0 * reads + 1.0 : reads) + (double)channels * ((gg ? 2.0 : 0.0) + (grad_z ? 1.0 : 0.0) +
                                                 (grad_gamma ? 1.0 : 0.0) + (grad_beta ? 1.0 : 0.0))));
    hipError_t e = s3r::launch_batchnorm_train_backward(z, y, grad_y, gamma, save_mean, save_invstd, act, grad_z, grad_gamma, grad_beta, batch,
                                                        channels, positions, scratch, s, &ps.launches);
    if (e != hipSuccess) return hip_fail(e, "batchnorm backward launch");
    return S3R_OK;
}

int s3r_disparity_wta(const float* feat_l, const float* feat_r, float* disp_l, float* disp_r, int batch, int channels,
                      int height, int width, int max_disp, void* stream) {
    if (!feat_l || !feat_r || !disp_l || !disp_r) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || max_disp <= 0)
        return fail(S3R_ERR_INVALID, "disparity dims must be positive");
    if ((size_t)2 * channels * width * sizeof(float) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "disparity read-out: a feature row pair (2*C*W floats) must fit 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    const double px = (double)batch * height * width;
    ProfScope ps(s, F_DISP, 0, 0.0, 4.0 * px * (2.0 * channels + 2.0));
    hipError_t e = s3r::launch_disparity_wta(feat_l, feat_r, disp_l, disp_r, batch, channels, max_disp, height, width, s);
    if (e != hipSuccess) return hip_fail(e, "disparity read-out launch");
    return S3R_OK;
}

int s3r_disparity_epe(const float* pred, const float* gt, float* epe, int32_t* count, int batch, int64_t pixels,
                      void* stream) {
    if (!pred || !gt || !epe || !count) return fail(S3R_ERR_INVALID, "null tensor pointer");
    if (batch <= 0 || pixels <= 0) return fail(S3R_ERR_INVALID, "epe dims must be positive");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_DISP, 1, 0.0, 8.0 * batch * (double)pixels);
    hipError_t e = s3r::launch_disparity_epe(pred, gt, epe, count, batch, pixels, s);
    if (e != hipSuccess) return hip_fail(e, "epe launch");
    return S3R_OK;
}

// ---------------------------------------------------------------- sub-pixel read-out and stereo metrics (s3r_disparity.hip)

// The soft read-out's argument checks, shared by the forward and its backward (one message path: what the forward refuses, the
// backward refuses in the same words).  soft_args: temperature and dims; soft_shape: the LDS rule and the size limits.
static int soft_args(int batch, int channels, int height, int width, int max_disp, float temperature, int out_height, int out_width) {
    if (!(temperature > 0.f) || !std::isfinite(temperature))
        return fail(S3R_ERR_INVALID, "soft read-out temperature must be finite and > 0 (got %g)", (double)temperature);
    if (batch < 0 || channels <= 0 || height <= 0 || width <= 0 || max_disp <= 0 || out_height <= 0 || out_width <= 0)
        return fail(S3R_ERR_INVALID, "soft read-out dims must be positive (batch >= 0)");
    return S3R_OK;
}

static int soft_shape(int batch, int channels, int height, int width, int max_disp, int out_height, int out_width) {
    if (s3r::disparity_soft_lds_bytes(channels, max_disp, width) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "soft read-out: 4*(2*C*W + 2*W*min(max_disp, W) + 12*W) bytes must fit 64 KiB of LDS");
    const int64_t feat = (int64_t)batch * channels * height * width;
    const int64_t out = (int64_t)batch * out_height * out_width;
    if (feat >= kMaxElems || out >= kMaxElems) return fail(S3R_ERR_INVALID, "tensor of 2^31 elements or more: split the batch");
    if ((int64_t)batch * out_height >= (1 << 24))      // at most one workgroup of 256 per output row: < 2^32 work-items
        return fail(S3R_ERR_INVALID, "batch x out_height must stay below 2^24: split the batch");
    return S3R_OK;
}

int s3r_disparity_soft(const void* feat_l, const void* feat_r, int feat_dtype, float* disp_l, float* disp_r, float* conf_l,
                       float* conf_r, int batch, int channels, int height, int width, int max_disp, float temperature,
                       int out_height, int out_width, float disp_scale, void* stream) {
    int rc = soft_args(batch, channels, height, width, max_disp, temperature, out_height, out_width);
    if (rc) return rc;
    if (feat_dtype != S3R_F32 && feat_dtype != S3R_BF16) return fail(S3R_ERR_INVALID, "unknown feature dtype %d", feat_dtype);
    const bool bf16 = feat_dtype == S3R_BF16;
    if (bf16 && channels % 8 != 0) return fail(S3R_ERR_INVALID, "bf16 channels-last features need channels %% 8 == 0");
    if (bf16 && batch > 0 && (((uintptr_t)feat_l | (uintptr_t)feat_r) & 15))
        return fail(S3R_ERR_INVALID, "bf16 features must start 16-byte aligned (16-byte loads)");
    rc = soft_shape(batch, channels, height, width, max_disp, out_height, out_width);
    if (rc) return rc;
    const int64_t feat = (int64_t)batch * channels * height * width;
    const int64_t out = (int64_t)batch * out_height * out_width;
    if (batch == 0) return S3R_OK;
    if (!feat_l || !feat_r) return fail(S3R_ERR_INVALID, "null feature pointer");
    hipStream_t s = (hipStream_t)stream;
    const int maps = !!disp_l + !!disp_r + !!conf_l + !!conf_r;
    ProfScope ps(s, F_DISP, 2, 0.0, (bf16 ? 2.0 : 4.0) * 2.0 * (double)feat + 4.0 * maps * (double)out);
    hipError_t e = s3r::launch_disparity_soft(feat_l, feat_r, bf16, disp_l, disp_r, conf_l, conf_r, batch, channels, max_disp,
                                              height, width, temperature, out_height, out_width, disp_scale, s);
    if (e != hipSuccess) return hip_fail(e, "soft disparity read-out launch");
    return S3R_OK;
}

int s3r_disparity_metrics(const float* pred, const float* gt, float* epe, int32_t* counts, int batch, int64_t pixels,
                          void* stream) {
    if (batch < 0 || pixels < 0) return fail(S3R_ERR_INVALID, "metrics dims must be >= 0 (batch %d, pixels %lld)", batch,
                                             (long long)pixels);
    if (batch > 65535) return fail(S3R_ERR_INVALID, "batch > 65535: split the call");
    if (pixels >= kMaxElems || (int64_t)batch * pixels >= kMaxElems) return fail(S3R_ERR_INVALID, "tensor of 2^31 elements or more: split the batch");
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !epe || !counts) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_DISP, 3, 0.0, 8.0 * batch * (double)pixels + 20.0 * batch);
    hipError_t e = s3r::launch_disparity_metrics(pred, gt, epe, counts, batch, pixels, s);
    if (e != hipSuccess) return hip_fail(e, "disparity metrics launch");
    return S3R_OK;
}

// ---------------------------------------------------------------- disparity supervision (s3r_disparity_bwd.hip, s3r_disparity_loss.hip)
int s3r_disparity_soft_backward(const void* feat_l, const void* feat_r, int feat_dtype, const float* grad_disp_l,
                                const float* grad_disp_r, float* grad_left, float* grad_right, int batch, int channels, int height,
                                int width, int max_disp, float temperature, int out_height, int out_width, float disp_scale,
                                void* hip_stream) {
    if (!grad_disp_l && !grad_disp_r)
        return fail(S3R_ERR_INVALID, "soft read-out backward: grad_disp_l and grad_disp_r are both NULL (either may be: it counts as zeros)");
    if (!grad_left && !grad_right)
        return fail(S3R_ERR_INVALID, "soft read-out backward: grad_left and grad_right are both NULL (either may be: it is not computed)");
    int rc = soft_args(batch, channels, height, width, max_disp, temperature, out_height, out_width);
    if (rc) return rc;
    if (feat_dtype == S3R_BF16)
        return fail(S3R_ERR_INVALID, "soft read-out backward: bf16 features have no backward (fp32 NCHW features only)");
    if (feat_dtype != S3R_F32) return fail(S3R_ERR_INVALID, "unknown feature dtype %d", feat_dtype);
    rc = soft_shape(batch, channels, height, width, max_disp, out_height, out_width);
    if (rc) return rc;
    if ((int64_t)batch * height >= (1 << 24))          // one workgroup of 256 per feature row: < 2^32 work-items
        return fail(S3R_ERR_INVALID, "batch x height must stay below 2^24: split the batch");
    if (batch == 0) return S3R_OK;
    if (!feat_l || !feat_r) return fail(S3R_ERR_INVALID, "null feature pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const double feat = (double)batch * channels * height * width;
    const double out = (double)batch * out_height * out_width;
    const int grads = !!grad_disp_l + !!grad_disp_r, outs = !!grad_left + !!grad_right;
    ProfScope ps(s, F_DISP, 4, 0.0, 4.0 * (2.0 * feat + grads * out + outs * feat));
    hipError_t e = s3r::launch_disparity_soft_backward((const float*)feat_l, (const float*)feat_r, grad_disp_l, grad_disp_r, grad_left,
                                                       grad_right, batch, channels, max_disp, height, width, temperature, out_height,
                                                       out_width, disp_scale, s);
    if (e != hipSuccess) return hip_fail(e, "soft disparity read-out backward launch");
    return S3R_OK;
}

static int disp_loss_dims(int batch, int64_t pixels, float beta) {
    if (!(beta >= 0.f) || !std::isfinite(beta))
        return fail(S3R_ERR_INVALID, "disparity loss: beta must be finite and >= 0 (got %g)", (double)beta);
    if (batch < 0 || pixels <= 0)
        return fail(S3R_ERR_INVALID, "disparity loss dims: batch >= 0 and pixels > 0 (batch %d, pixels %lld)", batch, (long long)pixels);
    if (pixels >= kMaxElems || (int64_t)batch * pixels >= kMaxElems || 4 * (int64_t)batch * pixels >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "tensor of 2^31 elements or more: split the batch");
    return S3R_OK;
}

int s3r_disparity_loss_forward(const float* pred, const float* gt, float beta, float* loss_sum, int32_t* count, float* loss_elem,
                               int batch, int64_t pixels, void* hip_stream) {
    int rc = disp_loss_dims(batch, pixels, beta);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !loss_sum || !count) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const double n = (double)batch * (double)pixels;
    ProfScope ps(s, F_DISP, 5, 0.0, 4.0 * (n * (loss_elem ? 3.0 : 2.0) + 2.0 * batch));
    hipError_t e = s3r::launch_disparity_loss(pred, gt, beta, loss_sum, count, loss_elem, batch, pixels, s);
    if (e != hipSuccess) return hip_fail(e, "disparity loss launch");
    return S3R_OK;
}

int s3r_disparity_loss_backward(const float* pred, const float* gt, const float* grad_scale, float beta, float* grad_pred, int batch,
                                int64_t pixels, void* hip_stream) {
    int rc = disp_loss_dims(batch, pixels, beta);
    if (rc) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !grad_scale || !grad_pred) return fail(S3R_ERR_INVALID, "null tensor pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    ProfScope ps(s, F_DISP, 6, 0.0, 4.0 * (3.0 * batch * (double)pixels + batch));
    hipError_t e = s3r::launch_disparity_loss_backward(pred, gt, grad_scale, beta, grad_pred, batch, pixels, s);
    if (e != hipSuccess) return hip_fail(e, "disparity loss backward launch");
    return S3R_OK;
}

// ---------------------------------------------------------------- optimizer step (s3r_optim.hip)
namespace {

bool optim_bad(float x, bool below_one) { return !std::isfinite(x) || x < 0.f || (below_one && x >= 1.f); }

// the list's own checks, shared by the query and the step: pointers are looked at by the step only (`need_m`, `need_v` < 0: the query)
int optim_list(const s3r_optim_tensor* t, int n_tensors, int need_m, int need_v) {
    if (!t) return fail(S3R_ERR_INVALID, "optimizer: null tensor list");
    if (n_tensors <= 0 || n_tensors > S3R_OPTIM_MAX_TENSORS)
        return fail(S3R_ERR_INVALID, "optimizer: n_tensors = %d must be in [1, %d]", n_tensors, S3R_OPTIM_MAX_TENSORS);
    for (int i = 0; i < n_tensors; ++i) {
        if (t[i].elems <= 0 || t[i].elems >= kMaxElems)
            return fail(S3R_ERR_INVALID, "optimizer: tensor %d has elems = %lld (must be in [1, 2^31))", i, (long long)t[i].elems);
        if (need_m < 0) continue;
        if (!t[i].param || !t[i].grad) return fail(S3R_ERR_INVALID, "optimizer: tensor %d has a null param or grad", i);
        if (need_m && !t[i].m) return fail(S3R_ERR_INVALID, "optimizer: tensor %d has a null m (momentum / first moment)", i);
        if (need_v && !t[i].v) return fail(S3R_ERR_INVALID, "optimizer: tensor %d has a null v (second moment)", i);
    }
    if (s3r::optim_chunks(t, n_tensors) + n_tensors >= kMaxElems) return fail(S3R_ERR_INVALID, "optimizer: the list has 2^31 chunks or more");
    return S3R_OK;
}

bool optim_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    return a && b && x < y + bytes && y < x + bytes;
}

}  // namespace

int64_t s3r_optim_scratch_elems(const s3r_optim_tensor* t, int n_tensors) {
    int rc = optim_list(t, n_tensors, -1, -1);
    if (rc) return rc;
    return s3r::optim_chunks(t, n_tensors) + n_tensors;
}

int s3r_optim_state_init(float* state, float lr, void* hip_stream) {
    if (!state) return fail(S3R_ERR_INVALID, "optimizer: null state");
    if (optim_bad(lr, false)) return fail(S3R_ERR_INVALID, "optimizer: lr must be finite and >= 0");
    hipError_t e = s3r::launch_optim_state_init(state, lr, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "optimizer state init launch");
    return S3R_OK;
}

int s3r_optim_set_lr(float* state, float lr, void* hip_stream) {
    if (!state) return fail(S3R_ERR_INVALID, "optimizer: null state");
    if (optim_bad(lr, false)) return fail(S3R_ERR_INVALID, "optimizer: lr must be finite and >= 0");
    hipError_t e = s3r::launch_optim_set_lr(state, lr, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "optimizer set-lr launch");
    return S3R_OK;
}

int s3r_optim_step(const s3r_optim_desc* d, const s3r_optim_tensor* t, int n_tensors, float* state, float* scratch,
                   int64_t scratch_elems, void* hip_stream) {
    if (!d) return fail(S3R_ERR_INVALID, "optimizer: null descriptor");
    if (d->kind != S3R_OPT_SGD && d->kind != S3R_OPT_ADAM) return fail(S3R_ERR_INVALID, "optimizer: unknown kind %d", d->kind);
    const int known = S3R_OPT_DECOUPLED_DECAY | S3R_OPT_NESTEROV | S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE;
    if (d->flags & ~known) return fail(S3R_ERR_INVALID, "optimizer: unknown flag bits 0x%x", d->flags & ~known);
    const bool adam = d->kind == S3R_OPT_ADAM;
    if (optim_bad(d->beta1, true)) return fail(S3R_ERR_INVALID, "optimizer: beta1 (SGD: momentum) must be finite and in [0, 1)");
    if (adam && optim_bad(d->beta2, true)) return fail(S3R_ERR_INVALID, "optimizer: beta2 must be finite and in [0, 1)");
    if (adam && optim_bad(d->eps, false)) return fail(S3R_ERR_INVALID, "optimizer: eps must be finite and >= 0");
    if (optim_bad(d->weight_decay, false)) return fail(S3R_ERR_INVALID, "optimizer: weight_decay must be finite and >= 0");
    if (optim_bad(d->max_norm, false)) return fail(S3R_ERR_INVALID, "optimizer: max_norm must be finite and >= 0");
    if ((d->flags & S3R_OPT_NESTEROV) && (adam || d->beta1 == 0.f))
        return fail(S3R_ERR_INVALID, "optimizer: the nesterov flag needs SGD with momentum");
    if ((d->flags & S3R_OPT_DECOUPLED_DECAY) && !adam) return fail(S3R_ERR_INVALID, "optimizer: the decoupled-decay flag needs Adam");
    if (!state) return fail(S3R_ERR_INVALID, "optimizer: null state");
    const bool need_m = adam || d->beta1 != 0.f;
    int rc = optim_list(t, n_tensors, need_m, adam);
    if (rc) return rc;
    const bool with_norm = (d->flags & (S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE)) != 0;
    if (with_norm) {
        const int64_t need = s3r::optim_chunks(t, n_tensors) + n_tensors;
        if (!scratch || scratch_elems < need)
            return fail(S3R_ERR_INVALID, "optimizer: the gradient norm needs %lld floats of scratch (s3r_optim_scratch_elems), got %lld",
                        (long long)need, scratch ? (long long)scratch_elems : 0ll);
    }
    std::vector<std::pair<uintptr_t, int>> ps((size_t)n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        const float* m = need_m ? t[i].m : nullptr;
        const float* v = adam ? t[i].v : nullptr;
        if (optim_overlap(t[i].param, m, t[i].elems) || optim_overlap(t[i].param, v, t[i].elems) || optim_overlap(m, v, t[i].elems))
            return fail(S3R_ERR_INVALID, "optimizer: tensor %d: param, m and v overlap", i);
        ps[(size_t)i] = {(uintptr_t)t[i].param, i};
    }
    std::sort(ps.begin(), ps.end());
    for (int i = 1; i < n_tensors; ++i)
        if (ps[(size_t)i].first == ps[(size_t)i - 1].first)
            return fail(S3R_ERR_INVALID, "optimizer: tensors %d and %d have the same param", ps[(size_t)i - 1].second, ps[(size_t)i].second);
    hipError_t e = s3r::launch_optim_step(d->kind, d->flags, d->beta1, d->beta2, d->eps, d->weight_decay, d->max_norm, t, n_tensors, state,
                                          scratch, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "optimizer step launch");
    return S3R_OK;
}

// ---------------------------------------------------------------- stereo augmentation (s3r_augment.hip)
namespace {

bool augment_bad_range(float lo, float hi) { return !std::isfinite(lo) || !std::isfinite(hi) || lo < 0.f || lo > hi; }

// the descriptor's and the shape's own checks, shared by the query and the call
int augment_shape(const s3r_augment_desc* d, int batch, int height, int width) {
    if (!d) return fail(S3R_ERR_INVALID, "augment: null descriptor");
    if (d->channels != 3 && d->channels != 4) return fail(S3R_ERR_INVALID, "augment: channels = %d must be 3 (RGB) or 4 (RGBA)", d->channels);
    if (batch <= 0 || height <= 0 || width <= 0)
        return fail(S3R_ERR_INVALID, "augment: batch = %d, height = %d, width = %d must be positive", batch, height, width);
    const int64_t S = (int64_t)height * width;
    if (S >= kMaxElems) return fail(S3R_ERR_INVALID, "augment: height * width = %lld must be below 2^31", (long long)S);
    if ((int64_t)batch > (kMaxElems - 1) / (d->channels * S))
        return fail(S3R_ERR_INVALID, "augment: a tensor of the call has 2^31 elements or more: split the batch");
    if (d->max_shift < 0 || d->max_shift > S3R_AUG_MAX_SHIFT)
        return fail(S3R_ERR_INVALID, "augment: max_shift = %d must be in [0, %d]", d->max_shift, S3R_AUG_MAX_SHIFT);
    if (d->flags & ~S3R_AUG_PERMUTE_RGB) return fail(S3R_ERR_INVALID, "augment: unknown flag bits 0x%x", d->flags & ~S3R_AUG_PERMUTE_RGB);
    if (d->bg_lo < 0 || d->bg_hi > 255 || d->bg_lo > d->bg_hi)
        return fail(S3R_ERR_INVALID, "augment: background codes [%d, %d] must satisfy 0 <= lo <= hi <= 255", d->bg_lo, d->bg_hi);
    if (augment_bad_range(d->brightness_lo, d->brightness_hi)) return fail(S3R_ERR_INVALID, "augment: the brightness range must be finite with 0 <= lo <= hi");
    if (augment_bad_range(d->contrast_lo, d->contrast_hi)) return fail(S3R_ERR_INVALID, "augment: the contrast range must be finite with 0 <= lo <= hi");
    if (augment_bad_range(d->saturation_lo, d->saturation_hi)) return fail(S3R_ERR_INVALID, "augment: the saturation range must be finite with 0 <= lo <= hi");
    if (!std::isfinite(d->noise_sigma) || d->noise_sigma < 0.f) return fail(S3R_ERR_INVALID, "augment: noise_sigma must be finite and >= 0");
    return S3R_OK;
}

int64_t augment_need(const s3r_augment_desc* d, int batch, int height, int width) {
    return s3r::augment_scratch(d, batch, (int64_t)height * width);
}

struct AugSpan { const void* p; int64_t bytes; const char* name; };
bool augment_overlap(const AugSpan& a, const AugSpan& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + (uintptr_t)b.bytes && y < x + (uintptr_t)a.bytes;
}

}  // namespace

int64_t s3r_augment_scratch_elems(const s3r_augment_desc* d, int batch, int height, int width) {
    int rc = augment_shape(d, batch, height, width);
    if (rc) return rc;
    return augment_need(d, batch, height, width);
}

int s3r_augment_pair(const s3r_augment_desc* d, const uint8_t* left, const uint8_t* right, const int64_t* sample_ids,
                     const float* disp_left, const float* disp_right, float* out_left, float* out_right,
                     float* out_disp_left, float* out_disp_right, int batch, int height, int width,
                     float* scratch, int64_t scratch_elems, void* hip_stream) {
    int rc = augment_shape(d, batch, height, width);
    if (rc) return rc;
    if (!left || !right || !sample_ids) return fail(S3R_ERR_INVALID, "augment: null left, right or sample_ids");
    if (!out_left || !out_right) return fail(S3R_ERR_INVALID, "augment: null out_left or out_right");
    const int given = (disp_left != nullptr) + (disp_right != nullptr) + (out_disp_left != nullptr) + (out_disp_right != nullptr);
    if (given != 0 && given != 4)
        return fail(S3R_ERR_INVALID, "augment: disp_left, disp_right, out_disp_left and out_disp_right must be all NULL or all given");
    const int64_t need = augment_need(d, batch, height, width);
    if (need > 0 && (!scratch || scratch_elems < need))
        return fail(S3R_ERR_INVALID, "augment: contrast needs %lld floats of scratch (s3r_augment_scratch_elems), got %lld",
                    (long long)need, scratch ? (long long)scratch_elems : 0ll);
    const int64_t S = (int64_t)height * width, px = (int64_t)batch * S;
    const AugSpan outs[5] = {{out_left, 12 * px, "out_left"}, {out_right, 12 * px, "out_right"}, {out_disp_left, 4 * px, "out_disp_left"},
                             {out_disp_right, 4 * px, "out_disp_right"}, {need > 0 ? scratch : nullptr, 4 * need, "scratch"}};
    const AugSpan ins[5] = {{left, d->channels * px, "left"}, {right, d->channels * px, "right"}, {sample_ids, 8 * (int64_t)batch, "sample_ids"},
                            {disp_left, 4 * px, "disp_left"}, {disp_right, 4 * px, "disp_right"}};
    for (int i = 0; i < 5; ++i) {
        for (int j = i + 1; j < 5; ++j)
            if (augment_overlap(outs[i], outs[j])) return fail(S3R_ERR_INVALID, "augment: %s and %s overlap", outs[i].name, outs[j].name);
        for (int j = 0; j < 5; ++j)
            if (augment_overlap(outs[i], ins[j])) return fail(S3R_ERR_INVALID, "augment: %s overlaps the input %s", outs[i].name, ins[j].name);
    }
    hipError_t e = s3r::launch_augment_pair(d, left, right, sample_ids, disp_left, disp_right, out_left, out_right, out_disp_left,
                                            out_disp_right, batch, height, width, scratch, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "augment launch");
    return S3R_OK;
}

// ---------------------------------------------------------------- surface point clouds (s3r_surface_points.hip)
namespace {

// the geometry's own checks, shared by the query and the call
int surface_shape(int batch, int depth, int height, int width) {
    if (batch <= 0) return fail(S3R_ERR_INVALID, "surface points: batch = %d must be positive", batch);
    if (depth < 1 || depth > 256 || height < 1 || height > 256 || width < 1 || width > 256)
        return fail(S3R_ERR_INVALID, "surface points: the grid's edges (%d, %d, %d) must be in 1..256", depth, height, width);
    const int64_t V = (int64_t)depth * height * width;
    if (V > (int64_t)1 << 21) return fail(S3R_ERR_INVALID, "surface points: depth * height * width = %lld must be at most 2^21", (long long)V);
    if (s3r::surface_points_scratch(batch, V) >= kMaxElems)
        return fail(S3R_ERR_INVALID, "surface points: the scratch of the call has 2^31 elements or more: split the batch");
    return S3R_OK;
}

}  // namespace

int64_t s3r_voxel_surface_points_scratch_elems(int batch, int depth, int height, int width) {
    int rc = surface_shape(batch, depth, height, width);
    if (rc) return rc;
    return s3r::surface_points_scratch(batch, (int64_t)depth * height * width);
}

int s3r_voxel_surface_points(const float* occupancy, float threshold, const int64_t* sample_ids, uint64_t seed, float* points,
                             int32_t* n_faces, int batch, int depth, int height, int width, int n_points, float* scratch,
                             int64_t scratch_elems, void* hip_stream) {
    int rc = surface_shape(batch, depth, height, width);
    if (rc) return rc;
    if (!occupancy || !sample_ids || !points) return fail(S3R_ERR_INVALID, "surface points: null occupancy, sample_ids or points");
    if (n_points <= 0) return fail(S3R_ERR_INVALID, "surface points: n_points = %d must be positive", n_points);
    if ((int64_t)batch * n_points * 3 >= kMaxElems)
        return fail(S3R_ERR_INVALID, "surface points: batch * n_points * 3 must be below 2^31: split the batch");
    if (!std::isfinite(threshold)) return fail(S3R_ERR_INVALID, "surface points: the threshold must be finite");
    const int64_t V = (int64_t)depth * height * width, need = s3r::surface_points_scratch(batch, V);
    if (!scratch || scratch_elems < need)
        return fail(S3R_ERR_INVALID, "surface points: needs %lld floats of scratch (s3r_voxel_surface_points_scratch_elems), got %lld",
                    (long long)need, scratch ? (long long)scratch_elems : 0ll);
    const AugSpan outs[3] = {{points, 12 * (int64_t)batch * n_points, "points"}, {n_faces, 4 * (int64_t)batch, "n_faces"},
                             {scratch, 4 * need, "scratch"}};
    const AugSpan ins[2] = {{occupancy, 4 * (int64_t)batch * V, "occupancy"}, {sample_ids, 8 * (int64_t)batch, "sample_ids"}};
    for (int i = 0; i < 3; ++i) {
        for (int j = i + 1; j < 3; ++j)
            if (augment_overlap(outs[i], outs[j])) return fail(S3R_ERR_INVALID, "surface points: %s and %s overlap", outs[i].name, outs[j].name);
        for (int j = 0; j < 2; ++j)
            if (augment_overlap(outs[i], ins[j])) return fail(S3R_ERR_INVALID, "surface points: %s overlaps the input %s", outs[i].name, ins[j].name);
    }
    hipError_t e = s3r::launch_surface_points(occupancy, threshold, sample_ids, seed, points, n_faces, batch, depth, height, width, n_points,
                                              scratch, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "surface points launch");
    return S3R_OK;
}

}  // extern "C"
