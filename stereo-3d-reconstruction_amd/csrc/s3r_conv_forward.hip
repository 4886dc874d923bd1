// The forward convolution of libs3r_hip.so's C-ABI (include/s3r.h).  Top to bottom: what every forward convolution shares (ConvCall,
// the scratch / launch / activation helpers), ONE runner per kernel path (run_*), the dispatcher over them (conv_forward_impl:
// validation and a switch, no launch), the fused conv + head launch and the chain walker; then ONE extern "C" block of the entry
// points that are thin fronts for them.  Planning lives in the four s3r_plan_*.hip units (geometry; kernel policy, sizes and the packed
// image's layout; parameter blocks; the arena), the profiler in s3r_prof.hip, every other entry point in s3r_api_layers.hip /
// s3r_api_tasks.hip.  Host code only.
#include "s3r_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>

using namespace s3rh;

namespace {

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

int check_stem_input(const s3r_conv_desc* d, const void* x, const void* x2, int nsplit) {
    if (x2 && (nsplit <= 0 || nsplit >= d->batch)) return fail(S3R_ERR_INVALID, "split %d outside (0, batch=%d)", nsplit, d->batch);
    return check_renders_aligned(x, x2);
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

// a sub-batch (s3r_host.h, sub_batch): samples [b0, b0 + nb) of the call, x_sample floats of (staged / transformed) input each
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
    int rc = in_place ? S3R_OK : check_scratch(c, align_up(sg.elems, 256), "a parameter-general layer stages its input in");
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
    if (bmax <= 0 || (pre && !fits_one_call(d, ALG_WINO)))
        return fail(S3R_ERR_INVALID, "a Winograd-transformed input takes at most %d samples per call here "
                    "(s3r_conv_wino_input_elems)", bmax);
    const WinoNeed need = wino_need(d, form, false);
    int rc = need.total > 0 ? check_scratch(c, need.total, "the Winograd form of this layer needs") : S3R_OK;
    if (rc) return rc;
    const int64_t v_sample = operand_elems(d, S3R_LAYOUT_WINO_H, 1), x_sample = g.x_elems / d->batch;
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
    if (g2.bmax <= 0 || ((pre || to_v || p.out_mode) && !fits_one_call(d, ALG_WINO2)))
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
            s3r::AuxScope aux(c.s, 4.0 * ((double)nb * x_sample + (double)operand_elems(d, g2.ax == 2 ? S3R_LAYOUT_WINO_HW : S3R_LAYOUT_WINO_3D, nb)));
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
    if (!c.x || !c.w || !c.y) return null_tensor();
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
    if (!x || !y) return null_tensor();
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

int s3r_decoder_forward(const s3r_layer* layers, int n_layers, const void* volume, float* occupancy, float* ws,
                        int64_t ws_elems, int ws_fresh, void* stream) {
    if (!layers || n_layers <= 0) return fail(S3R_ERR_INVALID, "empty decoder");
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].desc.op == S3R_OP_LINEAR || layers[i].desc.ndim != 3)
            return fail(S3R_ERR_INVALID, "decoder layer %d is not a 3D (transposed) convolution", i);
    return s3r_chain_forward(layers, n_layers, volume, occupancy, ws, ws_elems, ws_fresh, stream);
}

}  // extern "C"
