// Planner, unit 3 of 4 (s3r_host.h): the kernel-side parameter blocks of the direct kernels (fp32, bf16, and the staged /
// residue-class / depth-to-space views of a parameter-general layer) and their launch forms.  Nothing here enqueues anything.
#include "s3r_host.h"
#include "s3r_bf16.h"      // the bf16 tile-code table

#include <cstring>

namespace s3rh {

// positions, taps and input origin of a convolution / the tuned transposed layer (8 parity classes of 2 x 2 x 2 taps), fp32 and bf16
// alike; ws: the innermost input stride (1, bf16 channels-last: Cin)
template <class Params> static void set_positions(Params& p, const s3r_conv_desc* d, const Geo& g, int ws) {
    const bool is3 = d->ndim == 3;
    if (d->op == S3R_OP_DECONV) {
        p.transposed = 1;
        p.Nd = g.in; p.Nh = g.in; p.Nw = g.in;
        p.kd = p.kh = p.kw = 2; p.T = 8;
        p.stride = 1;
        p.x_org = d->in_halo * (p.x_ds + p.x_hs + ws);
    } else {
        p.transposed = 0;
        p.Nd = is3 ? g.out : 1; p.Nh = g.out; p.Nw = g.out;
        p.kd = is3 ? d->k : 1; p.kh = d->k; p.kw = d->k; p.T = p.kd * p.kh * p.kw;
        p.stride = d->stride;
        p.x_org = (d->in_halo - d->pad) * (p.x_ds + p.x_hs + ws);
    }
    p.Ntotal = p.B * p.Nd * p.Nh * p.Nw;
}

s3r::ConvParamsH make_params_h(const s3r_conv_desc* d, const Geo& g) {
    s3r::ConvParamsH p;
    memset(&p, 0, sizeof(p));
    const bool is3 = d->ndim == 3;
    p.B = d->batch; p.Cin = d->cin; p.Cout = d->cout; p.CoutPad = cout_pad_h(d->cout);
    p.act = d->act;
    p.x_ws = d->cin; p.x_hs = g.in_p * d->cin; p.x_ds = is3 ? g.in_p * g.in_p * d->cin : 0;
    p.x_bs = (int)ipow(g.in_p, g.nd) * d->cin;
    p.y_ws = d->cout; p.y_hs = g.out_p * d->cout; p.y_ds = is3 ? g.out_p * g.out_p * d->cout : 0;
    p.y_bs = (int)ipow(g.out_p, g.nd) * d->cout;
    p.y_org = d->out_halo * (p.y_ds + p.y_hs + p.y_ws);
    p.x_bytes = (unsigned)(g.x_elems * 2);
    set_positions(p, d, g, p.x_ws);
    p.dS = s3r::FastDiv((unsigned)(p.Nd * p.Nh * p.Nw));
    p.dHW = s3r::FastDiv((unsigned)(p.Nh * p.Nw));
    p.dW = s3r::FastDiv((unsigned)p.Nw);
    p.dDH = s3r::FastDiv((unsigned)(p.Nd * p.Nh));
    p.dH = s3r::FastDiv((unsigned)p.Nh);
    p.ksplit = 1;
    return p;
}

int resolve_launch_h(const s3r_conv_desc* d, s3r::ConvParamsH* p, LaunchH* L) {
    const int chunks = d->cin / 32;
    if (d->ksplit < 0 || (d->ksplit > 0 && chunks % d->ksplit != 0))
        return fail(S3R_ERR_INVALID, "ksplit=%d must divide cin/32=%d", d->ksplit, chunks);
    L->ksplit = d->ksplit > 0 ? d->ksplit : s3r::conv_bf16_pick_ksplit(*p);
    p->ksplit = L->ksplit;
    if (d->tile >= 0 && !s3r::bf16_tile(d->tile))
        return fail(S3R_ERR_INVALID, "bf16 path: tile must be -1 (auto), 1, 2, 4 (x128 positions, per-tap gather), 3 (128 x 128 couts), 5, 6 "
                    "(x128 positions = 1, 2, plane-reuse gather) or 9, 10 (row-reuse gather); per-tap / plane + 16 = "
                    "32-channel K tiles; 40 (row-persistent e2)");
    L->tm = d->tile >= 0 ? d->tile : s3r::conv_bf16_pick_tm(*p);
    return S3R_OK;
}

s3r::ConvParams make_params(const s3r_conv_desc* d, const Geo& g) {
    s3r::ConvParams p;
    memset(&p, 0, sizeof(p));
    const bool is3 = d->ndim == 3;
    p.B = d->batch; p.Cin = d->cin; p.Cout = d->cout; p.CoutPad = cout_pad(d->cout);
    p.act = d->act;
    // strides of the padded buffers; a 2D layer has no depth axis (x_ds = y_ds = 0, Nd = kd = 1)
    p.x_hs = g.in_p; p.x_ds = is3 ? g.in_p * g.in_p : 0; p.x_cs = (int)ipow(g.in_p, g.nd);
    p.y_hs = g.out_p; p.y_ds = is3 ? g.out_p * g.out_p : 0; p.y_cs = (int)ipow(g.out_p, g.nd);
    p.y_org = d->out_halo * (p.y_ds + p.y_hs + 1);
    p.y_bs = d->cout * p.y_cs;
    p.x_bytes = (unsigned)(g.x_elems * 4);
    p.y_bytes = (unsigned)(g.y_elems * 4);
    set_positions(p, d, g, 1);
    p.dil = dil_of(d);
    if (leaky_fused(d)) { p.act = S3R_ACT_RELU; p.slope = d->act_param; }      // max(t, slope t) in the direct kernel's epilogue
    else if (p.act > S3R_ACT_SIGMOID) p.act = S3R_ACT_NONE;     // (ELU / Tanh, LeakyReLU with a slope outside [0, 1]: launch_act behind the convolution)
    set_divs(p);
    p.ksplit = 1;
    return p;
}

// the layer's parameter block re-aimed at the staged tensor `sg` (CinPad channels, its own strides; never the transposed form)
static void aim_at_staged(s3r::ConvParams& p, const StagedGeo& sg, int nd) {
    p.Cin = sg.cin_pad;
    p.transposed = 0;
    p.x_hs = sg.sp; p.x_ds = nd == 3 ? sg.sp * sg.sp : 0; p.x_cs = (int)ipow(sg.sp, nd);
    p.x_bytes = (unsigned)(sg.elems * 4);
}
// ... and at its own positions: Nd x Nh x Nw per sample
static void set_counts(s3r::ConvParams& p, int Nd, int Nh, int Nw) {
    p.Nd = Nd; p.Nh = Nh; p.Nw = Nw;
    p.Ntotal = p.B * p.Nd * p.Nh * p.Nw;
    set_divs(p);
}

s3r::ConvParams make_params_staged(const s3r_conv_desc* d, const Geo& g) {
    s3r::ConvParams p = make_params(d, g);
    const bool is3 = d->ndim == 3;
    aim_at_staged(p, staged_geo(d), g.nd);
    p.x_org = 0;
    if (im2col_layer(d)) {                        // the unfolded tensor: a 1 x 1 GEMM, one position per output
        p.kd = p.kh = p.kw = 1; p.T = 1;
        p.stride = 1; p.dil = 1;
    } else {
        p.kd = is3 ? d->k : 1; p.kh = d->k; p.kw = d->k; p.T = p.kd * p.kh * p.kw;
        p.stride = d->op == S3R_OP_DECONV ? 1 : d->stride;
    }
    set_counts(p, is3 ? g.out : 1, g.out, g.out);
    return p;
}

s3r::ConvParams make_params_tshuf(const s3r_conv_desc* d, const Geo& g) {
    const bool is3 = d->ndim == 3;
    const StagedGeo sg = tclass_input_geo(d);     // (k == stride, pad 0: the classes read no halo; staged only to pad the channels)
    const int s = d->stride, sc = (int)ipow(s, d->ndim);
    s3r::ConvParams p = make_params(d, g);
    aim_at_staged(p, sg, g.nd);
    p.Cout = d->cout * sc;                        // GEMM rows: (cout, tap); y_bs / y_cs stay the real output's
    p.CoutPad = cout_pad(p.Cout);
    p.x_org = sg.pe * (p.x_ds + p.x_hs + 1);
    p.kd = p.kh = p.kw = 1; p.T = 1;
    p.stride = 1; p.dil = 1;
    p.y_step = s;
    p.shuf_s = s; p.shuf_nd = d->ndim;
    p.dSC = s3r::FastDiv((unsigned)sc);
    p.dS1 = s3r::FastDiv((unsigned)s);
    set_counts(p, is3 ? d->in_size : 1, d->in_size, d->in_size);
    p.ksplit = 1;
    return p;
}

bool make_params_tclass(const s3r_conv_desc* d, const Geo& g, int rd, int rh, int rw, s3r::ConvParams* q, int64_t* w_off, double* macs) {
    const bool is3 = d->ndim == 3;
    const StagedGeo sg = tclass_input_geo(d);
    const int s = d->stride, h = sg.pe;
    const TClassAxis ad = is3 ? tclass_axis(d, rd) : TClassAxis{1, 1, 0, 1}, ah = tclass_axis(d, rh), aw = tclass_axis(d, rw);
    // slab offset: classes in (rd, rh, rw) order, each prod(ke) taps
    int64_t taps_before = 0;
    {
        int64_t sum_ke = 0;
        for (int r = 0; r < s; ++r) sum_ke += tclass_axis(d, r).ke;
        int64_t kd_before = 0, kh_before = 0, kw_before = 0;
        for (int r = 0; r < rd; ++r) kd_before += tclass_axis(d, r).ke;
        for (int r = 0; r < rh; ++r) kh_before += tclass_axis(d, r).ke;
        for (int r = 0; r < rw; ++r) kw_before += tclass_axis(d, r).ke;
        // classes before (rd, rh, rw): all (rd' < rd, *, *), then (rd, rh' < rh, *), then (rd, rh, rw' < rw)
        taps_before = (is3 ? kd_before * sum_ke * sum_ke : 0) + (int64_t)ad.ke * kh_before * sum_ke + (int64_t)ad.ke * ah.ke * kw_before;
    }
    *w_off = taps_before * sg.cin_pad * cout_pad(d->cout);
    if (ad.nq <= 0 || ah.nq <= 0 || aw.nq <= 0) return false;
    s3r::ConvParams p = make_params(d, g);
    aim_at_staged(p, sg, g.nd);
    p.kd = is3 ? ad.ke : 1; p.kh = ah.ke; p.kw = aw.ke; p.T = p.kd * p.kh * p.kw;
    p.stride = 1; p.dil = 1;
    // position u of an axis is q = qmin + u: it reads staged indices h + q - (ke - 1) .. h + q and writes output s q + r - pad
    p.x_org = (is3 ? (h + ad.qmin - (ad.ke - 1)) * p.x_ds : 0) + (h + ah.qmin - (ah.ke - 1)) * p.x_hs + (h + aw.qmin - (aw.ke - 1));
    p.y_step = s;
    p.y_org += (is3 ? (s * ad.qmin + rd - d->pad) * p.y_ds : 0) + (s * ah.qmin + rh - d->pad) * p.y_hs + (s * aw.qmin + rw - d->pad);
    set_counts(p, is3 ? ad.nq : 1, ah.nq, aw.nq);
    p.ksplit = 1;
    *macs = (double)p.Ntotal * p.T * (double)sg.cin_pad * d->cout;
    *q = p;
    return true;
}

int resolve_launch(const s3r_conv_desc* d, s3r::ConvParams* p, Launch* L) {
    const int chunks = d->cin / 16;
    if (d->ksplit < 0 || (d->ksplit > 0 && chunks % d->ksplit != 0))
        return fail(S3R_ERR_INVALID, "ksplit=%d must divide cin/16=%d", d->ksplit, chunks);
    L->ksplit = d->ksplit > 0 ? d->ksplit : s3r::conv_pick_ksplit(*p, 0);
    p->ksplit = L->ksplit;
    const int code = d->tile >= 0 ? d->tile : 15;
    L->cfg = code & 15;
    L->vec = code >> 4;
    if (L->cfg != 15 && L->cfg >= s3r::conv_num_tiles()) return fail(S3R_ERR_INVALID, "unknown tile configuration %d", L->cfg);
    if (L->cfg == 15) L->cfg = s3r::conv_pick_tile(*p);
    // a forced tile wider than 256 gathers of the width the geometry allows has no kernel: refuse it here, not as a launch error
    const int vmax = s3r::conv_pick_vec(*p);
    const int vec = (L->vec == 1 || L->vec == 4) && L->vec <= vmax ? L->vec : vmax;
    int bm, bn;
    s3r::conv_tile_dims(L->cfg, &bm, &bn);
    if (bn > 256 * vec)
        return fail(S3R_ERR_INVALID, "tile configuration %d (%d positions) needs the 16-byte gather: rows of a multiple of 4 positions, "
                    "stride 1", L->cfg, bn);
    return S3R_OK;
}

int plan_direct(const s3r_conv_desc* d, const Geo& g, s3r::ConvParams* p, Launch* L) {
    *p = make_params(d, g);
    return resolve_launch(d, p, L);
}
int plan_direct_h(const s3r_conv_desc* d, const Geo& g, s3r::ConvParamsH* p, LaunchH* L) {
    *p = make_params_h(d, g);
    return resolve_launch_h(d, p, L);
}
int direct_ksplit(const s3r_conv_desc* d, const Geo& g, int* ksplit) {
    s3r::ConvParams p; Launch L = {0, 0, 0};
    s3r::ConvParamsH ph; LaunchH Lh = {0, 0};
    const int rc = d->dtype == S3R_BF16 ? plan_direct_h(d, g, &ph, &Lh) : plan_direct(d, g, &p, &L);
    *ksplit = d->dtype == S3R_BF16 ? Lh.ksplit : L.ksplit;
    return rc;
}

}  // namespace s3rh
