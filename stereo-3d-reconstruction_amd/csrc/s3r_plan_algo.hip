// Planner, unit 2 of 4 (s3r_host.h): which algorithm and launch form serve a descriptor (the library's policy), every size that
// follows (transformed operands, slabs, packed images, scratch) and the C-ABI size queries that answer from them — they live here
// because they ARE the plan.  Nothing here enqueues anything.
#include "s3r_host.h"

#include <cstdlib>

namespace s3rh {

int wino_mode() {
    static const int mode = getenv("S3R_WINO") ? atoi(getenv("S3R_WINO")) : 1;      // process-level: read once
    return mode;
}
int wino_r(const s3r_conv_desc*) { return 4; }

// ---------------------------------------------------------------- which forms a layer / descriptor has
bool wino_layer(const s3r_conv_desc* d) {
    return d->dtype != S3R_BF16 && d->op == S3R_OP_CONV && (d->ndim == 2 || d->ndim == 3) && d->k == 3 && d->stride == 1 &&
           d->pad == 1 && d->cin % s3r::wino_bk() == 0 && d->cout > 1 && d->in_size >= 4;
}
bool dwino_layer(const s3r_conv_desc* d) {
    return d->dtype != S3R_BF16 && deconv_fast(d) && d->cin % s3r::wino_bk() == 0 && d->in_size >= 4 && (d->in_size & 3) == 0;
}
bool dwino3_layer(const s3r_conv_desc* d) {
    return d->dtype != S3R_BF16 && deconv_fast(d) && d->cin % 16 == 0 && d->cout > 1 && s3r::dwino3_edge_ok(d->in_size);
}
bool dwino3_desc_ok(const s3r_conv_desc* d) {
    return dwino3_layer(d) && d->act < S3R_ACT_SIGMOID && d->in_halo == 1 && d->ksplit <= 1 && d->in_layout == S3R_LAYOUT_PLAIN &&
           d->out_layout == S3R_LAYOUT_PLAIN;
}
bool wino_desc_ok(const s3r_conv_desc* d) {
    if (!(wino_layer(d) || dwino_layer(d)) || d->act >= S3R_ACT_SIGMOID || d->in_halo != 1 || d->ksplit > 1 || dil_of(d) != 1) return false;
    // (a transposed layer may read its operand from, and write its consumer's to, the difference-tensor layout)
    if (d->out_layout != S3R_LAYOUT_PLAIN && !(d->out_layout == S3R_LAYOUT_DIFF && dwino_layer(d))) return false;
    return d->in_layout == S3R_LAYOUT_PLAIN || (d->in_layout == S3R_LAYOUT_WINO_H && wino_layer(d)) ||
           (d->in_layout == S3R_LAYOUT_DIFF && dwino_layer(d));
}
int wino2_ax(const s3r_conv_desc* d) {
    if (d->dtype == S3R_BF16 || d->op != S3R_OP_CONV || d->stride != 1 || d->cin % s3r::wino_bk() != 0 || d->cout <= 1) return -1;
    // (2D: the finish kernel stages a whole padded output plane in 64 KiB of LDS)
    if (d->ndim == 2) return d->k == 3 && d->pad == 1 && d->in_size >= 4 && d->in_size <= 124 ? 2 : -1;
    if (d->ndim != 3) return -1;
    if (d->k == 3 && d->pad == 1 && d->in_size >= 4) return 0;
    if (d->k == 4 && d->pad == 0 && d->in_size >= 5) return 1;
    return -1;
}
bool wino2_plane_fits(const s3r_conv_desc* d) {
    return wino2_ax(d) != 2 || d->out_layout == S3R_LAYOUT_WINO_HW || out_size(d) + 2 * d->out_halo <= kWino2PlaneEdge;
}
bool wino2_semi_fits(const s3r_conv_desc* d) {
    return wino2_ax(d) == 2 || (wino2_ax(d) == 0 && d->in_size <= kWino2SemiMaxEdge && out_size(d) + 2 * d->out_halo <= kWino2SemiEdge);
}
bool wino2_desc_ok(const s3r_conv_desc* d) {
    return wino2_ax(d) >= 0 && d->act < S3R_ACT_SIGMOID && dil_of(d) == 1 && d->in_halo == d->pad && d->ksplit <= 1 &&
           (d->in_layout == S3R_LAYOUT_PLAIN || (d->in_layout == S3R_LAYOUT_WINO_DH && wino2_ax(d) == 0 && d->in_size % 4 == 0) ||
            (d->in_layout == S3R_LAYOUT_WINO_HW && wino2_ax(d) == 2 && d->in_size % 4 == 0) ||
            (d->in_layout == S3R_LAYOUT_WINO_3D && wino2_ax(d) <= 1)) &&
           (d->out_layout == S3R_LAYOUT_PLAIN || (d->out_layout == S3R_LAYOUT_WINO_HW && wino2_ax(d) == 2 && d->in_size % 4 == 0) ||
            ((d->out_layout == S3R_LAYOUT_WINO_3D || d->out_layout == S3R_LAYOUT_DIFF) && wino2_ax(d) <= 1));
}
// the descriptor asks for the direct kernel
static bool forced_direct(const s3r_conv_desc* d) {
    return d->algo == S3R_ALGO_DIRECT || (d->algo == S3R_ALGO_AUTO && (d->tile >= 0 || d->ksplit >= 1));
}
// the producer wrote the two-axis kernel's plane sets
static bool wino2_planes_in(const s3r_conv_desc* d) {
    return d->in_layout == S3R_LAYOUT_WINO_DH || d->in_layout == S3R_LAYOUT_WINO_HW || d->in_layout == S3R_LAYOUT_WINO_3D;
}
// a layout only the two-axis kernel reads / writes (a consumer's operand may also come from the direct kernel's split-K finish)
static bool two_axis_io(const s3r_conv_desc* d) {
    if (wino2_planes_in(d) || d->out_layout == S3R_LAYOUT_WINO_HW) return true;
    return d->op == S3R_OP_CONV && (d->out_layout == S3R_LAYOUT_WINO_3D || d->out_layout == S3R_LAYOUT_DIFF) && wino2_ax(d) >= 0 &&
           !forced_direct(d);
}
int wino2_max_edge() {
    static const int e = getenv("S3R_WINO2_MAX_EDGE") ? atoi(getenv("S3R_WINO2_MAX_EDGE")) : 28;
    return e;
}

// ---------------------------------------------------------------- the algorithm a descriptor resolves to
// the two refusals resolve_algo gives on its WINOGRAD path (`forced`) and again on its AUTO path
static int two_axis_only_fail(bool forced) {
    return fail(S3R_ERR_INVALID, "a two-axis transformed input / output runs the two-axis kernel only%s",
                forced ? "" : ": algo AUTO / WINOGRAD, no direct tile / split-K override");
}
static int plane_edge_fail(const s3r_conv_desc* d, bool forced) {
    return fail(S3R_ERR_INVALID, "%sthe two-axis form of a Conv2d stages one padded output plane in 64 KiB of LDS: edge + 2 out_halo <= %d "
                "(got %d + 2 x %d)", forced ? "algo = WINOGRAD: " : "", kWino2PlaneEdge, out_size(d), d->out_halo);
}

int resolve_algo(const s3r_conv_desc* d, int* alg, int* form) {
    *alg = ALG_DIRECT;
    *form = -1;
    if (d->algo != S3R_ALGO_AUTO && d->algo != S3R_ALGO_DIRECT && d->algo != S3R_ALGO_WINOGRAD)
        return fail(S3R_ERR_INVALID, "unknown algo %d", d->algo);
    if (staged_layer(d) || d->act > S3R_ACT_SIGMOID || dil_of(d) != 1) {      // parameter-general layers: the direct kernel
        if (d->algo == S3R_ALGO_WINOGRAD) return fail(S3R_ERR_INVALID, "algo = WINOGRAD: a parameter-general layer (staged input, dilation, "
                                                      "LeakyReLU / ELU / Tanh) has no Winograd form");
        if (d->in_layout != S3R_LAYOUT_PLAIN || d->out_layout != S3R_LAYOUT_PLAIN)
            return fail(S3R_ERR_INVALID, "a parameter-general layer reads and writes plain layouts");
        return S3R_OK;
    }
    if (d->algo == S3R_ALGO_WINOGRAD && d->tile >= 6 && d->tile <= 8) {        // the three-axis form of a transposed layer
        if (!dwino3_desc_ok(d))
            return fail(S3R_ERR_INVALID, "algo = WINOGRAD, tile = 6: the three-axis form serves an fp32 ConvTranspose3d k4 s2 p1 over an edge of "
                        "8, 16 or 32 with cin %% 16 == 0 (in_halo = 1, plain layouts, no split-K, no sigmoid)");
        *alg = ALG_WINO3;
        *form = d->tile == 6 ? -1 : d->tile == 7 ? 1 : 0;      // 6: the library's launch form; 7: class-parallel; 8: serial (same bits)
        return S3R_OK;
    }
    if (d->algo == S3R_ALGO_WINOGRAD) {
        const bool one = wino_desc_ok(d), two = wino2_desc_ok(d);
        // tile: -1 the library's pick between the forms the layer has; 0, 1, 2 a launch form of the one-axis kernel; 3 the two-axis
        // algorithm (4: its class-parallel form, 5: its semi-fused form)
        if ((d->tile >= 3 && !two) || (d->tile >= 0 && d->tile <= 2 && !one) || (!one && !two) || d->tile > 5 ||
            (d->tile == 5 && wino2_ax(d) == 1))
            return fail(S3R_ERR_INVALID, "algo = WINOGRAD: this layer / descriptor has no such Winograd form (one-axis: fp32 Conv k3 s1 p1 "
                        "with cin %% %d == 0 and edge >= 4, or ConvTranspose3d k4 s2 p1 over an edge %% 4 == 0, in_halo = 1; two-axis "
                        "(tile = 3): Conv3d k3 s1 p1 / k4 s1 p0, in_halo = pad; plain layouts, no split-K, no sigmoid)", s3r::wino_bk());
        if (d->tile == 5 && !wino2_semi_fits(d))      // (tile 3 / -1 plan such a layer class-parallel: wino2_form_of)
            return fail(S3R_ERR_INVALID, "algo = WINOGRAD, tile = 5: the semi-fused form of a Conv3d stages four padded output slices in 64 KiB of "
                        "LDS: edge <= %d and edge + 2 out_halo <= %d (got %d + 2 x %d); the class-parallel form (tile = 4) has no such bound",
                        kWino2SemiMaxEdge, kWino2SemiEdge, out_size(d), d->out_halo);
        const bool two_io = two_axis_io(d);
        if (two_io && !(two && (d->tile < 0 || d->tile >= 3))) return two_axis_only_fail(true);
        if (d->tile >= 3 || !one || two_io ||
            (d->tile < 0 && two && d->in_layout == S3R_LAYOUT_PLAIN && d->in_size <= wino2_max_edge() && wino2_plane_fits(d))) {
            if (!wino2_plane_fits(d)) return plane_edge_fail(d, true);
            *alg = ALG_WINO2;
            *form = d->tile >= 4 ? d->tile - 4 : -1;
        } else { *alg = ALG_WINO; *form = d->tile; }
        return S3R_OK;
    }
    if (two_axis_io(d)) {
        // only the two-axis kernel reads / writes the 36 plane sets
        if (d->algo == S3R_ALGO_DIRECT || !wino2_desc_ok(d) || d->tile >= 0) return two_axis_only_fail(false);
        if (!wino2_plane_fits(d)) return plane_edge_fail(d, false);
        *alg = ALG_WINO2;
        return S3R_OK;
    }
    if (d->in_layout == S3R_LAYOUT_WINO_H) {             // only the one-axis Winograd kernel reads the transformed planes
        if (d->algo == S3R_ALGO_DIRECT || !wino_desc_ok(d) || d->tile >= 0)
            return fail(S3R_ERR_INVALID, "a Winograd-transformed input runs the Winograd kernel only: algo AUTO / WINOGRAD, no direct tile / "
                        "split-K override, a plain output");
        *alg = ALG_WINO;
        return S3R_OK;
    }
    if (d->in_layout == S3R_LAYOUT_DIFF || d->out_layout == S3R_LAYOUT_DIFF) {      // (a transposed layer here: a convolution writing it is two_axis_io)
        if (d->op != S3R_OP_DECONV || forced_direct(d) || !wino_desc_ok(d))
            return fail(S3R_ERR_INVALID, "the difference-tensor layout is read / written by the Winograd form of a ConvTranspose3d k4 s2 p1 (algo AUTO / "
                        "WINOGRAD, no direct tile / split-K override), or written by a two-axis Conv3d");
        *alg = ALG_WINO;
        return S3R_OK;
    }
    if (d->in_layout == S3R_LAYOUT_WINO_3D || (d->out_layout == S3R_LAYOUT_WINO_3D && d->op != S3R_OP_CONV))
        return fail(S3R_ERR_INVALID, "the general two-axis layout is read by the two-axis kernel and written by a convolution only");
    if (d->algo == S3R_ALGO_DIRECT || d->tile >= 0 || d->ksplit >= 1 || wino_mode() <= 0) return S3R_OK;
    if (d->out_layout == S3R_LAYOUT_WINO_3D) return S3R_OK;      // (a convolution without the two-axis form: its split-K finish writes the planes)
    if (wino2_desc_ok(d) && d->in_size <= wino2_max_edge() && wino2_plane_fits(d)) *alg = ALG_WINO2;
    // transposed layers with an edge >= 16: the three-axis form (27 / 64 of the multiplications).  r05, d3 (16^3 -> 32^3, fused head)
    // inside the forward: 0.694 -> 0.622 ms at B = 32, -4 % at B = 8 / 16, equal at 4, +5 % at B = 1 / 2 (serial form only: 64
    // workgroups); at edge 8 (d2) its one round of long workgroups loses to the two-axis form's dual launch (0.438 vs 0.380 ms)
    else if (d->op == S3R_OP_DECONV && dwino3_desc_ok(d) && d->in_size >= 16) *alg = ALG_WINO3;
    else if (wino_desc_ok(d)) *alg = ALG_WINO;
    return S3R_OK;
}
bool resolves_to_wino(const s3r_conv_desc* d) {
    int a, f;
    return resolve_algo(d, &a, &f) == S3R_OK && a != ALG_DIRECT;
}

// ---------------------------------------------------------------- transformed operands and the samples one call takes
int64_t wino2_operand_elems(int ax, int C, int out, int wp, int64_t nb) {
    const int m = s3r::wino2_outputs(ax), sg = (out + m - 1) / m;
    if (ax == 2) return (int64_t)s3r::wino2_classes(ax) * C * s3r::wino2_npad(nb * sg * sg);
    return (int64_t)s3r::wino2_classes(ax) * C * sg * sg * wp * nb;
}
int64_t operand_elems(const s3r_conv_desc* c, int layout, int64_t nb) {
    if (layout != S3R_LAYOUT_WINO_H) return wino2_operand_elems(wino2_ax(c), c->cin, out_size(c), c->in_size + 2 * c->in_halo, nb);
    const int R = wino_r(c);
    const int64_t dp = c->ndim == 3 ? c->in_size + 2 : 1, hq = (c->in_size + R - 1) / R, wp = c->in_size + 2;
    return (R + 2) * nb * c->cin * dp * hq * wp;
}
int call_samples(int64_t per_sample_elems, int batch) {
    const int64_t m = per_sample_elems > 0 ? (((int64_t)1 << 31) - 1) / (4 * per_sample_elems) : 0;
    return (int)(m < batch ? m : batch);
}
Wino2Geo wino2_geo(const s3r_conv_desc* d) {
    Wino2Geo w;
    w.ax = wino2_ax(d);
    w.m = s3r::wino2_outputs(w.ax);
    w.ncls = s3r::wino2_classes(w.ax);
    w.out = out_size(d);
    w.sg = (w.out + w.m - 1) / w.m;                       // groups per axis
    w.wp = d->in_size + 2 * d->in_halo;
    w.kw = w.ax == 2 ? 1 : d->k;                          // column taps left to the class kernel
    w.w_elems = (int64_t)w.ncls * w.kw * d->cin * cout_pad(d->cout);
    // ax 2: the positions of a sub-batch are rounded up to a GEMM tile as a whole: v_sample is the bound used to size a sub-batch
    w.v_sample = w.ax == 2 ? (int64_t)w.ncls * d->cin * (w.sg * w.sg + 64) : operand_elems(d, S3R_LAYOUT_WINO_3D, 1);
    w.pos_sample = w.ax == 2 ? (int64_t)w.sg * w.sg : (int64_t)w.sg * w.sg * w.out;
    w.bmax = call_samples(w.v_sample, d->batch);
    w.n = 0;
    return w;
}
int wino_bmax(const s3r_conv_desc* d) { return call_samples(operand_elems(d, S3R_LAYOUT_WINO_H, 1), d->batch); }
bool fits_one_call(const s3r_conv_desc* d, int alg) { return (alg == ALG_WINO2 ? wino2_geo(d).bmax : wino_bmax(d)) >= d->batch; }

// a batch that goes through in sub-batches of bmax has at most two different sub-batch sizes: the larger slab of the two
template <class SlabOf> static int64_t max_slab_over_sub_batches(int batch, int bmax, SlabOf slab_of) {
    const int64_t first = slab_of(sub_batch(batch, 0, bmax)), last = batch > bmax && batch % bmax ? slab_of(batch % bmax) : 0;
    return first > last ? first : last;
}

// ---------------------------------------------------------------- packed images
int64_t wino_w_elems(const s3r_conv_desc* d) {
    return (wino_r(d) + 2) * ipow(3, d->ndim - 1) * d->cin * (int64_t)cout_pad(d->cout);
}
int64_t dwino_w_elems(const s3r_conv_desc* d) { return 72 * 2 * (int64_t)d->cin * cout_pad(d->cout); }
PackedLayout packed_layout(const s3r_conv_desc* d, const Geo& g) {
    PackedLayout at = {0, -1, -1, -1, -1, 0};
    int64_t end = (d->op == S3R_OP_DECONV ? 64 : ipow(d->k, g.nd)) * d->cin * cout_pad(d->cout);
    if (wino_layer(d)) { at.wino = end; end += wino_w_elems(d); }
    if (wino2_ax(d) >= 0) { at.wino2 = end; end += wino2_geo(d).w_elems; }
    if (dwino_layer(d)) { at.dwino = end; end += dwino_w_elems(d); }
    if (dwino3_layer(d)) { at.dwino3 = end; end += s3r::dwino3_w_elems(d->cin, d->cout); }
    at.total = end; return at;
}

// ---------------------------------------------------------------- scratch of the Winograd forms
bool dwino_materialise(const s3r_conv_desc* d) {
    static const int forced = getenv("S3R_DWINO_MAT") ? atoi(getenv("S3R_DWINO_MAT")) : -1;      // A/B switch, read once
    if (forced >= 0) return forced != 0;
    return 4 * 4 * (int64_t)d->batch * d->cin * ipow(d->in_size + 2, 3) <= (int64_t)192 << 20;
}
int64_t dwino_d_elems(const s3r_conv_desc* d) {
    return (dwino_materialise(d) ? 3 : 1) * (int64_t)d->batch * d->cin * ipow(d->in_size + 2, 3);
}
int wino_kind(const s3r_conv_desc* d) { return d->op == S3R_OP_DECONV ? 2 : 1; }
int wino_kcls(const s3r_conv_desc* d) {
    return d->cin * (d->op == S3R_OP_DECONV ? 2 : (d->ndim == 3 ? 9 : 3));
}
int64_t wino_positions(const s3r_conv_desc* d, int nb) {
    const int n = d->in_size;
    if (d->op == S3R_OP_DECONV) return (int64_t)nb * (n / 2) * (n / 2) * n;
    const int R = wino_r(d);
    return (int64_t)nb * (d->ndim == 3 ? n : 1) * ((n + R - 1) / R) * n;
}
WinoNeed wino_need(const s3r_conv_desc* d, int form, bool head) {
    WinoNeed w = {0, 0, 0};
    if (d->batch <= 0) return w;
    const int kind = wino_kind(d);
    const auto slab_of = [&](int nb, bool with_head) {
        const int nt = (int)wino_positions(d, nb);
        return s3r::wino_slab_elems(kind, d->cout, nt, s3r::wino_plan(kind, d->cout, wino_kcls(d), nt, with_head, form < 0 ? 1 : form));
    };
    if (d->op == S3R_OP_DECONV) {
        if (d->in_layout != S3R_LAYOUT_DIFF) w.v = dwino_d_elems(d);
        w.slab = slab_of(d->batch, head);
    } else {
        const int bmax = wino_bmax(d);
        if (bmax <= 0) return w;
        if (d->in_layout != S3R_LAYOUT_WINO_H) w.v = operand_elems(d, S3R_LAYOUT_WINO_H, bmax);
        w.slab = max_slab_over_sub_batches(d->batch, bmax, [&](int nb) { return slab_of(nb, false); });
    }
    w.v = align_up(w.v, 256);
    w.total = w.v + w.slab;
    return w;
}
double wino_exec_flops(const s3r_conv_desc* d, const Geo& g) {
    if (d->op == S3R_OP_DECONV) return g.flops * 0.5625;
    const int R = wino_r(d);
    const double taps = (d->ndim == 3 ? 3.0 : 1.0) * 3.0 * (R + 2);
    return 2.0 * (double)wino_positions(d, d->batch) * d->cout * d->cin * taps;
}

int wino2_form_of(const s3r_conv_desc* d, int ntotal, int forced) {
    if (forced < 0 && !wino2_semi_fits(d)) forced = 0;
    return s3r::wino2_form(wino2_ax(d), d->cout, ntotal, forced);
}
WinoNeed wino2_need(const s3r_conv_desc* d, int form) {
    WinoNeed w = {0, 0, 0};
    const Wino2Geo g2 = wino2_geo(d);
    if (d->batch <= 0 || g2.bmax <= 0) return w;
    if (!wino2_planes_in(d)) w.v = align_up(operand_elems(d, g2.ax == 2 ? S3R_LAYOUT_WINO_HW : S3R_LAYOUT_WINO_3D, g2.bmax), 256);
    w.slab = max_slab_over_sub_batches(d->batch, g2.bmax, [&](int nb) {
        const int nt = (int)(g2.pos_sample * nb);
        // (form < 0: sized for the class-parallel form — 36 / 25 class slabs against the semi-fused form's 24)
        return s3r::wino2_slab_elems(g2.ax, d->cout, nt, form < 0 ? 0 : wino2_form_of(d, nt, form));
    });
    w.total = w.v + w.slab;
    return w;
}
double wino2_exec_flops(const s3r_conv_desc* d) {
    const Wino2Geo g2 = wino2_geo(d);
    return 2.0 * (double)g2.pos_sample * d->batch * g2.ncls * d->cout * d->cin * g2.kw;
}

Dwino3Need dwino3_need(const s3r_conv_desc* d, int form) {
    Dwino3Need n;
    n.diff = align_up(3 * (int64_t)d->batch * d->cin * ipow(d->in_size + 2, 3), 256);
    const int ntotal = d->batch * (int)ipow(d->in_size / 2, 3);
    n.split = s3r::dwino3_split(d->cout, ntotal, form);
    // (sized for the class-parallel form whenever the LIBRARY picks the launch form: ADVICE r05, as wino_need)
    n.total = n.diff + ((n.split || form < 0) ? align_up(s3r::dwino3_slab_elems(d->cout, ntotal), 256) : 0);
    return n;
}

// which transformed layout (if any) the producer of layer `d`'s input may write instead of the plain halo-padded tensor
static int wino_input_layout(const s3r_conv_desc* d, int64_t* elems) {
    *elems = 0;
    s3r_conv_desc t = *d;
    t.in_layout = S3R_LAYOUT_PLAIN;
    int alg, form, lay = S3R_LAYOUT_PLAIN;
    if (resolve_algo(&t, &alg, &form) != S3R_OK || t.op != S3R_OP_CONV) return S3R_LAYOUT_PLAIN;
    if (alg == ALG_WINO && t.in_size % wino_r(&t) == 0) lay = S3R_LAYOUT_WINO_H;
    else if (alg == ALG_WINO2 && wino2_ax(&t) == 0 && t.in_size % 4 == 0) lay = S3R_LAYOUT_WINO_DH;
    else if (alg == ALG_WINO2 && wino2_ax(&t) == 2 && t.in_size % 4 == 0) lay = S3R_LAYOUT_WINO_HW;
    if (lay == S3R_LAYOUT_PLAIN || !fits_one_call(&t, alg)) return S3R_LAYOUT_PLAIN;
    *elems = operand_elems(&t, lay, t.batch);
    return lay;
}

}  // namespace s3rh

using namespace s3rh;

extern "C" {

int s3r_conv_packed_elems(const s3r_conv_desc* d, int64_t* elems) {
    Geo g; Route r;
    int rc = geometry(d, &g);
    if (rc) return rc;
    if ((rc = route(d, &r))) return rc;
    if (!elems) return fail(S3R_ERR_INVALID, "null output");
    switch (r) {
        case R_STEM: *elems = 27 * 32; break;
        case R_HEAD: *elems = d->cin; break;
        case R_LINEAR: *elems = g.w_elems; break;
        case R_MFMA: {
            if (tclass_layer(d)) { *elems = tclass_w_elems(d); break; }
            if (im2col_layer(d)) { *elems = (int64_t)staged_geo(d).cin_pad * cout_pad(d->cout); break; }
            if (staged_layer(d)) { *elems = ipow(d->k, g.nd) * staged_geo(d).cin_pad * cout_pad(d->cout); break; }
            const int64_t taps = d->op == S3R_OP_DECONV ? 64 : ipow(d->k, g.nd);
            if (d->dtype == S3R_BF16) *elems = (taps * d->cin * cout_pad_h(d->cout) + 1) / 2;   // bf16, in float units
            else *elems = packed_layout(d, g).total;
            break;
        }
    }
    return S3R_OK;
}

int64_t s3r_conv_scratch_elems(const s3r_conv_desc* d) {
    Geo g; Route r;
    int rc = geometry(d, &g);
    if (rc) return rc;
    if ((rc = route(d, &r))) return rc;
    if (r == R_LINEAR) return s3r::linear_scratch_elems(d->batch, d->cin, d->cout);
    if (r != R_MFMA) return 0;
    if (d->dtype == S3R_BF16) {
        s3r::ConvParamsH ph;
        LaunchH Lh;
        if ((rc = plan_direct_h(d, g, &ph, &Lh))) return rc;
        return s3r::conv_bf16_scratch_elems(ph, Lh.tm);
    }
    int alg, form;
    if ((rc = resolve_algo(d, &alg, &form))) return rc;
    if (tclass_direct(d)) return 0;                                                // (reads the producer's halo: nothing staged)
    if (staged_layer(d)) return align_up(staged_geo(d).elems, 256);               // the staged copy (no split-K behind it)
    if (alg == ALG_WINO3) return dwino3_need(d, form).total;      // Dh, Dd, Ddh (+ the class-parallel form's slabs)
    if (alg == ALG_WINO) return wino_need(d, form, false).total;
    if (alg == ALG_WINO2) return wino2_need(d, form).total;
    s3r::ConvParams p;
    Launch L;
    if ((rc = plan_direct(d, g, &p, &L))) return rc;
    return s3r::conv_scratch_elems(p, L.cfg);
}

int64_t s3r_conv_wino_input_elems(const s3r_conv_desc* d) {
    int64_t elems;
    return d ? (wino_input_layout(d, &elems), elems) : fail(S3R_ERR_INVALID, "null descriptor");
}

int s3r_conv_wino_input_layout(const s3r_conv_desc* d) {
    int64_t elems;
    return d ? wino_input_layout(d, &elems) : fail(S3R_ERR_INVALID, "null descriptor");
}

}  // extern "C"
