// Planner, unit 1 of 4 (s3r_host.h): error plumbing, the shape predicates, staged / residue-class / unfolded geometry, descriptor
// validation and layer geometry, which kernel serves a shape and the halo it reads.  Nothing here enqueues anything.
#include "s3r_host.h"

#include <cstdarg>
#include <cstdio>

namespace s3rh {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) { return fail(S3R_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
const char* last_error() { return g_err; }

int64_t ipow(int64_t b, int e) {
    int64_t r = 1;
    while (e-- > 0) r *= b;
    return r;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
int cout_pad(int cout) { return (cout + 127) / 128 * 128; }
int cout_pad_h(int cout) { return (cout + 63) / 64 * 64; }
int cin_pad16(int k_rows) { return (k_rows + 15) / 16 * 16; }

int dil_of(const s3r_conv_desc* d) { return d->dilation > 0 ? d->dilation : 1; }

int out_size(const s3r_conv_desc* d) {
    if (d->op == S3R_OP_LINEAR) return 1;
    if (d->op == S3R_OP_DECONV) return (d->in_size - 1) * d->stride - 2 * d->pad + dil_of(d) * (d->k - 1) + d->out_pad + 1;
    const int span = d->in_size + 2 * d->pad - dil_of(d) * (d->k - 1) - 1;
    return span < 0 ? 0 : span / d->stride + 1;
}

// ---------------------------------------------------------------- shape predicates
bool deconv_fast(const s3r_conv_desc* d) {
    return d->op == S3R_OP_DECONV && d->ndim == 3 && d->k == 4 && d->stride == 2 && d->pad == 1 && dil_of(d) == 1 && d->out_pad == 0;
}
static bool stem_shape(const s3r_conv_desc* d) {
    return d->op == S3R_OP_CONV && d->ndim == 2 && d->cin == 3 && d->cout == 32 && d->k == 3 && d->stride == 2 && d->pad == 1 &&
           d->act == S3R_ACT_RELU && dil_of(d) == 1;
}
static bool head_shape(const s3r_conv_desc* d) {
    return d->op == S3R_OP_CONV && d->cout == 1 && d->k == 1 && d->stride == 1 && d->pad == 0 && d->act <= S3R_ACT_SIGMOID &&
           (ipow(d->in_size, d->ndim) % 4) == 0;
}
bool staged_layer(const s3r_conv_desc* d) {
    if (d->dtype != S3R_F32 || (d->op != S3R_OP_CONV && d->op != S3R_OP_DECONV) || (d->ndim != 2 && d->ndim != 3)) return false;
    if (stem_shape(d) || head_shape(d)) return false;
    if (d->op == S3R_OP_DECONV) return !(deconv_fast(d) && d->cin % 16 == 0);
    return d->cin % 16 != 0;
}
bool tclass_layer(const s3r_conv_desc* d) { return d->op == S3R_OP_DECONV && staged_layer(d) && dil_of(d) == 1; }
bool tclass_direct(const s3r_conv_desc* d) {
    return tclass_layer(d) && d->cin % 16 == 0 && d->in_halo >= tclass_halo(d) && d->in_layout == S3R_LAYOUT_PLAIN;
}
bool tshuf_layer(const s3r_conv_desc* d) {
    return tclass_layer(d) && d->k == d->stride && d->stride >= 2 && d->pad == 0 && d->out_pad == 0;
}
bool leaky_fused(const s3r_conv_desc* d) {
    return d->dtype == S3R_F32 && d->op != S3R_OP_LINEAR && d->act == S3R_ACT_LEAKY_RELU && d->act_param >= 0.f && d->act_param <= 1.f;
}
bool needs_act_pass(const s3r_conv_desc* d) { return d->act > S3R_ACT_SIGMOID && !leaky_fused(d); }

// ---------------------------------------------------------------- staged / residue-class / unfolded geometry
TClassAxis tclass_axis(const s3r_conv_desc* d, int r) {
    TClassAxis a;
    const int k = d->k, s = d->stride, p = d->pad, n_out = out_size(d);
    a.kr = r < k ? (k - r + s - 1) / s : 0;
    a.ke = a.kr > 0 ? a.kr : 1;
    a.qmin = p > r ? (p - r + s - 1) / s : 0;                       // first q with s q + r - p >= 0
    const int top = n_out - 1 + p - r;                               // last q: s q + r - p <= n_out - 1
    a.nq = top < 0 ? 0 : top / s - a.qmin + 1;
    return a;
}
int tclass_halo(const s3r_conv_desc* d) {
    int h = 0;
    for (int r = 0; r < d->stride; ++r) {
        const TClassAxis a = tclass_axis(d, r);
        if (a.nq <= 0) continue;
        const int lo = (a.ke - 1) - a.qmin, hi = a.qmin + a.nq - 1 - (d->in_size - 1);      // inputs q - (ke - 1) .. q
        if (lo > h) h = lo;
        if (hi > h) h = hi;
    }
    return h;
}
int64_t tclass_w_elems(const s3r_conv_desc* d) {
    if (tshuf_layer(d)) return (int64_t)cin_pad16(d->cin) * cout_pad(d->cout * (int)ipow(d->stride, d->ndim));      // [CinPad][cout x taps]
    int64_t per_axis = 0;
    for (int r = 0; r < d->stride; ++r) per_axis += tclass_axis(d, r).ke;
    return ipow(per_axis, d->ndim) * cin_pad16(d->cin) * cout_pad(d->cout);      // sum over classes of prod ke = (sum ke)^nd
}
bool im2col_layer(const s3r_conv_desc* d) {
    if (d->op != S3R_OP_CONV || !staged_layer(d) || d->cin > 8 || d->k > 16 || d->k < 2 || d->in_size > 4096) return false;
    const int no = out_size(d);
    if (no <= 0) return false;
    const double per_sample = ((double)d->cin * (double)ipow(d->k, d->ndim) + 15.0) * (d->ndim == 3 ? (double)no * no * no : (double)no * no);
    return per_sample * 4 <= 64.0 * (1 << 20);      // (else: channels padded to 16, the halo-padded copy)
}
StagedGeo staged_geo(const s3r_conv_desc* d) {
    StagedGeo s;
    s.bmax = 0;
    s.too_large = false;
    s.cin_pad = cin_pad16(d->cin);
    if (im2col_layer(d)) {                        // (B, KPad, n_out, ...): every tap of every channel is a K row
        s.cin_pad = cin_pad16(d->cin * (int)ipow(d->k, d->ndim));
        s.step = 1; s.pe = 0;
        s.sp = out_size(d);
        const int64_t per_sample = (int64_t)s.cin_pad * ipow(s.sp, d->ndim);
        s.bmax = (int)(((int64_t)1 << 28) / per_sample);          // 1 GiB of floats per pass (>= 16 samples by im2col_layer's bound)
        s.elems = (int64_t)(d->batch < s.bmax ? d->batch : s.bmax) * per_sample;
        return s;
    }
    // the padded edge in int64: a staged layer's halo is not bounded by the caller-halo limit, and geometry() asks before it has bounded the copy
    int64_t u = d->in_size;
    if (tclass_layer(d)) {
        s.step = 1;
        s.pe = tclass_halo(d);
    } else {
        const bool tr = d->op == S3R_OP_DECONV;
        s.step = tr ? d->stride : 1;
        s.pe = tr ? dil_of(d) * (d->k - 1) - d->pad : d->pad;
        if (tr) u = ((int64_t)d->in_size - 1) * d->stride + 1 + d->out_pad;
    }
    const int64_t sp = u + 2 * (int64_t)s.pe;
    s.sp = (int)sp;
    s.too_large = too_large({d->batch, s.cin_pad, sp, sp, d->ndim == 3 ? sp : 1}, 4);
    s.elems = s.too_large ? 0 : (int64_t)d->batch * s.cin_pad * ipow(sp, d->ndim);
    return s;
}
StagedGeo tclass_input_geo(const s3r_conv_desc* d) {
    StagedGeo sg = staged_geo(d);
    if (tclass_direct(d)) {
        sg.pe = d->in_halo;
        sg.sp = d->in_size + 2 * d->in_halo;
        sg.elems = (int64_t)d->batch * sg.cin_pad * ipow(sg.sp, d->ndim);
    }
    return sg;
}

// ---------------------------------------------------------------- descriptor validation and layer geometry
constexpr int kInLayouts[] = {S3R_LAYOUT_PLAIN, S3R_LAYOUT_WINO_H, S3R_LAYOUT_WINO_DH, S3R_LAYOUT_WINO_HW, S3R_LAYOUT_WINO_3D, S3R_LAYOUT_DIFF};
constexpr int kOutLayouts[] = {S3R_LAYOUT_PLAIN, S3R_LAYOUT_WINO_HW, S3R_LAYOUT_WINO_3D, S3R_LAYOUT_DIFF};

// the rules of the transformed layouts, and x_elems / y_elems of a tensor that is a consumer's operand instead of a plain activation
static int layout_elems(const s3r_conv_desc* d, Geo* g) {
    if (d->in_layout == S3R_LAYOUT_WINO_H) {     // the four F(2,3)-along-H plane sets a 3 x 3 [x 3] stride-1 pad-1 convolution reads
        if (d->dtype != S3R_F32 || d->op != S3R_OP_CONV || d->stride != 1 || d->k != 3 || d->pad != 1 || (g->in & 1) || d->in_halo != 1 ||
            d->cin % 16 != 0 || d->cout <= 1)
            return fail(S3R_ERR_INVALID, "a Winograd-transformed input serves an fp32 Conv k=3 s=1 p=1 over an even edge, in_halo = 1");
        if (g->in % wino_r(d) != 0) return fail(S3R_ERR_INVALID, "a Winograd-transformed input needs an edge that is a multiple of %d", wino_r(d));
        g->x_elems = operand_elems(d, S3R_LAYOUT_WINO_H, d->batch);
    }
    if (d->in_layout == S3R_LAYOUT_WINO_DH) {    // the 36 two-axis plane sets a 3 x 3 x 3 stride-1 pad-1 convolution reads
        if (d->dtype != S3R_F32 || d->op != S3R_OP_CONV || d->ndim != 3 || d->stride != 1 || d->k != 3 || d->pad != 1 || (g->in & 3) ||
            d->in_halo != 1 || d->cin % 32 != 0 || d->cout <= 1)
            return fail(S3R_ERR_INVALID, "a two-axis Winograd-transformed input serves an fp32 Conv3d k=3 s=1 p=1 over an edge %% 4 == 0, in_halo = 1");
        g->x_elems = wino2_operand_elems(0, d->cin, g->in, g->in_p, d->batch);
    }
    if (d->in_layout == S3R_LAYOUT_WINO_HW) {    // the 36 two-axis plane sets of a 2D layer, positions flat
        if (d->dtype != S3R_F32 || d->op != S3R_OP_CONV || d->ndim != 2 || d->stride != 1 || d->k != 3 || d->pad != 1 || (g->in & 3) ||
            d->in_halo != 1 || d->cin % 32 != 0 || d->cout <= 1)
            return fail(S3R_ERR_INVALID, "a two-axis Winograd-transformed input (2D) serves an fp32 Conv2d k=3 s=1 p=1 over an edge %% 4 == 0, in_halo = 1");
        g->x_elems = wino2_operand_elems(2, d->cin, g->in, g->in_p, d->batch);
    }
    if (d->out_layout == S3R_LAYOUT_WINO_HW) {   // ... written by the layer in front of it: the plane sets of THIS layer's halo-1 output
        if (d->dtype != S3R_F32 || d->op != S3R_OP_CONV || d->ndim != 2 || (g->out & 3) || d->cout % 32 != 0 || d->act == S3R_ACT_SIGMOID)
            return fail(S3R_ERR_INVALID, "the two-axis Winograd output layout is written by an fp32 Conv2d with an output edge %% 4 == 0 and cout %% 32 == 0");
        g->y_elems = wino2_operand_elems(2, d->cout, g->out, g->out + 2, d->batch);
    }
    if (d->in_layout == S3R_LAYOUT_WINO_3D) {    // the plane sets of any 3D two-axis layer, partial last groups included
        const int ax = wino2_ax(d);
        if ((ax != 0 && ax != 1) || d->in_halo != d->pad)
            return fail(S3R_ERR_INVALID, "the general two-axis Winograd input layout serves an fp32 Conv3d k=3 s=1 p=1 / k=4 s=1 p=0 with cin %% %d == 0, "
                        "in_halo = pad", s3r::wino_bk());
        g->x_elems = operand_elems(d, S3R_LAYOUT_WINO_3D, d->batch);
    }
    if (d->in_layout == S3R_LAYOUT_DIFF) {       // [x | Dh | Dd | Ddh] of the transposed Winograd form
        if (!dwino_layer(d) || d->in_halo != 1)
            return fail(S3R_ERR_INVALID, "the difference-tensor input layout serves the Winograd form of an fp32 ConvTranspose3d k=4 s=2 p=1 over an "
                        "edge %% 4 == 0, in_halo = 1");
        g->x_elems *= 4;
    }
    if (d->out_layout == S3R_LAYOUT_WINO_3D || d->out_layout == S3R_LAYOUT_DIFF) {      // ... written by the layer in front of such a consumer
        const bool diff = d->out_layout == S3R_LAYOUT_DIFF;
        if (d->dtype != S3R_F32 || d->ndim != 3 || d->cout % s3r::wino_bk() != 0 || d->act > S3R_ACT_RELU ||
            (diff ? d->out_halo != 1 || (g->out & 3) : d->out_halo > 1 || g->out < (d->out_halo ? 4 : 5)))
            return fail(S3R_ERR_INVALID, "a consumer's operand is written by an fp32 3D layer with cout %% %d == 0, no activation or ReLU, and the halo the "
                        "consumer reads (two-axis planes: out_halo 1 for k3 p1, 0 for k4 p0; difference tensors: out_halo 1, output edge %% 4 == 0)",
                        s3r::wino_bk());
        if (diff) g->y_elems *= 4;
        // (the consumer's OUTPUT edge: out_halo 1, k3 p1, keeps this layer's; out_halo 0, k4 p0, loses 3)
        else g->y_elems = wino2_operand_elems(d->out_halo ? 0 : 1, d->cout, d->out_halo ? g->out : g->out - 3, g->out_p, d->batch);
    }
    return S3R_OK;
}

int geometry(const s3r_conv_desc* d, Geo* g) {
    if (!d) return fail(S3R_ERR_INVALID, "null descriptor");
    if (d->batch <= 0 || d->cin <= 0 || d->cout <= 0) return fail(S3R_ERR_INVALID, "batch/cin/cout must be positive");
    if (d->in_halo < 0 || d->out_halo < 0 || d->in_halo > 8 || d->out_halo > 8)
        return fail(S3R_ERR_INVALID, "halo must be in [0, 8]");
    if (d->dtype != S3R_F32 && d->dtype != S3R_BF16) return fail(S3R_ERR_INVALID, "unknown dtype %d", d->dtype);
    if (!one_of(d->in_layout, kInLayouts) || !one_of(d->out_layout, kOutLayouts)) return fail(S3R_ERR_INVALID, "unknown layout");
    if ((d->in_layout || d->out_layout) && d->op == S3R_OP_LINEAR)
        return fail(S3R_ERR_INVALID, "the transformed input layout exists on the convolution paths only");
    if (d->op == S3R_OP_LINEAR) {
        if (d->in_halo || d->out_halo) return fail(S3R_ERR_INVALID, "linear layers take no halo");
        if (d->act < S3R_ACT_NONE || d->act > S3R_ACT_TANH) return fail(S3R_ERR_INVALID, "unknown activation %d", d->act);
        g->nd = 0; g->in = g->out = g->in_p = g->out_p = 1; g->in_sp = 1; g->out_sp = 1;
        g->x_elems = (int64_t)d->batch * d->cin;
        g->y_elems = (int64_t)d->batch * d->cout;
        g->w_elems = (int64_t)d->cin * d->cout;
        g->x_store = g->x_elems; g->y_store = g->y_elems;
        g->flops = 2.0 * d->batch * (double)d->cin * d->cout;
        g->bytes = 4.0 * (g->x_elems + g->y_elems + g->w_elems);
        if (d->dtype != S3R_F32) return fail(S3R_ERR_INVALID, "linear layers exist on the fp32 path only");
        return S3R_OK;
    }
    if (d->op != S3R_OP_CONV && d->op != S3R_OP_DECONV) return fail(S3R_ERR_INVALID, "unknown op %d", d->op);
    if (d->ndim != 2 && d->ndim != 3) return fail(S3R_ERR_INVALID, "ndim must be 2 or 3");
    if (d->in_size <= 0 || d->k <= 0 || d->stride <= 0 || d->pad < 0) return fail(S3R_ERR_INVALID, "bad size/k/stride/pad");
    if (d->dilation < 0 || d->out_pad < 0) return fail(S3R_ERR_INVALID, "dilation / out_pad must not be negative");
    if (d->act < S3R_ACT_NONE || d->act > S3R_ACT_TANH) return fail(S3R_ERR_INVALID, "unknown activation %d", d->act);
    if (d->dtype == S3R_BF16 && (dil_of(d) != 1 || d->out_pad != 0 || d->act > S3R_ACT_SIGMOID || (d->op == S3R_OP_DECONV && !deconv_fast(d))))
        return fail(S3R_ERR_INVALID, "bf16 path: Conv with dilation 1 / ConvTranspose3d k4 s2 p1 and none / relu / sigmoid only (the "
                    "parameter-general layers are fp32)");
    if (d->op == S3R_OP_CONV && d->out_pad != 0) return fail(S3R_ERR_INVALID, "out_pad belongs to transposed convolutions");
    if (d->op == S3R_OP_DECONV && !deconv_fast(d)) {
        if (dil_of(d) * (d->k - 1) - d->pad < 0)
            return fail(S3R_ERR_INVALID, "ConvTranspose with pad %d > dilation * (k - 1) = %d crops more than the kernel reaches: not supported",
                        d->pad, dil_of(d) * (d->k - 1));
        if (d->out_pad >= (d->stride > dil_of(d) ? d->stride : dil_of(d)))
            return fail(S3R_ERR_INVALID, "out_pad %d must be smaller than max(stride, dilation)", d->out_pad);
    }
    if (staged_layer(d) && !im2col_layer(d)) {
        if (d->stride > 64 || d->k > 1024) return fail(S3R_ERR_INVALID, "stride / kernel size out of range");
        if (staged_geo(d).too_large)
            return fail(S3R_ERR_INVALID, "staged input too large for one call (>= 2^31 elements / 4 GiB): split the batch");
    }
    g->nd = d->ndim;
    g->in = d->in_size;
    g->out = out_size(d);
    if (g->out <= 0) return fail(S3R_ERR_INVALID, "empty output");
    g->in_p = g->in + 2 * d->in_halo;
    g->out_p = g->out + 2 * d->out_halo;
    g->in_sp = ipow(g->in, g->nd);
    g->out_sp = ipow(g->out, g->nd);
    g->x_elems = (int64_t)d->batch * d->cin * ipow(g->in_p, g->nd);
    g->y_elems = (int64_t)d->batch * d->cout * ipow(g->out_p, g->nd);
    const int rc = layout_elems(d, g);
    if (rc) return rc;
    g->w_elems = (int64_t)d->cin * d->cout * ipow(d->k, g->nd);
    if (d->op == S3R_OP_DECONV)
        g->flops = 2.0 * d->batch * (double)d->cin * g->in_sp * d->cout * ipow(d->k, g->nd);
    else
        g->flops = 2.0 * d->batch * (double)d->cout * g->out_sp * d->cin * ipow(d->k, g->nd);
    // element sizes: the bf16 path reads fp32 renders in its stem and writes fp32 probabilities from its head
    const bool bf = d->dtype == S3R_BF16;
    const bool stem = d->ndim == 2 && d->cin == 3;
    const bool head = d->cout == 1 && d->k == 1;
    const int xs = (bf && !stem) ? 2 : 4, ys = (bf && !head) ? 2 : 4, wsz = bf && !stem && !head ? 2 : 4;
    g->x_store = (g->x_elems * xs + 3) / 4;
    g->y_store = (g->y_elems * ys + 3) / 4;
    g->bytes = (double)d->batch * (xs * d->cin * (double)g->in_sp + ys * d->cout * (double)g->out_sp) + wsz * (double)g->w_elems;
    if (g->x_elems >= kMaxElems || g->y_elems >= kMaxElems || g->x_elems * 4 >= kMaxBytes || g->y_elems * 4 >= kMaxBytes)
        return fail(S3R_ERR_INVALID, "tensor too large for one call (>= 2^31 elements / 4 GiB): split the batch");
    return S3R_OK;
}

// ---------------------------------------------------------------- route and halos
int route(const s3r_conv_desc* d, Route* r) {
    if (d->op == S3R_OP_LINEAR) { *r = R_LINEAR; return S3R_OK; }
    if (stem_shape(d)) { *r = R_STEM; return S3R_OK; }
    if (head_shape(d)) { *r = R_HEAD; return S3R_OK; }
    if (d->dtype == S3R_BF16 ? d->cin % 32 == 0 : (d->cin % 16 == 0 || staged_layer(d))) { *r = R_MFMA; return S3R_OK; }
    return fail(S3R_ERR_INVALID, "no kernel for this layer shape (cin=%d cout=%d k=%d s=%d p=%d ndim=%d): the MFMA path "
                "needs cin %% 16 == 0", d->cin, d->cout, d->k, d->stride, d->pad, d->ndim);
}

int need_halo(const s3r_conv_desc* d, Route r) {
    if (r != R_MFMA || staged_layer(d)) return 0;
    return d->op == S3R_OP_DECONV ? 1 : d->pad;
}

int want_halo(const s3r_conv_desc* d, Route r) {
    if (r == R_MFMA && tclass_layer(d) && d->cin % 16 == 0 && tclass_halo(d) <= 8) return tclass_halo(d);
    return need_halo(d, r);
}

int check_halos(const s3r_conv_desc* d, Route r) {
    if ((d->in_layout || d->out_layout) && r != R_MFMA)
        return fail(S3R_ERR_INVALID, "the transformed input layout is read by the MFMA convolution kernels only");
    if (d->in_halo < need_halo(d, r))
        return fail(S3R_ERR_INVALID, "this layer's kernel reads its zero padding from memory: the input must carry a "
                    "zero halo of >= %d (got in_halo=%d); s3r_chain_forward pads unpadded inputs itself",
                    need_halo(d, r), d->in_halo);
    if ((r == R_STEM || r == R_HEAD) && d->in_halo != 0) return fail(S3R_ERR_INVALID, "stem / head kernels take an unpadded input");
    if (r == R_HEAD && d->out_halo != 0) return fail(S3R_ERR_INVALID, "head kernel writes an unpadded output");
    return S3R_OK;
}

}  // namespace s3rh

extern "C" int s3r_conv_out_size(const s3r_conv_desc* d) {
    using namespace s3rh;
    if (!d) return fail(S3R_ERR_INVALID, "null descriptor");
    if (d->op == S3R_OP_LINEAR) return 1;
    if (d->op != S3R_OP_CONV && d->op != S3R_OP_DECONV) return fail(S3R_ERR_INVALID, "unknown op %d", d->op);
    if (d->in_size <= 0 || d->k <= 0 || d->stride <= 0 || d->pad < 0)
        return fail(S3R_ERR_INVALID, "bad size/k/stride/pad (in_size=%d k=%d stride=%d pad=%d)", d->in_size, d->k, d->stride, d->pad);
    const int n = out_size(d);
    if (n <= 0) return fail(S3R_ERR_INVALID, "empty output");
    return n;
}
