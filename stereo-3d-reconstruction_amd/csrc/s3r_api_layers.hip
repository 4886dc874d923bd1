// C-ABI entry points of the layer-level ops (declared in include/s3r.h): the version and the error text, the bf16 -> fp32 conversion,
// linear forward / backward, head, conv, stem and BatchNorm backward, the optimizer.  A forward, its backward and their scratch
// queries live together; a family's own checks are the file-local helpers below, the checks every family shares are at the end of
// s3r_host.h.  Every entry point validates on the host, refuses before anything is enqueued, then launches ONCE.  Host code only.
#include "s3r_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

using namespace s3rh;

namespace {

int linear_dims(int batch, int cin, int cout) {
    if (batch <= 0 || cin <= 0 || cout <= 0) return fail(S3R_ERR_INVALID, "linear dims must be positive");
    return S3R_OK;
}
// ... and every tensor of a linear-backward call within the header's limits
int linbwd_dims(int batch, int cin, int cout) {
    if (int rc = linear_dims(batch, cin, cout)) return rc;
    if (too_large({batch, cin}, 4) || too_large({batch, cout}, 4) || too_large({cin, cout}, 4)) return too_large_fail();
    return S3R_OK;
}

// x / grad_x of a head-backward call within the header's limits; they are its largest tensors
int headbwd_dims(int batch, int channels, int64_t voxels) {
    if (batch < 0 || channels <= 0 || voxels <= 0)
        return fail(S3R_ERR_INVALID, "head backward dims: batch >= 0, channels > 0 and voxels > 0 (batch %d, channels %d, voxels %lld)", batch,
                    channels, (long long)voxels);
    if (too_large({voxels, channels, batch}, 4)) return too_large_fail();
    return S3R_OK;
}

// what the conv-backward entry points take: an fp32 Conv / ConvTranspose, dilation 1, plain tensors without halos, none / relu / sigmoid.
// `batch_min` 0: s3r_conv_backward and its scratch query accept an empty batch.  Fills the geometry (of batch max(batch, 1)) and tiling
int convbwd_check(const s3r_conv_desc* d, const char* who, int batch_min, Geo* g, s3r::ConvBwdGeo* cg) {
    if (!d) return fail(S3R_ERR_INVALID, "%s: null descriptor", who);
    if (d->dtype != S3R_F32) return fail(S3R_ERR_INVALID, "%s: fp32 layers only (dtype %d)", who, d->dtype);
    if (d->op != S3R_OP_CONV && d->op != S3R_OP_DECONV)
        return fail(S3R_ERR_INVALID, "%s: Conv / ConvTranspose layers only (op %d; linear layers have s3r_linear_backward)", who, d->op);
    if (dil_of(d) != 1) return fail(S3R_ERR_INVALID, "%s: dilation 1 only (got %d)", who, d->dilation);
    if (d->in_layout != S3R_LAYOUT_PLAIN || d->out_layout != S3R_LAYOUT_PLAIN || d->in_halo != 0 || d->out_halo != 0)
        return fail(S3R_ERR_INVALID, "%s: plain tensors only (layouts PLAIN, halos 0)", who);
    if (int rc = check_act(d->act, who)) return rc;
    if (d->batch < batch_min) return fail(S3R_ERR_INVALID, "%s: batch must be >= %d (got %d)", who, batch_min, d->batch);
    s3r_conv_desc one = *d;
    if (one.batch == 0) one.batch = 1;
    if (int rc = geometry(&one, g)) return rc;
    if (g->w_elems >= kMaxElems) return fail(S3R_ERR_INVALID, "%s: weight of 2^31 elements or more", who);
    if (!s3r::convbwd_geo(d->op == S3R_OP_DECONV, d->ndim, d->cin, d->cout, g->in, g->out, d->k, d->stride, d->pad, cg))
        return fail(S3R_ERR_INVALID, "%s: no tiling of the weight-gradient GEMM fits this kernel size / stride (k %d, stride %d)", who, d->k,
                    d->stride);
    if ((int64_t)d->batch * cg->nsl * cg->tiles >= kMaxElems) return fail(S3R_ERR_INVALID, "%s: too many workgroups: split the batch", who);
    return S3R_OK;
}

// the stem backward's shape: in_size >= 1, n_images >= 0, y / grad_y (n_images,32,m,m) within the header's limits; fills m
int stembwd_dims(int n_images, int in_size, const char* who, int* m_out) {
    if (n_images < 0 || in_size < 1)
        return fail(S3R_ERR_INVALID, "%s: n_images >= 0 and in_size >= 1 (n_images %d, in_size %d)", who, n_images, in_size);
    const int m = (in_size - 1) / 2 + 1;
    if (too_large({32, m, m, n_images}, 4)) return fail(S3R_ERR_INVALID, "%s: tensor of 2^31 elements / 4 GiB or more: split the batch", who);
    *m_out = m;
    return S3R_OK;
}

// z / y / grad_z of a train-mode BatchNorm call within the header's limits
int bn_dims(int batch, int channels, int64_t positions) {
    if (batch < 0 || channels <= 0 || positions <= 0)
        return fail(S3R_ERR_INVALID, "batchnorm dims: batch >= 0, channels > 0 and positions > 0 (batch %d, channels %d, positions %lld)", batch,
                    channels, (long long)positions);
    if (too_large({positions, channels, batch}, 4)) return fail(S3R_ERR_INVALID, "tensor of 4 GiB or more: split the channels");
    return S3R_OK;
}
// ... and what the forward and the backward check between the empty-batch return and their pointers
int bn_stats(int batch, int64_t positions) {
    if ((int64_t)batch * positions >= 2) return S3R_OK;
    return fail(S3R_ERR_INVALID, "batchnorm: batch statistics need more than one value per channel (batch * positions = 1)");
}

bool optim_bad(float x, bool below_one) { return !std::isfinite(x) || x < 0.f || (below_one && x >= 1.f); }

int optim_state_lr(const float* state, float lr) {
    if (!state) return fail(S3R_ERR_INVALID, "optimizer: null state");
    if (optim_bad(lr, false)) return fail(S3R_ERR_INVALID, "optimizer: lr must be finite and >= 0");
    return S3R_OK;
}

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

// the descriptor's own checks
int optim_desc(const s3r_optim_desc* d) {
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
    return S3R_OK;
}

}  // namespace

extern "C" {

int s3r_abi_version(void) { return S3R_ABI_VERSION; }

const char* s3r_last_error(void) { return last_error(); }

int s3r_channels_last_to_f32(const void* x, float* y, int batch, int channels, int64_t positions, void* stream) {
    if (!x || !y) return null_tensor();
    if (misaligned16(x)) return bf16_align_fail("the bf16 channels-last tensor", x);
    if (batch <= 0 || channels <= 0 || positions <= 0) return fail(S3R_ERR_INVALID, "dims must be positive");
    if (batch > 65535 || (int64_t)channels * positions >= kMaxElems)
        return fail(S3R_ERR_INVALID, "tensor too large for one call: split the batch");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_PAD, 1, 0.0, 6.0 * (double)batch * channels * (double)positions);
    return launched(s3r::launch_cl_bf16_to_f32(x, y, batch, positions, channels, s), "channels-last to fp32 launch");
}

// ---------------------------------------------------------------- linear (s3r_pointwise.hip, s3r_linear_bwd.hip)
int64_t s3r_linear_scratch_elems(int batch, int cin, int cout) {
    if (int rc = linear_dims(batch, cin, cout)) return rc;
    return s3r::linear_scratch_elems(batch, cin, cout);
}

int s3r_linear_forward(const float* x, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                       int act, float* scratch, int64_t scratch_elems, void* stream) {
    if (!x || !w || !y) return null_tensor();
    if (int rc = linear_dims(batch, cin, cout)) return rc;
    if (act < S3R_ACT_NONE || act > S3R_ACT_SIGMOID)
        return fail(S3R_ERR_INVALID, "s3r_linear_forward takes none / relu / sigmoid (act %d): LeakyReLU / ELU / Tanh carry a parameter — "
                    "run the layer as an S3R_OP_LINEAR descriptor through s3r_conv_forward / s3r_chain_forward", act);
    if (!scratch || scratch_elems < s3r::linear_scratch_elems(batch, cin, cout))      // (its own words: no ", got")
        return fail(S3R_ERR_WORKSPACE, "linear needs %lld floats of scratch (s3r_linear_scratch_elems)",
                    (long long)s3r::linear_scratch_elems(batch, cin, cout));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_LINEAR, 0, 2.0 * batch * (double)cin * cout, 4.0 * ((double)cin * cout + (double)batch * (cin + cout)));
    return launched(s3r::launch_linear(x, w, nullptr, bias, y, batch, cin, cout, act, scratch, s), "linear launch");
}

int64_t s3r_linear_backward_scratch_elems(int batch, int cin, int cout) {
    if (int rc = linbwd_dims(batch, cin, cout)) return rc;
    return s3r::linear_backward_scratch_elems(batch, cin, cout);
}

int s3r_linear_backward(const float* x, const float* w, const float* y, const float* grad_y, float* grad_x, float* grad_w,
                        float* grad_bias, int batch, int cin, int cout, int act, float* scratch, int64_t scratch_elems, void* stream) {
    if (!grad_x && !grad_w && !grad_bias)
        return fail(S3R_ERR_INVALID, "linear backward: grad_x, grad_w and grad_bias are all NULL (each may be: it is not computed)");
    if (int rc = check_act(act, "s3r_linear_backward")) return rc;
    if (!grad_y || (grad_w && !x) || (grad_x && !w)) return null_tensor();
    if (int rc = check_y(act, y, "linear backward")) return rc;
    if (int rc = linbwd_dims(batch, cin, cout)) return rc;
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "linear backward", s3r::linear_backward_scratch_elems(batch, cin, cout),
                              "s3r_linear_backward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const double B = batch, I = cin, O = cout;
    const double flops = 2.0 * B * I * O * ((grad_w ? 1.0 : 0.0) + (grad_x ? 1.0 : 0.0));
    const double elems = B * O * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (grad_w ? B * I + I * O : 0.0) + (grad_x ? I * O + B * I : 0.0) +
                         (grad_bias ? O : 0.0);
    ProfScope ps(s, F_LINEAR, 1, flops, 4.0 * elems);
    return launched(s3r::launch_linear_backward(x, w, y, grad_y, grad_x, grad_w, grad_bias, batch, cin, cout, act, scratch, s, &ps.launches),
                    "linear backward launch");
}

// ---------------------------------------------------------------- head backward (s3r_head_bwd.hip)
int64_t s3r_head_backward_scratch_elems(int batch, int channels, int64_t voxels) {
    if (int rc = headbwd_dims(batch, channels, voxels)) return rc;
    return s3r::head_backward_scratch_elems(batch, channels, voxels);
}

int s3r_head_backward(const float* x, const float* w, const float* scale, const float* y, const float* grad_y, float* grad_x,
                      float* grad_w, float* grad_shift, int batch, int channels, int64_t voxels, int act, float* scratch,
                      int64_t scratch_elems, void* stream) {
    if (!grad_x && !grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "head backward: grad_x, grad_w and grad_shift are all NULL (each may be: it is not computed)");
    if (int rc = check_act(act, "s3r_head_backward")) return rc;
    if (int rc = headbwd_dims(batch, channels, voxels)) return rc;
    if (batch == 0) return S3R_OK;
    if (!grad_y || (grad_w && !x) || (grad_x && !w)) return null_tensor();
    if (int rc = check_y(act, y, "head backward")) return rc;
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "head backward", s3r::head_backward_scratch_elems(batch, channels, voxels),
                              "s3r_head_backward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const double B = batch, C = channels, S = (double)voxels;
    const double flops = (grad_w ? 2.0 * B * C * S : 0.0) + (grad_x ? B * C * S : 0.0);
    const double elems = B * S * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale ? 1.0 : 0.0) + (grad_w ? B * C * S + C : 0.0) +
                         (grad_x ? C + B * C * S : 0.0) + (grad_shift ? 1.0 : 0.0);
    ProfScope ps(s, F_HEAD, 1, flops, 4.0 * elems);
    return launched(s3r::launch_head_backward(x, w, scale, y, grad_y, grad_x, grad_w, grad_shift, batch, channels, voxels, act, scratch, s,
                                              &ps.launches), "head backward launch");
}

// ---------------------------------------------------------------- conv backward (s3r_conv_bwd.hip)
int s3r_conv_adjoint_desc(const s3r_conv_desc* d, s3r_conv_desc* adj) {
    Geo g, ga;
    s3r::ConvBwdGeo cg;
    if (!adj) return fail(S3R_ERR_INVALID, "s3r_conv_adjoint_desc: null output descriptor");
    if (int rc = convbwd_check(d, "s3r_conv_adjoint_desc", 1, &g, &cg)) return rc;
    s3r_conv_desc a;
    memset(&a, 0, sizeof(a));
    a.op = d->op == S3R_OP_CONV ? S3R_OP_DECONV : S3R_OP_CONV;
    a.ndim = d->ndim; a.batch = d->batch; a.tag = d->tag;
    a.cin = d->cout; a.cout = d->cin;
    a.in_size = g.out;
    a.k = d->k; a.stride = d->stride; a.pad = d->pad;
    a.act = S3R_ACT_NONE; a.tile = -1; a.dtype = S3R_F32; a.algo = S3R_ALGO_AUTO; a.dilation = 1;
    a.out_pad = d->op == S3R_OP_CONV ? (d->in_size + 2 * d->pad - d->k) % d->stride : 0;
    if (int rc = geometry(&a, &ga)) return rc;                           // (a Conv with pad > k - 1 has no ConvTranspose this library runs)
    if (ga.out != d->in_size) return fail(S3R_ERR_INVALID, "s3r_conv_adjoint_desc: internal: adjoint output edge %d != input edge %d", ga.out, d->in_size);
    *adj = a;
    return S3R_OK;
}

int64_t s3r_conv_backward_scratch_elems(const s3r_conv_desc* d) {
    Geo g;
    s3r::ConvBwdGeo cg;
    if (int rc = convbwd_check(d, "s3r_conv_backward_scratch_elems", 0, &g, &cg)) return rc;
    if (d->batch == 0) return 0;
    return s3r::conv_backward_scratch_elems(cg, d->batch, d->cout, g.out_sp);
}

int s3r_conv_backward(const s3r_conv_desc* d, const float* x, const float* y, const float* grad_y, const float* scale, float* gs,
                      float* grad_w, float* grad_shift, float* scratch, int64_t scratch_elems, void* hip_stream) {
    if (!gs && !grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "conv backward: gs, grad_w and grad_shift are all NULL (each may be: it is not computed)");
    Geo g;
    s3r::ConvBwdGeo cg;
    if (int rc = convbwd_check(d, "s3r_conv_backward", 0, &g, &cg)) return rc;
    if (d->batch == 0) return S3R_OK;
    if (!grad_y || (grad_w && !x)) return null_tensor();
    if (int rc = check_y(d->act, y, "conv backward")) return rc;
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "conv backward", s3r::conv_backward_scratch_elems(cg, d->batch, d->cout, g.out_sp),
                              "s3r_conv_backward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const double B = d->batch, Y = B * d->cout * (double)g.out_sp, X = B * d->cin * (double)g.in_sp;
    const double flops = grad_w ? 2.0 * B * (double)cg.Q * cg.Ca * cg.Cf * cg.T : 0.0;
    const double elems = Y * (d->act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale ? d->cout : 0.0) + (gs ? Y : 0.0) +
                         (grad_w ? X + (double)g.w_elems : 0.0) + (grad_shift ? d->cout : 0.0);
    ProfScope ps(s, F_MFMA, S3R_CONV_BACKWARD_TAG + d->tag, flops, 4.0 * elems);
    return launched(s3r::launch_conv_backward(cg, d->op == S3R_OP_DECONV, x, y, grad_y, scale, gs, grad_w, grad_shift, d->batch, d->cout,
                                              g.out_sp, d->act, scratch, s, &ps.launches), "conv backward launch");
}

// ---------------------------------------------------------------- stem backward (s3r_stem_bwd.hip)
int64_t s3r_stem_backward_scratch_elems(int n_images, int in_size) {
    int m = 0;
    if (int rc = stembwd_dims(n_images, in_size, "s3r_stem_backward_scratch_elems", &m)) return rc;
    return s3r::stem_backward_scratch_elems(n_images, m);
}

int s3r_stem_backward(const void* images_left, const void* images_right, int n_left, int renders_u8, const float* y, const float* grad_y,
                      const float* scale, float* grad_w, float* grad_shift, int n_images, int in_size, int act, float* scratch,
                      int64_t scratch_elems, void* hip_stream) {
    if (!grad_w && !grad_shift)
        return fail(S3R_ERR_INVALID, "stem backward: grad_w and grad_shift are both NULL (each may be: it is not computed)");
    if (act != S3R_ACT_NONE && act != S3R_ACT_RELU) return fail(S3R_ERR_INVALID, "s3r_stem_backward takes none / relu (act %d)", act);
    int m = 0;
    if (int rc = stembwd_dims(n_images, in_size, "s3r_stem_backward", &m)) return rc;
    if (n_images == 0) return S3R_OK;
    if (images_right ? (n_left < 1 || n_left > n_images) : n_left != n_images)
        return fail(S3R_ERR_INVALID, "stem backward: n_left must lie in [1, n_images] with two render tensors and equal n_images with one "
                                     "(n_left %d, n_images %d)", n_left, n_images);
    if (!images_left || !grad_y) return null_tensor();
    if (int rc = check_y(act, y, "stem backward")) return rc;
    if (int rc = check_renders_aligned(images_left, images_right)) return rc;
    if (too_large({3, in_size, in_size, n_left > n_images - n_left ? n_left : n_images - n_left}, renders_u8 ? 1 : 4))
        return fail(S3R_ERR_INVALID, "stem backward: render tensor of 2^31 elements / 4 GiB or more: split the batch");
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "stem backward", s3r::stem_backward_scratch_elems(n_images, m),
                              "s3r_stem_backward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const double B = n_images, Y = B * 32.0 * (double)m * m, P = (double)in_size * in_size;
    const double flops = grad_w ? 2.0 * B * (double)m * m * 32.0 * 27.0 : 0.0;
    const double bytes = 4.0 * (Y * (act != S3R_ACT_NONE ? 2.0 : 1.0) + (scale && grad_w ? 32.0 : 0.0) + (grad_w ? 864.0 : 0.0) +
                                (grad_shift ? 32.0 : 0.0)) + (grad_w ? (renders_u8 ? 1.0 : 4.0) * B * 3.0 * P : 0.0);
    ProfScope ps(s, F_STEM, 1, flops, bytes);
    return launched(s3r::launch_stem_backward(images_left, images_right, n_left, renders_u8 != 0, y, grad_y, scale, grad_w, grad_shift,
                                              n_images, in_size, m, act, scratch, s, &ps.launches), "stem backward launch");
}

// ---------------------------------------------------------------- train-mode BatchNorm (s3r_batchnorm.hip)
int64_t s3r_batchnorm_train_forward_scratch_elems(int batch, int channels, int64_t positions) {
    if (int rc = bn_dims(batch, channels, positions)) return rc;
    return s3r::batchnorm_forward_scratch_elems(batch, channels, positions);
}

int64_t s3r_batchnorm_train_backward_scratch_elems(int batch, int channels, int64_t positions) {
    if (int rc = bn_dims(batch, channels, positions)) return rc;
    return s3r::batchnorm_backward_scratch_elems(batch, channels, positions);
}

int s3r_batchnorm_train_forward(const float* z, const float* gamma, const float* beta, float eps, int act, float* y, float* save_mean,
                                float* save_var, float* save_invstd, int batch, int channels, int64_t positions, float* scratch,
                                int64_t scratch_elems, void* hip_stream) {
    if (int rc = check_act(act, "s3r_batchnorm_train_forward")) return rc;
    if (int rc = bn_dims(batch, channels, positions)) return rc;
    if (batch == 0) return S3R_OK;
    if (int rc = bn_stats(batch, positions)) return rc;
    if (!z || !gamma || !beta || !y || !save_mean || !save_var || !save_invstd) return null_tensor();
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "batchnorm forward", s3r::batchnorm_forward_scratch_elems(batch, channels, positions),
                              "s3r_batchnorm_train_forward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const double T = (double)batch * channels * (double)positions;
    ProfScope ps(s, F_HEAD, 2, 0.0, 4.0 * (4.0 * T + 5.0 * channels));
    return launched(s3r::launch_batchnorm_train_forward(z, gamma, beta, eps, act, y, save_mean, save_var, save_invstd, batch, channels,
                                                        positions, scratch, s, &ps.launches), "batchnorm forward launch");
}

int s3r_batchnorm_train_backward(const float* z, const float* y, const float* grad_y, const float* gamma, const float* save_mean,
                                 const float* save_invstd, int act, float* grad_z, float* grad_gamma, float* grad_beta, int batch,
                                 int channels, int64_t positions, float* scratch, int64_t scratch_elems, void* hip_stream) {
    if (!grad_z && !grad_gamma && !grad_beta)
        return fail(S3R_ERR_INVALID, "batchnorm backward: grad_z, grad_gamma and grad_beta are all NULL (each may be: it is not computed)");
    if (int rc = check_act(act, "s3r_batchnorm_train_backward")) return rc;
    if (int rc = bn_dims(batch, channels, positions)) return rc;
    if (batch == 0) return S3R_OK;
    if (int rc = bn_stats(batch, positions)) return rc;
    const bool gg = grad_gamma || grad_z;
    if (!grad_y || (gg && (!z || !save_mean || !save_invstd)) || (grad_z && !gamma)) return null_tensor();
    if (int rc = check_y(act, y, "batchnorm backward")) return rc;
    if (int rc = need_scratch(S3R_ERR_WORKSPACE, "batchnorm backward", s3r::batchnorm_backward_scratch_elems(batch, channels, positions),
                              "s3r_batchnorm_train_backward_scratch_elems", scratch, scratch_elems))
        return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const double T = (double)batch * channels * (double)positions;
    const double reads = 1.0 + (act != S3R_ACT_NONE ? 1.0 : 0.0) + (gg ? 1.0 : 0.0);
    ProfScope ps(s, F_HEAD, 3, 0.0, 4.0 * (T * (grad_z ? 2.0 * reads + 1.0 : reads) + (double)channels * ((gg ? 2.0 : 0.0) + (grad_z ? 1.0 : 0.0) +
                                                 (grad_gamma ? 1.0 : 0.0) + (grad_beta ? 1.0 : 0.0))));
    return launched(s3r::launch_batchnorm_train_backward(z, y, grad_y, gamma, save_mean, save_invstd, act, grad_z, grad_gamma, grad_beta, batch,
                                                         channels, positions, scratch, s, &ps.launches), "batchnorm backward launch");
}

// ---------------------------------------------------------------- optimizer step (s3r_optim.hip)
int64_t s3r_optim_scratch_elems(const s3r_optim_tensor* t, int n_tensors) {
    if (int rc = optim_list(t, n_tensors, -1, -1)) return rc;
    return s3r::optim_chunks(t, n_tensors) + n_tensors;
}

int s3r_optim_state_init(float* state, float lr, void* hip_stream) {
    if (int rc = optim_state_lr(state, lr)) return rc;
    return launched(s3r::launch_optim_state_init(state, lr, (hipStream_t)hip_stream), "optimizer state init launch");
}

int s3r_optim_set_lr(float* state, float lr, void* hip_stream) {
    if (int rc = optim_state_lr(state, lr)) return rc;
    return launched(s3r::launch_optim_set_lr(state, lr, (hipStream_t)hip_stream), "optimizer set-lr launch");
}

int s3r_optim_step(const s3r_optim_desc* d, const s3r_optim_tensor* t, int n_tensors, float* state, float* scratch,
                   int64_t scratch_elems, void* hip_stream) {
    if (int rc = optim_desc(d)) return rc;
    if (!state) return fail(S3R_ERR_INVALID, "optimizer: null state");
    const bool adam = d->kind == S3R_OPT_ADAM, need_m = adam || d->beta1 != 0.f;
    if (int rc = optim_list(t, n_tensors, need_m, adam)) return rc;
    if (d->flags & (S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE))      // (S3R_ERR_INVALID, not _WORKSPACE: kept as ABI 8 answers)
        if (int rc = need_scratch(S3R_ERR_INVALID, "optimizer: the gradient norm", s3r::optim_chunks(t, n_tensors) + n_tensors,
                                  "s3r_optim_scratch_elems", scratch, scratch_elems))
            return rc;
    std::vector<std::pair<uintptr_t, int>> ps((size_t)n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        const int64_t bytes = 4 * t[i].elems;
        const Span p = {t[i].param, bytes, "param"}, m = {need_m ? t[i].m : nullptr, bytes, "m"}, v = {adam ? t[i].v : nullptr, bytes, "v"};
        if (overlap(p, m) || overlap(p, v) || overlap(m, v)) return fail(S3R_ERR_INVALID, "optimizer: tensor %d: param, m and v overlap", i);
        ps[(size_t)i] = {(uintptr_t)t[i].param, i};
    }
    std::sort(ps.begin(), ps.end());
    for (int i = 1; i < n_tensors; ++i)
        if (ps[(size_t)i].first == ps[(size_t)i - 1].first)
            return fail(S3R_ERR_INVALID, "optimizer: tensors %d and %d have the same param", ps[(size_t)i - 1].second, ps[(size_t)i].second);
    return launched(s3r::launch_optim_step(d->kind, d->flags, d->beta1, d->beta2, d->eps, d->weight_decay, d->max_norm, t, n_tensors, state,
                                           scratch, (hipStream_t)hip_stream), "optimizer step launch");
}

}  // extern "C"
