// C-ABI entry points of the stereo and shape ops (declared in include/s3r.h): cost volume, disparity read-outs, metrics and loss,
// augmentation, Chamfer distance, IoU, voxel BCE, surface point clouds.  A forward, its backward and their scratch queries live
// together; a family's own checks are the file-local helpers below, the checks every family shares are at the end of s3r_host.h.
// Every entry point validates on the host, refuses before anything is enqueued, then launches ONCE.  Host code only.
#include "s3r_host.h"

#include <cmath>

using namespace s3rh;

namespace {

int elems_fail() { return fail(S3R_ERR_INVALID, "tensor of 2^31 elements or more: split the batch"); }
int batch_fail() { return fail(S3R_ERR_INVALID, "batch > 65535: split the call"); }

// what the fp32 and the bf16 cost volume share: dims, halo and the padded volume's size (the LDS rule and its place differ)
int costvol_dims(int batch, int channels, int max_disp, int height, int width) {
    if (batch <= 0 || channels <= 0 || max_disp <= 0 || height <= 0 || width <= 0) return fail(S3R_ERR_INVALID, "cost volume dims must be positive");
    return S3R_OK;
}
int costvol_size(int batch, int channels, int max_disp, int height, int width, int out_halo) {
    if (out_halo < 0 || out_halo > 8) return fail(S3R_ERR_INVALID, "halo must be in [0, 8]");
    const int64_t out_p = (int64_t)batch * 2 * channels * (max_disp + 2 * out_halo) * (height + 2 * out_halo) * (width + 2 * out_halo);
    if (out_p >= kMaxElems) return fail(S3R_ERR_INVALID, "cost volume too large for one call: split the batch");
    return S3R_OK;
}
// ... and the two Winograd layouts: max_disp against the width, the kernel's LDS
int costvol_wino_fits(int max_disp, int height, int width) {
    if (max_disp > width) return fail(S3R_ERR_INVALID, "max_disp %d exceeds the feature width %d", max_disp, width);
    if ((size_t)2 * height * width * sizeof(float) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the kernel's 64 KiB of LDS", height, width);
    return S3R_OK;
}

// The soft read-out's argument checks, shared by the forward and its backward (one message path: what the forward refuses, the
// backward refuses in the same words).  soft_args: temperature and dims; soft_shape: the LDS rule and the size limits.
int soft_args(int batch, int channels, int height, int width, int max_disp, float temperature, int out_height, int out_width) {
    if (!(temperature > 0.f) || !std::isfinite(temperature))
        return fail(S3R_ERR_INVALID, "soft read-out temperature must be finite and > 0 (got %g)", (double)temperature);
    if (batch < 0 || channels <= 0 || height <= 0 || width <= 0 || max_disp <= 0 || out_height <= 0 || out_width <= 0)
        return fail(S3R_ERR_INVALID, "soft read-out dims must be positive (batch >= 0)");
    return S3R_OK;
}

int soft_shape(int batch, int channels, int height, int width, int max_disp, int out_height, int out_width) {
    if (s3r::disparity_soft_lds_bytes(channels, max_disp, width) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "soft read-out: 4*(2*C*W + 2*W*min(max_disp, W) + 12*W) bytes must fit 64 KiB of LDS");
    if (too_large({batch, channels, height, width}, 1) || too_large({batch, out_height, out_width}, 1)) return elems_fail();
    if ((int64_t)batch * out_height >= (1 << 24))      // at most one workgroup of 256 per output row: < 2^32 work-items
        return fail(S3R_ERR_INVALID, "batch x out_height must stay below 2^24: split the batch");
    return S3R_OK;
}

int disp_loss_dims(int batch, int64_t pixels, float beta) {
    if (!(beta >= 0.f) || !std::isfinite(beta))
        return fail(S3R_ERR_INVALID, "disparity loss: beta must be finite and >= 0 (got %g)", (double)beta);
    if (batch < 0 || pixels <= 0)
        return fail(S3R_ERR_INVALID, "disparity loss dims: batch >= 0 and pixels > 0 (batch %d, pixels %lld)", batch, (long long)pixels);
    if (too_large({pixels, batch}, 4)) return elems_fail();
    return S3R_OK;
}

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

int chamfer_dims(int batch, int n, int m) {
    if (batch <= 0 || n <= 0 || m <= 0) return fail(S3R_ERR_INVALID, "chamfer needs non-empty clouds (batch=%d n=%d m=%d)", batch, n, m);
    if (batch > 65535) return batch_fail();
    return S3R_OK;
}

// (B V) of a BCE call within the header's limits
int bce_dims(int batch, int64_t voxels) {
    if (batch < 0 || voxels <= 0) return fail(S3R_ERR_INVALID, "voxel BCE dims: batch >= 0 and voxels > 0 (batch %d, voxels %lld)", batch, (long long)voxels);
    if (too_large({voxels, batch}, 4)) return too_large_fail();
    return S3R_OK;
}

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

extern "C" {

// ---------------------------------------------------------------- cost volume (s3r_pointwise.hip, s3r_pointwise_bf16.hip, s3r_cost_volume_bwd.hip)
int s3r_cost_volume_forward(const float* fl, const float* fr, float* vol, int batch, int channels, int max_disp,
                            int height, int width, int out_halo, void* stream) {
    if (!fl || !fr || !vol) return null_tensor();
    if (int rc = costvol_dims(batch, channels, max_disp, height, width)) return rc;
    const int64_t hw = (int64_t)height * width;
    if (2 * hw * 4 > 64 * 1024) return fail(S3R_ERR_INVALID, "feature plane %dx%d does not fit the LDS staging", height, width);
    if (int rc = costvol_size(batch, channels, max_disp, height, width, out_halo)) return rc;
    const int64_t out = (int64_t)batch * 2 * channels * max_disp * hw;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, (double)out, 4.0 * (2.0 * batch * channels * hw + (double)out));
    return launched(s3r::launch_cost_volume(fl, fr, vol, batch, channels, max_disp, height, width, out_halo, s), "cost volume launch");
}

int s3r_cost_volume_forward_wino(const float* fl, const float* fr, float* planes, int batch, int channels, int max_disp,
                                 int height, int width, void* stream) {
    if (!fl || !fr || !planes) return null_tensor();
    if (batch <= 0 || channels <= 0 || max_disp <= 0 || height < 4 || width <= 0 || (height & 3))
        return fail(S3R_ERR_INVALID, "bad cost-volume shape for the Winograd layout (height a multiple of 4: F(4,3) groups)");
    if (int rc = costvol_wino_fits(max_disp, height, width)) return rc;
    const int64_t elems = 6 * (int64_t)batch * 2 * channels * (max_disp + 2) * (height / 4) * (width + 2);
    if (elems * 4 >= ((int64_t)1 << 31)) return fail(S3R_ERR_INVALID, "Winograd planes of %lld floats exceed 2 GiB: split the batch", (long long)elems);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, 2.0 * batch * channels * (double)max_disp * height * width,
                 4.0 * batch * channels * (2.0 * height * width) + 4.0 * (double)elems);
    return launched(s3r::launch_cost_volume_wino(fl, fr, planes, batch, channels, max_disp, height, width, 4, s),
                    "cost volume (Winograd layout) launch");
}

int s3r_cost_volume_forward_wino2(const float* fl, const float* fr, float* planes, int batch, int channels, int max_disp,
                                  int height, int width, void* stream) {
    if (!fl || !fr || !planes) return null_tensor();
    if (batch <= 0 || channels <= 0 || max_disp < 4 || height < 4 || width <= 0 || (height & 3) || (max_disp & 3))
        return fail(S3R_ERR_INVALID, "bad cost-volume shape for the two-axis Winograd layout (height and max_disp multiples of 4: F(4,3) groups)");
    if (int rc = costvol_wino_fits(max_disp, height, width)) return rc;
    const int64_t elems = 36 * (int64_t)batch * 2 * channels * (max_disp / 4) * (height / 4) * (width + 2);
    if (elems * 4 >= ((int64_t)1 << 31)) return fail(S3R_ERR_INVALID, "two-axis Winograd planes of %lld floats exceed 2 GiB: split the batch", (long long)elems);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, 2.0 * batch * channels * (double)max_disp * height * width,
                 4.0 * batch * channels * (2.0 * height * width) + 4.0 * (double)elems);
    return launched(s3r::launch_cost_volume_wino2(fl, fr, planes, batch, channels, max_disp, height, width, s),
                    "cost volume (two-axis Winograd layout) launch");
}

int s3r_cost_volume_forward_bf16(const void* fl, const void* fr, void* vol, int batch, int channels, int max_disp,
                                 int height, int width, int out_halo, void* stream) {
    if (!fl || !fr || !vol) return null_tensor();
    if (misaligned16(fl)) return bf16_align_fail("the left bf16 features", fl);
    if (misaligned16(fr)) return bf16_align_fail("the right bf16 features", fr);
    if (misaligned16(vol)) return bf16_align_fail("the bf16 cost volume", vol);
    if (int rc = costvol_dims(batch, channels, max_disp, height, width)) return rc;
    if (channels % 8 != 0) return fail(S3R_ERR_INVALID, "bf16 cost volume needs channels %% 8 == 0");
    if (int rc = costvol_size(batch, channels, max_disp, height, width, out_halo)) return rc;
    const int64_t hw = (int64_t)height * width, out = (int64_t)batch * 2 * channels * max_disp * hw;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_COSTVOL, 0, (double)out, 2.0 * (2.0 * batch * channels * hw + (double)out));
    return launched(s3r::launch_cost_volume_bf16(fl, fr, vol, batch, channels, max_disp, height, width, out_halo, s), "cost volume launch (bf16)");
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
    if (!grad_volume) return null_tensor();
    hipStream_t s = (hipStream_t)hip_stream;
    const double dn = max_disp < width ? max_disp : width;
    const double terms = dn * (dn + 1.0) / 2.0 + (width - dn) * dn;      // sum over w of n_L(w) = sum over w of n_R(w)
    const double sides = (grad_left ? 1.0 : 0.0) + (grad_right ? 1.0 : 0.0);
    const double rows = (double)batch * channels * height;
    ProfScope ps(s, F_COSTVOL, 1, 2.0 * sides * rows * terms, 4.0 * ((double)vol + sides * rows * width));
    return launched(s3r::launch_cost_volume_backward(grad_volume, grad_left, grad_right, batch, channels, max_disp, height, width, s),
                    "cost volume backward launch");
}

// ---------------------------------------------------------------- disparity read-outs, metrics and loss (s3r_disparity*.hip)
int s3r_disparity_wta(const float* feat_l, const float* feat_r, float* disp_l, float* disp_r, int batch, int channels,
                      int height, int width, int max_disp, void* stream) {
    if (!feat_l || !feat_r || !disp_l || !disp_r) return null_tensor();
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || max_disp <= 0)
        return fail(S3R_ERR_INVALID, "disparity dims must be positive");
    if ((size_t)2 * channels * width * sizeof(float) > 64 * 1024)
        return fail(S3R_ERR_INVALID, "disparity read-out: a feature row pair (2*C*W floats) must fit 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_DISP, 0, 0.0, 4.0 * (double)batch * height * width * (2.0 * channels + 2.0));
    return launched(s3r::launch_disparity_wta(feat_l, feat_r, disp_l, disp_r, batch, channels, max_disp, height, width, s),
                    "disparity read-out launch");
}

int s3r_disparity_epe(const float* pred, const float* gt, float* epe, int32_t* count, int batch, int64_t pixels,
                      void* stream) {
    if (!pred || !gt || !epe || !count) return null_tensor();
    if (batch <= 0 || pixels <= 0) return fail(S3R_ERR_INVALID, "epe dims must be positive");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_DISP, 1, 0.0, 8.0 * batch * (double)pixels);
    return launched(s3r::launch_disparity_epe(pred, gt, epe, count, batch, pixels, s), "epe launch");
}

int s3r_disparity_soft(const void* feat_l, const void* feat_r, int feat_dtype, float* disp_l, float* disp_r, float* conf_l,
                       float* conf_r, int batch, int channels, int height, int width, int max_disp, float temperature,
                       int out_height, int out_width, float disp_scale, void* stream) {
    if (int rc = soft_args(batch, channels, height, width, max_disp, temperature, out_height, out_width)) return rc;
    if (feat_dtype != S3R_F32 && feat_dtype != S3R_BF16) return fail(S3R_ERR_INVALID, "unknown feature dtype %d", feat_dtype);
    const bool bf16 = feat_dtype == S3R_BF16;
    if (bf16 && channels % 8 != 0) return fail(S3R_ERR_INVALID, "bf16 channels-last features need channels %% 8 == 0");
    if (bf16 && batch > 0 && (misaligned16(feat_l) || misaligned16(feat_r)))
        return fail(S3R_ERR_INVALID, "bf16 features must start 16-byte aligned (16-byte loads)");
    if (int rc = soft_shape(batch, channels, height, width, max_disp, out_height, out_width)) return rc;
    if (batch == 0) return S3R_OK;
    if (!feat_l || !feat_r) return fail(S3R_ERR_INVALID, "null feature pointer");
    const double feat = (double)batch * channels * height * width, out = (double)batch * out_height * out_width;
    hipStream_t s = (hipStream_t)stream;
    const int maps = !!disp_l + !!disp_r + !!conf_l + !!conf_r;
    ProfScope ps(s, F_DISP, 2, 0.0, (bf16 ? 2.0 : 4.0) * 2.0 * feat + 4.0 * maps * out);
    return launched(s3r::launch_disparity_soft(feat_l, feat_r, bf16, disp_l, disp_r, conf_l, conf_r, batch, channels, max_disp,
                                               height, width, temperature, out_height, out_width, disp_scale, s),
                    "soft disparity read-out launch");
}

int s3r_disparity_metrics(const float* pred, const float* gt, float* epe, int32_t* counts, int batch, int64_t pixels,
                          void* stream) {
    if (batch < 0 || pixels < 0) return fail(S3R_ERR_INVALID, "metrics dims must be >= 0 (batch %d, pixels %lld)", batch,
                                             (long long)pixels);
    if (batch > 65535) return batch_fail();
    if (too_large({pixels, batch}, 1)) return elems_fail();
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !epe || !counts) return null_tensor();
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_DISP, 3, 0.0, 8.0 * batch * (double)pixels + 20.0 * batch);
    return launched(s3r::launch_disparity_metrics(pred, gt, epe, counts, batch, pixels, s), "disparity metrics launch");
}

int s3r_disparity_soft_backward(const void* feat_l, const void* feat_r, int feat_dtype, const float* grad_disp_l,
                                const float* grad_disp_r, float* grad_left, float* grad_right, int batch, int channels, int height,
                                int width, int max_disp, float temperature, int out_height, int out_width, float disp_scale,
                                void* hip_stream) {
    if (!grad_disp_l && !grad_disp_r)
        return fail(S3R_ERR_INVALID, "soft read-out backward: grad_disp_l and grad_disp_r are both NULL (either may be: it counts as zeros)");
    if (!grad_left && !grad_right)
        return fail(S3R_ERR_INVALID, "soft read-out backward: grad_left and grad_right are both NULL (either may be: it is not computed)");
    if (int rc = soft_args(batch, channels, height, width, max_disp, temperature, out_height, out_width)) return rc;
    if (feat_dtype == S3R_BF16)
        return fail(S3R_ERR_INVALID, "soft read-out backward: bf16 features have no backward (fp32 NCHW features only)");
    if (feat_dtype != S3R_F32) return fail(S3R_ERR_INVALID, "unknown feature dtype %d", feat_dtype);
    if (int rc = soft_shape(batch, channels, height, width, max_disp, out_height, out_width)) return rc;
    if ((int64_t)batch * height >= (1 << 24))          // one workgroup of 256 per feature row: < 2^32 work-items
        return fail(S3R_ERR_INVALID, "batch x height must stay below 2^24: split the batch");
    if (batch == 0) return S3R_OK;
    if (!feat_l || !feat_r) return fail(S3R_ERR_INVALID, "null feature pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const double feat = (double)batch * channels * height * width, out = (double)batch * out_height * out_width;
    const int grads = !!grad_disp_l + !!grad_disp_r, outs = !!grad_left + !!grad_right;
    ProfScope ps(s, F_DISP, 4, 0.0, 4.0 * (2.0 * feat + grads * out + outs * feat));
    return launched(s3r::launch_disparity_soft_backward((const float*)feat_l, (const float*)feat_r, grad_disp_l, grad_disp_r, grad_left,
                                                        grad_right, batch, channels, max_disp, height, width, temperature, out_height,
                                                        out_width, disp_scale, s), "soft disparity read-out backward launch");
}

int s3r_disparity_loss_forward(const float* pred, const float* gt, float beta, float* loss_sum, int32_t* count, float* loss_elem,
                               int batch, int64_t pixels, void* hip_stream) {
    if (int rc = disp_loss_dims(batch, pixels, beta)) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !loss_sum || !count) return null_tensor();
    hipStream_t s = (hipStream_t)hip_stream;
    ProfScope ps(s, F_DISP, 5, 0.0, 4.0 * ((double)batch * (double)pixels * (loss_elem ? 3.0 : 2.0) + 2.0 * batch));
    return launched(s3r::launch_disparity_loss(pred, gt, beta, loss_sum, count, loss_elem, batch, pixels, s), "disparity loss launch");
}

int s3r_disparity_loss_backward(const float* pred, const float* gt, const float* grad_scale, float beta, float* grad_pred, int batch,
                                int64_t pixels, void* hip_stream) {
    if (int rc = disp_loss_dims(batch, pixels, beta)) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !gt || !grad_scale || !grad_pred) return null_tensor();
    hipStream_t s = (hipStream_t)hip_stream;
    ProfScope ps(s, F_DISP, 6, 0.0, 4.0 * (3.0 * batch * (double)pixels + batch));
    return launched(s3r::launch_disparity_loss_backward(pred, gt, grad_scale, beta, grad_pred, batch, pixels, s), "disparity loss backward launch");
}

// ---------------------------------------------------------------- stereo augmentation (s3r_augment.hip)
int64_t s3r_augment_scratch_elems(const s3r_augment_desc* d, int batch, int height, int width) {
    if (int rc = augment_shape(d, batch, height, width)) return rc;
    return s3r::augment_scratch(d, batch, (int64_t)height * width);
}

int s3r_augment_pair(const s3r_augment_desc* d, const uint8_t* left, const uint8_t* right, const int64_t* sample_ids,
                     const float* disp_left, const float* disp_right, float* out_left, float* out_right,
                     float* out_disp_left, float* out_disp_right, int batch, int height, int width,
                     float* scratch, int64_t scratch_elems, void* hip_stream) {
    if (int rc = augment_shape(d, batch, height, width)) return rc;
    if (!left || !right || !sample_ids) return fail(S3R_ERR_INVALID, "augment: null left, right or sample_ids");
    if (!out_left || !out_right) return fail(S3R_ERR_INVALID, "augment: null out_left or out_right");
    const int given = (disp_left != nullptr) + (disp_right != nullptr) + (out_disp_left != nullptr) + (out_disp_right != nullptr);
    if (given != 0 && given != 4)
        return fail(S3R_ERR_INVALID, "augment: disp_left, disp_right, out_disp_left and out_disp_right must be all NULL or all given");
    const int64_t px = (int64_t)batch * height * width, need = s3r::augment_scratch(d, batch, (int64_t)height * width);
    if (need > 0)      // (S3R_ERR_INVALID, not _WORKSPACE: kept as ABI 8 answers)
        if (int rc = need_scratch(S3R_ERR_INVALID, "augment: contrast", need, "s3r_augment_scratch_elems", scratch, scratch_elems)) return rc;
    const Span outs[5] = {{out_left, 12 * px, "out_left"}, {out_right, 12 * px, "out_right"}, {out_disp_left, 4 * px, "out_disp_left"},
                          {out_disp_right, 4 * px, "out_disp_right"}, {need > 0 ? scratch : nullptr, 4 * need, "scratch"}};
    const Span ins[5] = {{left, d->channels * px, "left"}, {right, d->channels * px, "right"}, {sample_ids, 8 * (int64_t)batch, "sample_ids"},
                         {disp_left, 4 * px, "disp_left"}, {disp_right, 4 * px, "disp_right"}};
    if (int rc = check_overlaps("augment", outs, 5, ins, 5)) return rc;
    return launched(s3r::launch_augment_pair(d, left, right, sample_ids, disp_left, disp_right, out_left, out_right, out_disp_left,
                                             out_disp_right, batch, height, width, scratch, (hipStream_t)hip_stream), "augment launch");
}

// ---------------------------------------------------------------- Chamfer distance (s3r_chamfer.hip)
int s3r_chamfer_forward(const float* p, const float* q, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                        int batch, int n, int m, void* stream) {
    if (!p || !q || !dist1 || !dist2 || !idx1 || !idx2) return null_tensor();
    if (int rc = chamfer_dims(batch, n, m)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_CHAMFER, 0, 2.0 * 8.0 * batch * (double)n * m, 4.0 * batch * (5.0 * n + 5.0 * m));
    return launched(s3r::launch_chamfer(p, q, dist1, dist2, idx1, idx2, batch, n, m, s), "chamfer launch");
}

int s3r_chamfer_backward(const float* p, const float* q, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                         const float* grad_dist2, float* grad_p, float* grad_q, int batch, int n, int m, void* stream) {
    if (!p || !q || !idx1 || !idx2) return null_tensor();
    if (!grad_dist1 && !grad_dist2) return fail(S3R_ERR_INVALID, "chamfer backward: grad_dist1 and grad_dist2 are both NULL (one may be: it means zeros)");
    if (!grad_p && !grad_q) return fail(S3R_ERR_INVALID, "chamfer backward: grad_p and grad_q are both NULL (one may be: it is not computed)");
    if (int rc = chamfer_dims(batch, n, m)) return rc;
    if (too_large({3, batch, n > m ? n : m}, 1)) return elems_fail();
    hipStream_t s = (hipStream_t)stream;
    // per computed direction: 7 per target (one doubling, 3 differences, 3 products: the own term) + 10 per source (one doubling, 3
    // differences, 3 products, 3 adds: every source scatters one term); the index compares of the scan are not counted
    const double B = batch, N = n, M = m;
    const double flops = B * ((grad_p ? 7.0 * N + 10.0 * M : 0.0) + (grad_q ? 7.0 * M + 10.0 * N : 0.0));
    const double elems = 3.0 * (N + M) + (N + M) + (grad_dist1 ? N : 0.0) + (grad_dist2 ? M : 0.0) + (grad_p ? 3.0 * N : 0.0) +
                         (grad_q ? 3.0 * M : 0.0);
    ProfScope ps(s, F_CHAMFER, 1, flops, 4.0 * B * elems);
    return launched(s3r::launch_chamfer_backward(p, q, idx1, idx2, grad_dist1, grad_dist2, grad_p, grad_q, batch, n, m, s),
                    "chamfer backward launch");
}

// ---------------------------------------------------------------- voxel IoU and BCE (s3r_pointwise.hip, s3r_voxel_loss.hip)
int s3r_voxel_iou(const float* pred, const float* gt, float threshold, float* iou, int batch, int64_t voxels,
                  void* stream) {
    if (!pred || !gt || !iou) return null_tensor();
    if (batch <= 0 || voxels <= 0) return fail(S3R_ERR_INVALID, "iou dims must be positive");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_IOU, 0, 0.0, 8.0 * batch * (double)voxels);
    return launched(s3r::launch_iou(pred, gt, threshold, iou, batch, voxels, s), "iou launch");
}

int s3r_voxel_bce_forward(const float* pred, const float* target, float* loss_sum, float* loss_elem, int batch, int64_t voxels,
                          void* stream) {
    if (!loss_sum && !loss_elem)
        return fail(S3R_ERR_INVALID, "voxel BCE: loss_sum and loss_elem are both NULL (one may be: it is not written)");
    if (int rc = bce_dims(batch, voxels)) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !target) return null_tensor();
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_IOU, 1, 0.0, 4.0 * ((double)batch * (double)voxels * (loss_elem ? 3.0 : 2.0) + (loss_sum ? batch : 0)));
    return launched(s3r::launch_voxel_bce(pred, target, loss_sum, loss_elem, batch, voxels, s), "voxel BCE launch");
}

int s3r_voxel_bce_backward(const float* pred, const float* target, const float* grad_scale, float* grad_pred, int batch,
                           int64_t voxels, void* stream) {
    if (int rc = bce_dims(batch, voxels)) return rc;
    if (batch == 0) return S3R_OK;
    if (!pred || !target || !grad_scale || !grad_pred) return null_tensor();
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(s, F_IOU, 2, 0.0, 4.0 * (3.0 * batch * (double)voxels + batch));
    return launched(s3r::launch_voxel_bce_backward(pred, target, grad_scale, grad_pred, batch, voxels, s), "voxel BCE backward launch");
}

// ---------------------------------------------------------------- surface point clouds (s3r_surface_points.hip)
int64_t s3r_voxel_surface_points_scratch_elems(int batch, int depth, int height, int width) {
    if (int rc = surface_shape(batch, depth, height, width)) return rc;
    return s3r::surface_points_scratch(batch, (int64_t)depth * height * width);
}

int s3r_voxel_surface_points(const float* occupancy, float threshold, const int64_t* sample_ids, uint64_t seed, float* points,
                             int32_t* n_faces, int batch, int depth, int height, int width, int n_points, float* scratch,
                             int64_t scratch_elems, void* hip_stream) {
    if (int rc = surface_shape(batch, depth, height, width)) return rc;
    if (!occupancy || !sample_ids || !points) return fail(S3R_ERR_INVALID, "surface points: null occupancy, sample_ids or points");
    if (n_points <= 0) return fail(S3R_ERR_INVALID, "surface points: n_points = %d must be positive", n_points);
    if ((int64_t)batch * n_points * 3 >= kMaxElems)
        return fail(S3R_ERR_INVALID, "surface points: batch * n_points * 3 must be below 2^31: split the batch");
    if (!std::isfinite(threshold)) return fail(S3R_ERR_INVALID, "surface points: the threshold must be finite");
    const int64_t V = (int64_t)depth * height * width, need = s3r::surface_points_scratch(batch, V);
    // (S3R_ERR_INVALID, not _WORKSPACE: kept as ABI 8 answers)
    if (int rc = need_scratch(S3R_ERR_INVALID, "surface points:", need, "s3r_voxel_surface_points_scratch_elems", scratch, scratch_elems)) return rc;
    const Span outs[3] = {{points, 12 * (int64_t)batch * n_points, "points"}, {n_faces, 4 * (int64_t)batch, "n_faces"},
                          {scratch, 4 * need, "scratch"}};
    const Span ins[2] = {{occupancy, 4 * (int64_t)batch * V, "occupancy"}, {sample_ids, 8 * (int64_t)batch, "sample_ids"}};
    if (int rc = check_overlaps("surface points", outs, 3, ins, 2)) return rc;
    return launched(s3r::launch_surface_points(occupancy, threshold, sample_ids, seed, points, n_faces, batch, depth, height, width, n_points,
                                               scratch, (hipStream_t)hip_stream), "surface points launch");
}

}  // extern "C"
