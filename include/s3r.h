/* s3r.h — C-ABI of libs3r_hip.so: the MI355X (gfx950) forward path of the Stereo2Voxel /
 * Stereo2Point network.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * What each entry point replaces on the reference side (the reference's model code lives on the
 * unmounted Stereo2Voxel / Stereo2Point branches, /root/reference/README.md:5, so the most specific
 * citation the mount supports is given):
 *
 *   s3r_conv_forward, s3r_encoder_forward   the torch conv2d+BatchNorm+ReLU calls inside the stereo
 *                                           feature encoder's nn.Module.forward        (README.md:5,73-74)
 *   s3r_encoder_forward_u8                  the same fed with the 8-bit renders the PNG decode yields: replaces the
 *                                           dataset transform's uint8 -> float32 / 255 as well (requirements.txt:5)
 *   s3r_cost_volume_forward                 the per-disparity shift/subtract Python loop that builds the
 *                                           disparity cost volume                       (README.md:75-76)
 *   s3r_cost_volume_backward                torch autograd's backward of that loop (slice assignments of differences): what
 *                                           `python3 runner.py` runs behind the loss between decoder and encoder (README.md:75-76)
 *   s3r_decoder_forward (+conv/deconv/head) the torch conv3d / ConvTranspose3d + BN + ReLU + sigmoid
 *                                           calls of the voxel decoder                  (README.md:77)
 *   s3r_linear_forward                      the point decoder's nn.Linear layers        (README.md:36)
 *   s3r_linear_backward                     torch autograd's backward of those layers: what `python3 runner.py` (training, the
 *                                           reference's default mode) runs behind the Chamfer loss   (README.md:36)
 *   s3r_chamfer_forward                     extensions/chamfer_dist (the reference's one native op,
 *                                           built by `python setup.py install`)         (README.md:64-65)
 *   s3r_chamfer_backward                    the backward half of the same extension: the op is usable as a LOSS, with a fixed
 *                                           summation order instead of the usual atomicAdd scatter   (README.md:64-65)
 *   s3r_voxel_iou                           the IoU metric of `runner.py --test`        (README.md:88-92)
 *   s3r_voxel_bce_forward / _backward       torch.nn.BCELoss on the sigmoid occupancy grid and its autograd backward: the loss the
 *                                           reference family trains voxel grids with (`python3 runner.py`), with a fixed summation
 *                                           order                                       (README.md:77)
 *   s3r_head_backward                       torch autograd's backward of the occupancy head's conv3d(64 -> 1, k = 1) + bias + sigmoid:
 *                                           one pass over the grid, fixed summation orders, no atomics   (README.md:77)
 *   s3r_conv_backward (+ s3r_conv_adjoint_desc) torch autograd's backward of a conv3d / ConvTranspose3d + BN + activation block of the voxel
 *                                           decoder: what `python3 runner.py` runs behind the loss for the up-path (README.md:77)
 *   s3r_stem_backward                       torch autograd's backward of the encoder's first conv2d + BN + ReLU block with respect to its
 *                                           parameters, from the 8-bit or fp32 renders in their two tensors: with s3r_conv_backward on
 *                                           the other seven blocks, what `python3 runner.py` runs behind the loss for the encoder (README.md:5,73-74)
 *   s3r_batchnorm_train_forward / _backward torch.nn.BatchNorm2d/3d in TRAINING mode (batch statistics) + activation and its autograd
 *                                           backward: what trains bn.weight / bn.bias of the conv + BN + ReLU blocks   (README.md:77)
 *   s3r_disparity_wta, s3r_disparity_epe    predicted left / right disparity and its end-point error
 *                                           against the disp_%02d_{l,r}.exr ground truth (README.md:75-76)
 *   s3r_disparity_soft                      the same prediction as a sub-pixel soft-argmin, upsampled to the
 *                                           ground truth's render resolution, with a confidence map   (README.md:75-76)
 *   s3r_disparity_metrics                   the end-point error and bad-pixel rates (>1 px, >3 px, KITTI D1) of a
 *                                           stereo evaluation against those maps        (README.md:75-76)
 *   s3r_disparity_soft_backward             torch autograd's backward of that read-out (abs, softmax, bilinear upsample) down to the two
 *                                           feature maps: what `python3 runner.py` runs behind a disparity loss (README.md:75-76)
 *   s3r_disparity_loss_forward / _backward  torch.nn.SmoothL1Loss on the pixels with a valid ground truth (the disp_%02d_{l,r}.exr maps
 *                                           mark background as inf or negative) and its backward, fixed summation order (README.md:75-76)
 *   s3r_optim_step (+ s3r_optim_state_init, torch.optim.SGD / Adam / AdamW's step and torch.nn.utils.clip_grad_norm_: the parameter update
 *   s3r_optim_set_lr, its scratch query)    of `python3 runner.py` (training), with a defined rounding order and its step count, powers
 *                                           and learning rate on the device                (README.md:36,77)
 *   s3r_augment_pair (+ its scratch query)  the input augmentation of `python3 runner.py` (training) on 8-bit stereo renders, the
 *                                           disparity maps shifted along; the transform set is INVENTED by this build (README.md:36,77)
 *   s3r_voxel_surface_points (+ its         the ground-truth clouds of `python3 runner.py --variant point` on a dataset tree: points drawn on
 *   scratch query)                          the exposed faces of the 32^3 occupancy grids; the sampling rule is INVENTED by this build (README.md:36,77)
 *
 * Conventions
 *   - every tensor is fp32, contiguous, NCHW / NCDHW, resident in device memory owned by the caller;
 *     the library never allocates, frees or synchronises;
 *   - `stream` is a hipStream_t (NULL = the default stream); work is enqueued, not waited for;  every entry point can be
 *     stream-captured into a HIP graph and replayed on new data in the same buffers; the event profiler must be off while capturing;
 *   - return value: S3R_OK (0) or a negative s3r_status; s3r_last_error() gives a message for the
 *     calling thread; nothing throws across the ABI;
 *   - every tensor of one call must be < 2^31 elements and < 4 GiB (32-bit buffer offsets);
 *   - alignment: an fp32 or int32 tensor needs 4-byte alignment, at every entry point and for every argument (activations,
 *     weights, packed weights, scale / shift / bias, scratch, workspaces, outputs, indices, counts), and the result does not depend
 *     on the address: the same bits at a 4-byte-aligned pointer as at a 256-byte-aligned one (carving x, y, scratch and ws out of one
 *     arena at float granularity is fine).  A bf16 tensor must be 16-byte aligned at every entry that takes or writes one, and so
 *     must the scratch of an S3R_BF16 layer call and the workspace of a chain with S3R_BF16 layers (they hold bf16 intermediates);
 *     channels-last with channels % 8 == 0 keeps every sample and pixel boundary 16-byte aligned.  Render tensors must be 16-byte
 *     aligned, fp32 and 8-bit alike (the stems fetch whole render rows 16 bytes at a time).  A pointer that breaks one of these is
 *     refused with S3R_ERR_INVALID and a message that contains "16-byte aligned", before anything is enqueued.  Nothing needs more:
 *     not 128, not 256 bytes;
 *   - size queries (s3r_conv_scratch_elems, s3r_chain_workspace_elems, ...) do not depend on the device they are asked on: launch
 *     forms of one algorithm (bit-identical among themselves) are planned against the current device's compute-unit count and have
 *     different scratch footprints, so whenever the LIBRARY picks the form the query is sized for the largest one (r06).  A process
 *     with no device (host-only planning) plans launches for an unpartitioned MI355X (256 CUs).
 */
#ifndef S3R_H
#define S3R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 8 (r05) over ABI 7: s3r_conv_desc grew `dilation`, `out_pad`, `act_param` and three activations — the parameter-general
 * fp32 layers; `tile` = 6 under S3R_ALGO_WINOGRAD names the three-axis form of a transposed convolution (AUTO takes it from edge
 * 16 up: other bits than ABI 7 for such a layer); s3r_profile_detail and record family 10 (aux passes).
 * s3r_disparity_soft and s3r_disparity_metrics were added later as new entry points only (no struct or existing signature changed):
 * the version stays 8.  s3r_chamfer_backward and s3r_linear_backward (+ its scratch query) likewise; s3r_voxel_bce_forward,
 * s3r_voxel_bce_backward and s3r_head_backward (+ its scratch query) likewise; s3r_conv_adjoint_desc and s3r_conv_backward (+ its scratch
 * query) likewise; s3r_cost_volume_backward likewise; s3r_batchnorm_train_forward and s3r_batchnorm_train_backward (+ their scratch queries)
 * likewise; s3r_stem_backward (+ its scratch query) likewise; s3r_disparity_soft_backward, s3r_disparity_loss_forward and
 * s3r_disparity_loss_backward likewise; s3r_optim_step, s3r_optim_state_init, s3r_optim_set_lr and s3r_optim_scratch_elems (with their two
 * structs) likewise; s3r_augment_pair and s3r_augment_scratch_elems (with their struct) likewise; s3r_voxel_surface_points and
 * s3r_voxel_surface_points_scratch_elems likewise: new entry points only, the version stays 8. */
#define S3R_ABI_VERSION 8

typedef enum s3r_status {
    S3R_OK = 0,
    S3R_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    S3R_ERR_HIP = -2,         /* a HIP runtime call failed (message has hipGetErrorString) */
    S3R_ERR_WORKSPACE = -3    /* workspace too small */
} s3r_status;

typedef enum s3r_op {
    S3R_OP_CONV = 0,          /* Conv2d / Conv3d (ndim selects) */
    S3R_OP_DECONV = 1,        /* ConvTranspose2d / 3d.  3D k4 s2 p1 has the tuned kernels (parity classes, Winograd forms); every
                                 other (k, stride, pad, out_pad) with dilation 1 runs as stride^ndim residue classes, each a stride-1
                                 launch of the direct kernel over a halo-padded copy (the algorithmic multiplications); dilation > 1
                                 runs zero-stuffed (stride^ndim times as many) (fp32) */
    S3R_OP_LINEAR = 2         /* nn.Linear on the flattened input */
} s3r_op;

typedef enum s3r_dtype {
    S3R_F32 = 0,              /* fp32 activations, NCHW / NCDHW, v_mfma_f32_32x32x2_f32 (exact fp32) */
    S3R_BF16 = 1              /* bf16 activations, CHANNELS-LAST (B,[D,]H,W,C), v_mfma_f32_32x32x16_bf16, fp32
                                 accumulate; the stem still reads fp32 NCHW renders and the occupancy head still
                                 writes fp32 probabilities */
} s3r_dtype;

typedef enum s3r_act { S3R_ACT_NONE = 0, S3R_ACT_RELU = 1, S3R_ACT_SIGMOID = 2,
                       S3R_ACT_LEAKY_RELU = 3, S3R_ACT_ELU = 4, S3R_ACT_TANH = 5 /* ABI 8: fp32 convolution layers only */ } s3r_act;

/* Memory layout of an activation buffer (beyond NCHW vs channels-last, which the dtype fixes):
 *   S3R_LAYOUT_PLAIN   the (halo-padded) tensor as described under "Halos" below;
 *   S3R_LAYOUT_WINO_H  fp32 path, INPUT of a 3 x 3 [x 3] stride-1 pad-1 convolution only, in_halo 1, edge n a multiple of 4: the six
 *                      Winograd F(4,3)-along-H plane sets of the halo-padded tensor, (6, B, C, [n+2,] n/4, n+2) — set i, row q =
 *                      the i-th F(4,3) input-transform combination of the padded rows 4 q .. 4 q + 5 (csrc/s3r_kernels.h,
 *                      wino_rows_to_classes).  What s3r_cost_volume_forward_wino writes: the consumer then skips its input
 *                      transform.  The batch of such a call is bounded: s3r_conv_wino_input_elems returns 0 when the layer /
 *                      batch cannot take it.
 * (Value 1 was S3R_LAYOUT_S2D — parity-split intermediates for stride-2 consumers, bf16 and fp32 forms — through ABI 6: built,
 * bit-identical, measured slower / no gain inside the forward in rounds 2 and 3, never planned by default; removed in ABI 7.) */
/*   S3R_LAYOUT_WINO_DH the same for the TWO-AXIS kernel (Conv3d k3 s1 p1, edge a multiple of 4): 36 plane sets of
 *                      36 B C (n/4) (n/4) (n+2) floats, in memory (36, B, C, n/4, n+2, n/4) — depth group s, PADDED COLUMN, row
 *                      group q, the row group fastest —, set 6 a + b = depth class a, row class b of the 6 x 6 window of padded
 *                      depths 4 s .. 4 s + 5 and padded rows 4 q .. 4 q + 5 (rows first, then depths).  A buffer in this layout IS
 *                      the output of s3r_cost_volume_forward_wino2, its only producer (there is no transform entry for it), and
 *                      the consumer relies on that: C is two halves of a cost volume of edge n, masked as that call masks them,
 *                      and the class GEMM never reads the K tiles that hold only the mask's zeros (csrc/s3r_cv_live.h).  Anything
 *                      else written there is not read as such: a value placed in a masked region may be ignored.  The layer's
 *                      weights must be finite: an infinite weight times a structural zero was NaN where the tile was multiplied
 *                      and is 0 where it is left out.
 *   S3R_LAYOUT_WINO_HW the two-axis kernel's input in 2D (Conv2d k3 s1 p1, edge n a multiple of 4): (36, C, P) with the positions
 *                      of the whole batch flat, P = B (n/4)^2 rounded up to a multiple of 64, position (b, q, s); set 6 a + b =
 *                      column class a, row class b of the 6 x 6 window of padded rows 4 q .. 4 q + 5 and padded columns
 *                      4 s .. 4 s + 5 (rows first, then columns).  It is also the one OUTPUT layout other than PLAIN: a
 *                      two-axis Conv2d whose consumer is another one writes these plane sets of its own (halo-1) output from
 *                      its finish kernel — s3r_chain_forward plans that hand-off itself (e6 -> e7 of this network).
 *   S3R_LAYOUT_WINO_3D the operand of ANY 3D two-axis layer exactly as that layer's own input transform lays it out, partial last
 *                      groups included: (ncls, B, C, G, G, n + 2 h) with h = in_halo = pad — Conv3d k3 s1 p1: ncls 36, G =
 *                      ceil(n / 4), windows of padded depths / rows 4 s .. 4 s + 5; Conv3d k4 s1 p0: ncls 25, G = ceil((n - 3) / 2),
 *                      windows 2 s .. 2 s + 4; rows and depths beyond the padded tensor read as 0.  As an OUTPUT layout it is the
 *                      same tensor written by the producer in place of its plain activation, which then does not exist; out_halo
 *                      (1 / 0) says which of the two consumers it is for.
 *   S3R_LAYOUT_DIFF    the operand of the Winograd form of a ConvTranspose3d k4 s2 p1 (in_halo 1): (4, B, C, n+2, n+2, n+2) — the
 *                      halo-padded plain tensor x, then Dh[z][r] = x[z][r] - x[z][r+1], Dd[z][r] = x[z][r] - x[z+1][r] and
 *                      Ddh[z][r] = Dh[z][r] - Dh[z+1][r] over the whole padded volume (0 in the last row / depth).  As an OUTPUT
 *                      layout: the four tensors written by the producer (out_halo 1).
 *                      Both are written by ONE pass that replaces the producer's finish pass and the consumer's operand pass — a
 *                      split-K direct convolution, a class-parallel two-axis Conv3d or a class-parallel transposed Winograd layer
 *                      in front of such a consumer — with the bits the two passes give.  s3r_chain_forward plans these hand-offs
 *                      itself (v4 -> v5 -> v6 -> d1 -> d2 of this network) where both layers' algorithms and launch forms allow it;
 *                      a single-layer call that asks for one its launch form cannot serve fails with S3R_ERR_INVALID. */
typedef enum s3r_layout { S3R_LAYOUT_PLAIN = 0, S3R_LAYOUT_WINO_H = 2, S3R_LAYOUT_WINO_DH = 3, S3R_LAYOUT_WINO_HW = 4,
                          S3R_LAYOUT_WINO_3D = 5, S3R_LAYOUT_DIFF = 6 } s3r_layout;

/* Which convolution algorithm a layer's forward runs (ABI 7).  The fp32 3 x 3 [x 3] stride-1 pad-1 convolutions and the
 * transposed convolutions have two kernels — the direct implicit GEMM and a Winograd form with 1/2 .. 9/16 of the
 * multiplications (csrc/s3r_wino.h and its units) — that agree to fp32 rounding, NOT bit for bit.  So the choice is part of the
 * descriptor and never depends on anything else a caller passes (workspace size, batch):
 *   S3R_ALGO_AUTO      the library's policy, a function of the layer's PER-SAMPLE geometry only: Winograd where the layer has
 *                      that form (fp32 Conv k3 s1 p1 with cin % 32 == 0, cout > 1, edge >= 4; ConvTranspose3d k4 s2 p1 over an
 *                      edge that is a multiple of 4, cin % 32 == 0; in_halo = 1, no sigmoid); direct otherwise, and direct whenever the descriptor
 *                      forces a direct-kernel tile / split-K (tile >= 0 or ksplit >= 1) or a non-plain layout.  The
 *                      process-level override S3R_WINO=0 (AUTO never picks Winograd) is read ONCE, when the library is loaded;
 *   S3R_ALGO_DIRECT    the direct kernel;
 *   S3R_ALGO_WINOGRAD  the Winograd kernel (S3R_ERR_INVALID if the layer has no such form or the descriptor cannot take it:
 *                      needs in_halo = 1, plain layouts — or S3R_LAYOUT_WINO_H input —, no split-K, no sigmoid).  `tile` >= 0 then
 *                      forces the launch FORM of the one-axis kernel (tuning / tests; every form gives the same bits, and the
 *                      library picks among them by batch): 0 serial, 1 class-parallel, 2 dual (bulk serial + remainder
 *                      class-parallel in one launch); `tile` = 6 (ABI 8): the THREE-AXIS form of a ConvTranspose3d k4 s2 p1 over an edge
 *                      of 8, 16 or 32 (F(2,2) along D, H and W: 27 / 64 of the multiplications; AUTO takes it from edge 16 up;
 *                      7 / 8 force its class-parallel / serial launch form: same bits, the library picks by batch); `tile` = 3: the TWO-AXIS algorithm (Conv3d k3 s1 p1 as F(4,3) x F(4,3) over D
 *                      and H, Conv2d k3 s1 p1 as F(4,3) x F(4,3) over H and W, Conv3d k4 s1 p0 as F(2,4) x F(2,4); in_halo = pad;
 *                      4 / 5 force its class-parallel / semi-fused launch form: same bits) — another algorithm, other bits than
 *                      the one-axis kernel; AUTO takes it for every stride-1 layer that has it and an edge <= 28 (e6, e7, v1, v3,
 *                      v5, v6 of this network).  Two of its finish kernels stage PADDED output planes in 64 KiB of LDS, which bounds
 *                      the edge n together with out_halo: the Conv2d form (tile 3, 4, 5) serves n <= 124 with n + 2 out_halo <= 128
 *                      (one plane), the semi-fused Conv3d form (tile 5) n <= 60 with n + 2 out_halo <= 64 (four slices).  The
 *                      class-parallel Conv3d form (tile 4) has no such bound, and the library's own pick (tile 3 or -1) takes it
 *                      for a Conv3d outside the semi-fused form's.  A descriptor outside these bounds is refused like any other
 *                      the layer has no form for: S3R_ERR_INVALID from s3r_conv_scratch_elems and s3r_conv_forward, nothing enqueued.
 * A call whose scratch is smaller than s3r_conv_scratch_elems says for the RESOLVED algorithm fails with S3R_ERR_WORKSPACE; it
 * is never answered with the other kernel's bits. */
typedef enum s3r_algo { S3R_ALGO_AUTO = 0, S3R_ALGO_DIRECT = 1, S3R_ALGO_WINOGRAD = 2 } s3r_algo;

/* One layer's geometry.  Spatial sizes are cubic/square: `in_size` per axis, `ndim` axes.
 *
 * Halos.  The MFMA convolution kernels read their zero padding from memory: an activation may be
 * stored with a ZERO HALO of `halo` elements on every spatial axis, i.e. as a contiguous
 * (B, C, n+2*halo, ...) tensor whose border is zero and whose interior is the logical (B, C, n, ...)
 * tensor.  `in_halo` / `out_halo` describe the buffers `x` / `y` of s3r_conv_forward.  A layer with
 * padding p (or a ConvTranspose) served by the MFMA kernel needs in_halo >= p (>= 1); kernels write
 * interiors only, so a buffer zeroed once keeps its halo.  Three writers store whole padded rows instead (whole 128-byte lines:
 * partial lines cost a read-modify-write) and so rewrite the halo rows / columns of the planes they write with +0.0, the value
 * the halo holds: the two-axis Winograd Conv2d (its finish kernel), the semi-fused launch form of the two-axis Conv3d k3 s1 p1
 * (its finish kernel stores whole padded depth slices) and the fp32 s3r_cost_volume_forward.  None ever writes anything but +0.0
 * there; the first and the last never touch a halo PLANE (depth) of a 3D output, the semi-fused Conv3d form rewrites those of its
 * output with +0.0 too.  (The plain tensor inside an S3R_LAYOUT_DIFF output is written
 * whole, every halo element with +0.0: that layout exists between two layers of a chain only.)  s3r_chain_forward plans the halos of all
 * intermediates itself and pads an unpadded chain input on the fly. */
typedef struct s3r_conv_desc {
    int32_t op;        /* s3r_op */
    int32_t ndim;      /* 2 or 3 (ignored for LINEAR) */
    int32_t batch;     /* B */
    int32_t cin, cout;
    int32_t in_size;   /* input edge (H=W[=D]) */
    int32_t k, stride, pad;
    int32_t act;       /* s3r_act */
    int32_t tag;       /* caller's label, echoed by the profiler */
    int32_t tile;      /* -1: library picks; >=0 (tuning): S3R_F32 direct kernel: MFMA tile cfg 0..7 + 16*gather_width (algo =
                          WINOGRAD: the launch form, see s3r_algo); S3R_BF16: 1,2,4 per-tap gather x128 positions (3: 128x128
                          couts; +16: 32-channel K tiles), 9,10 row-reuse gather, 5,6 / 21,22 plane-reuse gather (64- / 32-channel
                          K tiles), 23 plane-reuse 256x128 couts, 40 row-persistent (e2's geometry) */
    int32_t in_halo;   /* zero halo of the input buffer  (elements per spatial axis side) */
    int32_t out_halo;  /* zero halo of the output buffer */
    int32_t ksplit;    /* 0: library picks; >=1: force the split-K factor (must divide cin/16; bf16: cin/32) */
    int32_t dtype;     /* s3r_dtype: which path (layout + matrix instruction) the layer runs on */
    int32_t in_layout; /* s3r_layout of the input buffer: PLAIN, or the plane sets a producer wrote for this layer's Winograd kernel —
                          WINO_H (one-axis), WINO_DH (two-axis Conv3d), WINO_HW (two-axis Conv2d): in_halo must be 1 for those;
                          WINO_3D (any two-axis Conv3d, in_halo = pad), DIFF (transposed Winograd form, in_halo 1) */
    int32_t out_layout;/* s3r_layout of the output buffer: PLAIN, WINO_HW (a two-axis Conv2d writing its consumer's plane sets), or
                          WINO_3D / DIFF (a 3D layer writing its consumer's operand from its finish pass) */
    int32_t algo;      /* s3r_algo (ABI 7): AUTO = the library's geometry-only policy */
    /* ABI 8 — parameter-general layers (fp32 path).  The shapes this build's network has keep their tuned kernels; any other
     * (k, stride, pad, dilation) convolution with cin % 16 == 0 runs the direct kernel; everything else listed here goes through
     * the direct kernel too: cin % 16 != 0 behind a staged copy (channels zero-padded to 16; cin <= 8: unfolded so that every tap
     * of every channel is a K row, in sub-batches of <= 1 GiB), ConvTranspose2d / 3d with any k / stride / pad / output padding
     * (dilation 1: one stride-1 launch per output residue class, reading a halo of ceil(k / stride) — the producer's, when in_halo
     * provides it and cin % 16 == 0, else a halo-padded copy's; k == stride, pad 0: one GEMM with a depth-to-space store;
     * dilation > 1: the input zero-stuffed at the stride, the kernel flipped), LeakyReLU with a slope in [0, 1] inside the direct
     * kernel's epilogue, ELU / Tanh / other slopes as a pass of their own behind the layer.  0 / 0 / 0.f are NOT the neutral
     * values of `dilation`: a zero-initialised ABI-7 descriptor means dilation 1 and is read so. */
    int32_t dilation;  /* >= 1 (0 is read as 1) */
    int32_t out_pad;   /* ConvTranspose output_padding (< max(stride, dilation)) */
    float act_param;   /* S3R_ACT_LEAKY_RELU: negative slope; S3R_ACT_ELU: alpha (S3R_OP_LINEAR descriptors take the three too: a pass behind
                          the layer; the flat s3r_linear_forward entry, which has no parameter argument, takes none / relu / sigmoid) */
} s3r_conv_desc;

/* One layer of a stage: geometry + its packed weights + folded epilogue vectors (device pointers). */
typedef struct s3r_layer {
    s3r_conv_desc desc;
    const void* packed_w;    /* from s3r_conv_pack_weights (fp32 or bf16 image, per desc.dtype) */
    const float* scale;      /* [cout] gamma/sqrt(var+eps)            (NULL = 1) */
    const float* shift;      /* [cout] beta + (bias-mean)*scale       (NULL = 0) */
} s3r_layer;

int s3r_abi_version(void);
const char* s3r_last_error(void);

/* output edge of a layer: conv (n+2p-k)/s+1, deconv (n-1)s-2p+k, linear 1 */
int s3r_conv_out_size(const s3r_conv_desc* d);
/* size of the packed weight buffer for a layer IN 4-BYTE UNITS (>= the torch weight's numel on the fp32
 * path: couts are padded; about half of it on the bf16 path).  An fp32 3 x 3 [x 3] stride-1 pad-1 convolution packs every
 * form it has: the direct slab, the six Winograd F(4,3)-along-H class slabs (csrc/s3r_wino_axis1.hip: half the
 * multiplications) and the 36 slabs of the two-axis form (2D over H, W; 3D over D, H; a 3D k4 valid layer its 25); which kernel a forward
 * runs is the descriptor's `algo` (s3r_algo above).  The transposed convolutions likewise: 72 F(2,2) x F(2,2) (parity class, class) slabs
 * behind the direct ones. */
int s3r_conv_packed_elems(const s3r_conv_desc* d, int64_t* elems);
/* repack a torch-layout weight (Conv: [cout][cin][k..]; ConvTranspose: [cin][cout][k..]; Linear:
 * [cout][cin]) into the kernel's K-major layout.  Device to device, on `stream`. */
int s3r_conv_pack_weights(const s3r_conv_desc* d, const float* w, void* packed, void* stream);
/* floats of scratch s3r_conv_forward needs for this layer under its resolved algorithm: split-K partial slabs (direct
 * kernel), the transformed input and the class-parallel slabs (Winograd kernel); 0 when it needs none */
int64_t s3r_conv_scratch_elems(const s3r_conv_desc* d);
/* y = act(conv(x) * scale + shift); dispatches to the stem / MFMA / head kernel by shape.  `scratch` must hold
 * s3r_conv_scratch_elems floats: a smaller one is S3R_ERR_WORKSPACE, never a silent switch to another kernel or another
 * split (ABI 6 ran such a layer unsplit / on the direct kernel: other bits for the same descriptor). */
int s3r_conv_forward(const s3r_conv_desc* d, const void* x, const void* packed_w, const float* scale,
                     const float* shift, void* y, float* scratch, int64_t scratch_elems, void* stream);

/* Run a chain of layers x -> y.  Every intermediate activation gets its own region of `ws`
 * (s3r_chain_workspace_elems floats; with 288 GB of HBM nothing is recycled), laid out with the halo
 * the next layer wants.  layers[0].desc.in_halo / layers[n-1].desc.out_halo describe x / y; the halos
 * of the intermediates are planned by the library (the descriptors' values are ignored for them).
 * `ws_fresh` != 0 makes the call zero the workspace first: pass 1 the first time a (chain, batch,
 * workspace) combination is used — or whenever anything else wrote to `ws` — and 0 afterwards.
 * A layer may read its input in another geometry than its producer wrote (a linear layer's features as a (C, n, n) map, or a
 * conv's output as fewer channels over a larger edge): such an input carries no halo.  A consumer behind such a reshape stages its
 * own padded copy where it has one (staged and unfolded layers, residue-class ConvTranspose); one that reads its zero padding from
 * the producer's halo — a cin % 16 == 0 direct convolution with pad > 0, the Winograd forms, the tuned ConvTranspose3d k4 s2 p1 —
 * is refused (S3R_ERR_INVALID).  Linear and head layers write no halo either: the same holds behind them. */
int64_t s3r_chain_workspace_elems(const s3r_layer* layers, int n_layers);
int s3r_chain_forward(const s3r_layer* layers, int n_layers, const void* x, void* y, float* ws, int64_t ws_elems,
                      int ws_fresh, void* stream);

/* Stage entry points (thin, shape-checked views of s3r_chain_forward):
 *   encoder: renders -> features (N,C,28,28), N = layers[0].desc.batch = 2B images: the B left renders
 *            (B,3,224,224) at `images_left`, the B right renders at `images_right` — two tensors, as the
 *            reference's forward receives them (README.md:73-74); the shared-weight tower runs once over all 2B
 *            images and the first kernel picks its source by image index, so nothing is concatenated.
 *            images_right = NULL: `images_left` holds all N images (any N).
 *            images_left and images_right must be 16-byte aligned (also for s3r_chain_forward and s3r_conv_forward on the stem).
 *   decoder: cost volume (B,2C,D,H,W) -> occupancy (B,32,32,32)  */
int s3r_encoder_forward(const s3r_layer* layers, int n_layers, const float* images_left, const float* images_right,
                        void* features, float* ws, int64_t ws_elems, int ws_fresh, void* stream);
int s3r_decoder_forward(const s3r_layer* layers, int n_layers, const void* volume, float* occupancy, float* ws,
                        int64_t ws_elems, int ws_fresh, void* stream);

/* The encoder on 8-BIT renders: (B,3,224,224) uint8 NCHW, as the reference's PNG decode yields them (OpenCV,
 * /root/reference/requirements.txt:5; README.md:73-74) — a quarter of the bytes across PCIe and into the first kernel.
 * The stem scales a sample by 1/255 as it reads it, with the single rounding of the host conversion
 * float32(u) / float32(255) it replaces: the features equal, bit for bit, those of s3r_encoder_forward on renders
 * converted that way on the host.  Everything else as s3r_encoder_forward (both precisions; images_right may be NULL). */
int s3r_encoder_forward_u8(const s3r_layer* layers, int n_layers, const uint8_t* images_left, const uint8_t* images_right,
                           void* features, float* ws, int64_t ws_elems, int ws_fresh, void* stream);

/* Hand-off from the bf16 path to an fp32 consumer (s3r_linear_forward on the latent, s3r_disparity_wta on the features):
 * x channels-last bf16 (batch, positions, channels) -> y fp32 (batch, channels, positions), exact. */
int s3r_channels_last_to_f32(const void* x, float* y, int batch, int channels, int64_t positions, void* stream);

/* vol[b,c,d,h,w] = L[b,c,h,w]-R[b,c,h,w-d] (w>=d), vol[b,C+c,d,h,w] = R[b,c,h,w]-L[b,c,h,w+d] (w+d<W), else 0.
 * `out_halo` > 0 writes the interior of a (B,2C,D+2h,H+2h,W+2h) buffer whose halo the caller zeroed. */
int s3r_cost_volume_forward(const float* feat_left, const float* feat_right, float* volume, int batch, int channels,
                            int max_disp, int height, int width, int out_halo, void* stream);

/* The volume written directly as the S3R_LAYOUT_WINO_H input of the 3D convolution that consumes it (halo 1):
 * (6, B, 2C, D+2, H/4, W+2) floats (F(4,3) groups), bit-identical to the input transform of the padded volume; the caller
 * zeroed the buffer once (the depth-halo planes are never written).  height a multiple of 4. */
int s3r_cost_volume_forward_wino(const float* feat_left, const float* feat_right, float* planes, int batch, int channels,
                                 int max_disp, int height, int width, void* stream);
/* floats of the S3R_LAYOUT_WINO_H input of layer `d` (in_halo = 1) if a forward of it would run the Winograd kernel under the
 * library's current policy (S3R_WINO) and the batch fits one call; 0 otherwise (hand the layer its plain input then). */
int64_t s3r_conv_wino_input_elems(const s3r_conv_desc* d);
/* ... and which layout that is: S3R_LAYOUT_WINO_H (the one-axis kernel), S3R_LAYOUT_WINO_DH (the two-axis kernel), or
 * S3R_LAYOUT_PLAIN (none: hand the layer its plain halo-padded input) */
int s3r_conv_wino_input_layout(const s3r_conv_desc* d);
/* the volume as the S3R_LAYOUT_WINO_DH input of the 3D convolution that consumes it: 36 B 2C (D/4) (H/4) (W+2) floats, in memory
 * (36, B, 2C, D/4, W+2, H/4) — the column outside the row group —, each value bit-identical to the two-axis input transform of the
 * padded volume; max_disp and height multiples of 4 */
int s3r_cost_volume_forward_wino2(const float* feat_left, const float* feat_right, float* planes, int batch, int channels,
                                  int max_disp, int height, int width, void* stream);

/* the same on channels-last bf16 features (B,H,W,C) -> volume (B,D+2h,H+2h,W+2h,2C); channels % 8 == 0 */
int s3r_cost_volume_forward_bf16(const void* feat_left, const void* feat_right, void* volume, int batch, int channels,
                                 int max_disp, int height, int width, int out_halo, void* stream);

/* Backward of s3r_cost_volume_forward on the plain volume (out_halo 0): grad_volume (B, 2C, D, H, W) fp32, plain and contiguous, no halo
 * (what the adjoint layer's forward of the first 3D convolution writes); grad_left and grad_right (B, C, H, W).  With gv = grad_volume,
 * n_L(w) = min(D, w + 1) and n_R(w) = min(D, W - w):
 *   grad_left [b,c,h,w] = sum_{d = 0 .. n_L(w)-1} ( gv[b,  c,d,h,w] - gv[b,C+c,d,h,w-d] )
 *   grad_right[b,c,h,w] = sum_{d = 0 .. n_R(w)-1} ( gv[b,C+c,d,h,w] - gv[b,  c,d,h,w+d] )
 * Order, which IS the contract (bit for bit): per output element and per d the difference t_d is ONE fp32 subtraction; the accumulator
 * starts AS t_0 (not as +0.0); t_1, t_2, ... are added one at a time in ascending d, each add rounded once; nothing is fused into an FMA and
 * nothing is reassociated.  Every output is its own sequential sum: no cross-lane reduction, no atomics, no scratch — so the bits do not
 * depend on the run, on an address, on the batch a sample appears in or on the launch shape (a sample of a batch has, bit for bit, the
 * result of the B = 1 call on it).
 * Structural zeros are not read into the arithmetic: the positions of grad_volume that the forward writes as the constant 0 — left slab
 * w < d, right slab w + d >= W, every plane d >= W — appear in neither sum and are never loaded, so a NaN or an infinity there changes no
 * output bit (they are skipped, not multiplied by a mask: 0 * NaN is NaN).  A NaN or infinity at any other position propagates through
 * exactly this arithmetic: it reaches the outputs whose sums contain that position — gv[b,c,d,h,w] is in grad_left[b,c,h,w] and in
 * grad_right[b,c,h,w-d]; gv[b,C+c,d,h,w] is in grad_right[b,c,h,w] and in grad_left[b,c,h,w+d] — and no other.
 * grad_left or grad_right may be NULL: that side is not computed and the other keeps the bits of the full call; both NULL is
 * S3R_ERR_INVALID.  batch >= 0 (0 launches nothing and returns S3R_OK); channels, max_disp, height, width >= 1; the shapes
 * s3r_cost_volume_forward refuses are refused here too (a feature plane pair 2 H W floats beyond 64 KiB: no forward can have written such a
 * volume; this kernel itself uses no LDS); grad_volume < 2^31 elements.  Outputs are overwritten, never accumulated into.  4-byte alignment
 * for every argument (all accesses are single dwords).  Nothing is enqueued when the call is refused.  One kernel launch.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record of family 3, tag 1; `flops` = 2 per summed term (one subtraction, one add) of every side computed; `bytes` = one read
 * of grad_volume and one write of each gradient asked for: 4 B (2 C D H W + 2 C H W) with both. */
int s3r_cost_volume_backward(const float* grad_volume, float* grad_left, float* grad_right, int batch, int channels,
                             int max_disp, int height, int width, void* hip_stream);

/* y[b][o] = act(sum_i x[b][i] w[o][i] + bias[o]); w in torch Linear layout (no packing).  `scratch` holds the
 * split-K partial sums (s3r_linear_scratch_elems floats; reduced in a fixed order: deterministic). */
int64_t s3r_linear_scratch_elems(int batch, int cin, int cout);
int s3r_linear_forward(const float* x, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                       int act, float* scratch, int64_t scratch_elems, void* stream);

/* Backward of s3r_linear_forward's layer y = act(x W^T + bias): x (B,Cin), w (Cout,Cin) torch layout, y and grad_y (B,Cout); grad_x
 * (B,Cin), grad_w (Cout,Cin), grad_bias (Cout).  act is S3R_ACT_NONE, S3R_ACT_RELU or S3R_ACT_SIGMOID (anything else: S3R_ERR_INVALID).
 * The pre-activation gradient g (B,Cout) is fp32 with nothing fused:
 *   none: g = grad_y;   ReLU: g = (y > 0.f) ? grad_y : 0.f (a NaN y gives 0);   sigmoid: t = 1 - y; u = y * t; g = grad_y * u, each
 *   operation rounded once, in this order.
 *   grad_bias[o] = sum_b g[b][o]: ONE fp32 accumulator that starts as g[0][o], plain adds in ascending b.  This order IS the contract
 *                  (bit for bit; with B = 1 it is g itself).
 *   grad_w[o][i] = sum_b g[b][o] x[b][i]: v_mfma_f32_32x32x2_f32, b ascending inside one workgroup (no split, no scratch).
 *   grad_x[b][i] = sum_o g[b][o] w[o][i]: the same instruction, o ascending inside a K slice; the slices — a function of (cin, cout)
 *                  only, never of the device or an address — are written as slabs into `scratch` and added in ascending slice order.
 * No atomics: the same bits on every run and at every address the alignment rule allows (4 bytes, every argument).
 * grad_x, grad_w and grad_bias may each be NULL: that output is not computed and costs neither its GEMM nor its traffic (p1 behind a
 * frozen trunk needs no grad_x: 134 MB of weights not read); the computed ones carry the bits of the full call; all three NULL is
 * S3R_ERR_INVALID.  x may be NULL when grad_w is, w when grad_x is.  y may be NULL when act is none; y NULL with ReLU or sigmoid is
 * S3R_ERR_INVALID.  Outputs are overwritten, never accumulated into.  batch, cin, cout > 0; every tensor < 2^31 elements and < 4 GiB.
 * `scratch` holds g and the slabs: s3r_linear_backward_scratch_elems floats, sized for the worst case over the outputs asked for,
 * independent of the device, monotone in batch; its contents on entry do not matter; a shorter (or NULL) one is S3R_ERR_WORKSPACE.
 * Nothing is enqueued when the call is refused.  Profiler: family 4, tag 1; `flops` = 2 batch cin cout per GEMM actually run (grad_w,
 * grad_x); `bytes` = the tensors the call must read and write (grad_y; y unless act is none; x and grad_w; w and grad_x; grad_bias). */
int64_t s3r_linear_backward_scratch_elems(int batch, int cin, int cout);
int s3r_linear_backward(const float* x, const float* w, const float* y, const float* grad_y, float* grad_x, float* grad_w,
                        float* grad_bias, int batch, int cin, int cout, int act, float* scratch, int64_t scratch_elems, void* stream);

/* squared-L2 nearest neighbours both ways; p (B,N,3), q (B,M,3); dist1, idx1 (B,N): for every point of p its nearest point of q;
 * dist2, idx2 (B,M): the reverse.  The rule, which s3r_chamfer_backward's "same bits for every batch split" rests on:
 *   - the distance of a pair is ((dx*dx + dy*dy) + dz*dz) in fp32, dx = p.x - q.x and so on: eight operations, each rounded once, in
 *     this order, nothing fused;
 *   - dist is the smallest distance of the query and idx its FIRST minimum: the lowest index of the other cloud that holds that
 *     smallest distance (equal distances are common: duplicated points, points on a grid), whatever the cloud sizes — the result
 *     is that of one sequential scan in ascending index that replaces its best only on a strictly smaller distance;
 *   - minima are taken over the distances that are not NaN (IEEE minNum): a NaN distance (a NaN coordinate, inf - inf) is skipped;
 *   - a query with no candidate below +inf — its own coordinates are not finite, or every candidate's are not — gets
 *     dist = +inf, idx = 0;
 *   - inputs are expected finite.  A non-finite point is not an error here, and it cannot hide: its own distance is +inf, so
 *     it shows up as a non-finite loss (s3r.ChamferDistance: mean(dist1) + mean(dist2)), while the other points' answers are
 *     those of the cloud without it.  (torch.min, which the oracle uses, propagates NaN instead: the two differ on NaN only.) */
int s3r_chamfer_forward(const float* p, const float* q, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                        int batch, int n, int m, void* stream);

/* Backward of s3r_chamfer_forward: the gradient of sum_i grad_dist1[i] dist1[i] + sum_j grad_dist2[j] dist2[j] with respect to p and
 * q, the indices held fixed.  p (B,N,3), q (B,M,3); idx1 (B,N) into q and idx2 (B,M) into p as s3r_chamfer_forward wrote them;
 * grad_dist1 (B,N), grad_dist2 (B,M); grad_p (B,N,3), grad_q (B,M,3).  Per sample, with a_i = 2 grad_dist1[i] and c_j = 2 grad_dist2[j]
 * (both exact in fp32), per component x, y, z:
 *   grad_p[i] = a_i (p_i - q_idx1[i])  +  sum_{j ascending, idx2[j] == i}  c_j (p_i - q_j)
 *   grad_q[j] = c_j (q_j - p_idx2[j])  +  sum_{i ascending, idx1[i] == j}  a_i (q_j - p_i)
 * All arithmetic is fp32 without fused multiply-adds: the difference is rounded, then the product; the accumulator starts as the own
 * term and the scattered terms are added one at a time in ascending source index.  This fixed order IS the contract: a gather, no
 * atomics, no scratch — the same bits on every run, for every batch split, launch geometry and address (the usual atomicAdd scatter
 * depends on arrival order).  NaN / Inf in the inputs propagate through exactly this arithmetic.
 * grad_dist1 or grad_dist2 may be NULL: all zeros, the same bits as a zero tensor; both NULL is S3R_ERR_INVALID.  grad_p or grad_q
 * may be NULL: that direction is not computed (a ground-truth cloud needs no gradient); both NULL is S3R_ERR_INVALID.  Otherwise
 * validated as the forward: p, q, idx1, idx2 non-NULL, batch, n, m > 0, batch <= 65535, every tensor < 2^31 elements; 4-byte
 * alignment for every argument.  Indices are trusted to be in range; the own-term index is still clamped to [0, m-1] / [0, n-1], so a
 * garbage index never reads outside the clouds, and an out-of-range index matches no target in the scan.  One kernel launch, both
 * directions and all samples.  Profiler: family 5, tag 1; `bytes` = the tensors it must read and write; `flops`, per computed
 * direction, = 7 per target (one doubling, 3 differences, 3 products) + 10 per source (one doubling, 3 differences, 3 products, 3 adds):
 * batch (7 n + 10 m) for grad_p, batch (7 m + 10 n) for grad_q — the index compares of the scan are not counted. */
int s3r_chamfer_backward(const float* p, const float* q, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                         const float* grad_dist2, float* grad_p, float* grad_q, int batch, int n, int m, void* stream);

/* per-sample IoU of (pred > th) vs (gt > th) over `voxels` elements.  A voxel is occupied iff its value is strictly greater than
 * `threshold`, compared in fp32 — the threshold is the caller's value rounded to fp32 (0.2, 0.3 and 0.4 are not fp32 numbers: a voxel
 * holding float32(0.3) is NOT occupied at 0.3, although it is greater than the real number 0.3).  NaN is not occupied; -0.0 equals
 * +0.0; +inf is occupied at every finite threshold.  The two counts are exact integers (< 2^32); the result is
 * float32(intersection) / float32(union), both conversions round-to-nearest-even (they round from 2^24 voxels up), one fp32 division;
 * 1 when the union is empty. */
int s3r_voxel_iou(const float* pred, const float* gt, float threshold, float* iou, int batch, int64_t voxels,
                  void* stream);

/* Binary cross-entropy of an occupancy grid: torch.nn.BCELoss's per-element rule with a per-sample sum.  pred and target are (B, V)
 * fp32; target may be soft (any value in [0, 1]).  Per element, fp32, every operation rounded once, nothing fused:
 *   a = clamp(logf(p));  c = clamp(logf(1.f - p));  l = -(t * a + (1.f - t) * c);  clamp(v) = (v < -100.f) ? -100.f : v
 * logf is the device math library's (not correctly rounded: l is within a few ulp of the real value, not a bit-for-bit contract; the
 * sum's ORDER below is).  The clamp comes BEFORE the multiplication, so p = 0, t = 0 gives 0 and not 0 * -inf = NaN: p == 0, t == 1
 * gives exactly 100; p == 1, t == 0 gives exactly 100; p == t at either end gives 0.  The clamp is a compare-and-select, so a NaN
 * passes through it (fmaxf would swallow it): a NaN or out-of-range pred (p < 0 or p > 1) makes that element's l, and with it that
 * sample's loss_sum, NaN — that sample only, and it is not an error (torch.nn.BCELoss raises on an out-of-range input; this entry
 * never reads its inputs on the host).
 * loss_sum (B): the fp32 sum of the sample's V losses in a fixed order that is a function of V only — never of B, the device's
 * compute-unit count or an address — so sample b has the same bits in every batch split.  The order, which IS the contract:
 *   - the V losses are cut into chunks of 1024 consecutive elements (the last may be short; missing elements count as +0.0);
 *   - within a chunk, lane L (0..63) owns the 16 elements 256 j + 4 L + i (j = 0..3, i = 0..3) and adds them in ascending element
 *     order to a partial that starts as +0.0; the 64 partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o,
 *     o = 32, 16, 8, 4, 2, 1; v[0] is the chunk's sum;
 *   - the chunk sums are added in ascending chunk order into one accumulator that starts as chunk 0's sum.
 * loss_elem (B, V) may be NULL; otherwise it receives every l, and passing it does not change loss_sum's bits.  loss_sum may be NULL
 * when loss_elem is not; both NULL is S3R_ERR_INVALID.  One kernel launch, one workgroup per sample, no atomics, no scratch.
 * batch >= 0 (0 launches nothing and returns S3R_OK), voxels > 0, the tensors < 2^31 elements and < 4 GiB; pred and target non-NULL;
 * 4-byte alignment for every argument, the same bits at every address.  Outputs are overwritten.  Nothing is enqueued when the call is
 * refused.  Profiler: family 6, tag 1; `bytes` = pred, target, loss_elem when given, loss_sum when given. */
int s3r_voxel_bce_forward(const float* pred, const float* target, float* loss_sum, float* loss_elem, int batch, int64_t voxels,
                          void* stream);

/* Gradient of sum_b grad_scale[b] * loss_sum[b] with respect to pred: grad_pred (B, V), grad_scale (B); for the mean over all B V
 * elements a caller passes grad_output / (B V) in every grad_scale[b].  Per element, fp32, each operation rounded once, in this order:
 *   n = grad_scale[b] * (p - t);  d = max((1.f - p) * p, 1e-12f);  grad_pred = n / d      (the division is IEEE-correct)
 * which is torch's binary_cross_entropy_backward with its epsilon: elementwise, so bit for bit against a restatement.  A NaN pred gives
 * a NaN gradient in that element only.  All four pointers non-NULL; dims, limits, alignment and batch == 0 as the forward.  One kernel
 * launch.  Profiler: family 6, tag 2; `bytes` = pred, target, grad_pred and grad_scale. */
int s3r_voxel_bce_backward(const float* pred, const float* target, const float* grad_scale, float* grad_pred, int batch,
                           int64_t voxels, void* stream);

/* Backward of the pointwise head that s3r_conv_forward runs for Conv(C -> 1, k = 1) + affine + activation (the occupancy head d4):
 *   y[b][s] = act(fmaf(sum_c x[b][c][s] w[c], scale, shift))
 * x (B,C,S), w (C), scale ONE float or NULL for 1 (frozen: it gets no gradient), y and grad_y (B,S); grad_x (B,C,S), grad_w (C),
 * grad_shift (1).  Any S >= 1, not only multiples of 4.  act is S3R_ACT_NONE, S3R_ACT_RELU or S3R_ACT_SIGMOID (anything else:
 * S3R_ERR_INVALID).
 * The pre-activation gradient g (B,S) is fp32 with nothing fused:
 *   none: g = grad_y;   ReLU: g = (y > 0.f) ? grad_y : 0.f (a NaN y gives 0);   sigmoid: t = 1 - y; u = y * t; g = grad_y * u, each
 *   operation rounded once, in this order.
 *   gs = g * scale, rounded once; g itself when scale is NULL.
 *   grad_x[b][c][s] = gs[b][s] * w[c]: one multiplication (bit for bit).
 *   grad_w[c]  = sum_{b,s} gs[b][s] x[b][c][s]      grad_shift = sum_{b,s} g[b][s]
 * Summation order of grad_w[c] and grad_shift, which IS the contract (bit for bit):
 *   - a sample's S positions are cut into chunks of 512 consecutive positions (the last may be short; missing positions count as +0.0);
 *   - within a chunk, lane L (0..63) owns the 8 positions 256 j + 4 L + i (j = 0, 1; i = 0..3) and walks them in ascending position
 *     with a partial that starts as +0.0: grad_w takes partial = partial + gs * x — the product is rounded, then the add: they
 *     are NOT fused —, grad_shift takes partial = partial + g; the 64 partials are combined by the halving tree
 *     v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1; v[0] is the chunk's sum;
 *   - per sample, the chunk sums are added in ascending chunk order into a partial that starts as chunk 0's sum: a function of S only;
 *   - the per-sample partials are added into one accumulator in ascending b, starting from sample 0's.
 * The chunk sums go through `scratch`.  No atomics: the same bits on every run and at every address the alignment rule allows (4 bytes,
 * every argument; a sample's result does not depend on the batch it is in, only the final ascending-b sum does).
 * grad_x, grad_w and grad_shift may each be NULL: that output is not computed — grad_x NULL does not cost its write (268 MB at B = 32),
 * grad_w NULL does not cost the read of x; the computed ones carry the bits of the full call; all three NULL is S3R_ERR_INVALID.  x may
 * be NULL when grad_w is, w when grad_x is.  y may be NULL when act is none; y NULL with ReLU or sigmoid is S3R_ERR_INVALID.  Outputs
 * are overwritten, never accumulated into.  batch >= 0 (0 launches nothing, writes nothing and returns S3R_OK), channels, voxels > 0;
 * every tensor < 2^31 elements and < 4 GiB.
 * `scratch` holds the chunk sums: s3r_head_backward_scratch_elems floats ((channels + 1) * batch * ceil(voxels / 512)), sized for the
 * worst case over the outputs asked for, independent of the device, monotone in batch; its contents on entry do not matter; a shorter
 * (or NULL) one is S3R_ERR_WORKSPACE.  Nothing is enqueued when the call is refused.  One streaming launch plus one finish launch (none
 * for grad_x alone).  Profiler: family 2, tag 1; `flops` = 2 batch channels voxels for grad_w + batch channels voxels for grad_x;
 * `bytes` = the tensors the call must read and write (grad_y; y unless act is none; scale when given; x and grad_w; w and grad_x;
 * grad_shift). */
int64_t s3r_head_backward_scratch_elems(int batch, int channels, int64_t voxels);
int s3r_head_backward(const float* x, const float* w, const float* scale, const float* y, const float* grad_y, float* grad_x,
                      float* grad_w, float* grad_shift, int batch, int channels, int64_t voxels, int act, float* scratch,
                      int64_t scratch_elems, void* stream);

/* Backward of ONE fp32 convolution layer  y = act(conv(x, w) * scale[o] + shift[o])  — S3R_OP_CONV or S3R_OP_DECONV, 2D or 3D, any k,
 * stride, pad and output padding.  x (B,cin,n..); y, grad_y, gs (B,cout,m..); scale (cout) or NULL for 1 (frozen: it gets no gradient, as in
 * s3r_head_backward); grad_w in the layer's torch weight shape (Conv: [cout][cin][k..]; ConvTranspose: [cin][cout][k..]); grad_shift (cout).
 * The three entry points take fp32 layers with dilation 1 on plain tensors only: S3R_BF16, S3R_OP_LINEAR, dilation > 1, a layout other
 * than S3R_LAYOUT_PLAIN, a halo, or an activation other than none / ReLU / sigmoid is S3R_ERR_INVALID before anything is enqueued.
 *
 * The input gradient needs no kernel of its own: it is the FORWARD of the adjoint layer on gs, with the layer's own weight tensor read in
 * torch's layout for the other operator — no flip, no re-layout:
 *   Conv(cin -> cout, k, s, p) over edge n:          grad_x = ConvTranspose(cout -> cin, k, s, p, out_pad = (n + 2 p - k) mod s)(gs), the
 *                                                    weight [cout][cin][k..] read as a ConvTranspose weight [cin' = cout][cout' = cin][k..];
 *   ConvTranspose(cin -> cout, k, s, p, out_pad):    grad_x = Conv(cout -> cin, k, s, p)(gs), the weight [cin][cout][k..] read as a Conv
 *                                                    weight [cout' = cin][cin' = cout][k..].
 * s3r_conv_adjoint_desc (host only) fills that layer's descriptor: op swapped, cin / cout swapped, in_size = d's output edge, k / stride /
 * pad copied, out_pad by the rule above, act none, halos 0, layouts PLAIN, algo AUTO, dilation 1; batch, ndim and tag copied.  A caller
 * packs the layer's own torch-layout weight with s3r_conv_pack_weights(adj, w, ...) and runs adj as a forward on gs with scale and shift
 * NULL: s3r_conv_forward(adj, gs, packed, NULL, NULL, grad_x, ...) where adj's kernel takes an unpadded input (s3r_conv_forward says so),
 * else as a one-layer s3r_chain_forward, which pads an unpadded input itself.  grad_x then has the forward kernels' accuracy and their
 * batch-independent bits.
 *
 * s3r_conv_backward computes, in this order of dependence:
 *   g   the pre-activation gradient, s3r_linear_backward's rule, fp32, nothing fused:  none: g = grad_y;  ReLU: g = (y > 0.f) ? grad_y : 0.f
 *       (a NaN y gives 0);  sigmoid: t = 1 - y; u = y * t; g = grad_y * u — every operation rounded once, in this order;
 *   gs[b][o][.] = g * scale[o], rounded once; g itself when scale is NULL.  Bit for bit.  gs is an OUTPUT (the caller hands it to grad_x's
 *       forward call), not scratch;
 *   grad_shift[o] = sum_{b, pos} g[b][o][pos], bit for bit, in the head backward's order (s3r_head_backward above) with channel o's S = m^ndim
 *       positions of a sample in place of the sample's: chunks of 512 consecutive positions, lane L owns the 8 positions 256 j + 4 L + i
 *       and adds them in ascending position to a partial that starts as +0.0, the halving tree over the 64 partials, the chunk sums in
 *       ascending chunk order per sample starting from chunk 0's, the per-sample partials in ascending b starting from sample 0's;
 *   grad_w[a][f][t] = sum_{b, q over the coarse grid} A[b][a][q] * F[b][f][q * s - p + t]  (per axis; F reads 0 outside its grid), where the
 *       coarse grid is the Conv's output or the ConvTranspose's input — Conv: A = gs, F = x; ConvTranspose: A = x, F = gs — on
 *       v_mfma_f32_32x32x2_f32.  The sum over (b, q) is cut into slices that are a function of the layer's PER-SAMPLE geometry only — never
 *       of B, the device or an address; a slice never spans two samples, and inside one q ascends.  The slices are written as slabs into
 *       `scratch`, and a finish kernel adds them in ascending (sample, slice) order: per element, a sample's slabs in ascending slice order
 *       starting from its slab 0, then the per-sample partials in ascending b starting from sample 0's.  So: no atomics; the same bits on
 *       every run, at every 4-byte-aligned address and with any scratch contents on entry; a sample's partial is the same in every batch it
 *       appears in (grad_w of a batch equals, bit for bit, the ascending fp32 sum of the B = 1 results of its samples).
 *       Coarse positions, channels and taps beyond the tensors are loaded from clamped addresses and replaced by 0 in BOTH operands (0 * NaN
 *       would be NaN); they add +0.0 to accumulators that started as +0.0, which changes no bit.
 * gs, grad_w and grad_shift may each be NULL: that output is not computed, and the computed ones keep the bits of the full call; all three
 * NULL is S3R_ERR_INVALID.  grad_w needs gs: with gs NULL it lives in scratch.  y may be NULL when act is none (y NULL with ReLU or sigmoid:
 * S3R_ERR_INVALID), x when grad_w is.  Outputs are overwritten, never accumulated into.  batch >= 0 (0 launches nothing and returns
 * S3R_OK; the query returns 0); every tensor < 2^31 elements and < 4 GiB.
 * `scratch`: s3r_conv_backward_scratch_elems floats (gs, the chunk sums, the slabs), sized for the worst case over the outputs asked for,
 * independent of the device, monotone in batch; a shorter (or NULL) one is S3R_ERR_WORKSPACE.  Nothing is enqueued when the call is refused.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record of family 0 whose tag is S3R_CONV_BACKWARD_TAG + d->tag (a layer's forward record keeps d->tag; under
 * s3r_profile_detail(1) the prep pass and the two finish passes get family-10 records of the same tag nested inside it); `flops` =
 * 2 B Q Ca Cf k^ndim when grad_w is computed (Q coarse positions per sample), else 0; `bytes` = the tensors the call must read and write
 * (grad_y; y unless act is none; scale when given; gs when given; x and grad_w; grad_shift). */
#define S3R_CONV_BACKWARD_TAG 1000000
int s3r_conv_adjoint_desc(const s3r_conv_desc* d, s3r_conv_desc* adj);
int64_t s3r_conv_backward_scratch_elems(const s3r_conv_desc* d);
int s3r_conv_backward(const s3r_conv_desc* d, const float* x, const float* y, const float* grad_y, const float* scale, float* gs,
                      float* grad_w, float* grad_shift, float* scratch, int64_t scratch_elems, void* hip_stream);

/* Backward of the STEM, the encoder's first layer  y = act(conv2d(X, w; 3 -> 32, k 3, stride 2, pad 1) * scale[o] + shift[o]):  its weight and
 * shift gradients, read from the renders as the forward reads them.  X is the render: fp32 taken as is (renders_u8 = 0), or 8-bit
 * (renders_u8 != 0) scaled as the forward scales it, the correctly rounded float32(u) / float32(255).  in_size is any edge >= 1, the output
 * edge m = (in_size - 1) / 2 + 1.  Images [0, n_left) are read from images_left (n_left,3,in_size,in_size), images [n_left, n_images) from
 * images_right; images_right NULL: all images are in images_left and n_left must equal n_images.  y, grad_y (n_images,32,m,m) fp32; scale
 * (32) or NULL for 1 (frozen, as in s3r_conv_backward); grad_w (32,3,3,3), torch's weight shape; grad_shift (32).  act is S3R_ACT_NONE or
 * S3R_ACT_RELU.  There is no gs output and no input gradient (s3r_conv_backward serves a caller who wants one for fp32 renders).
 *   g, gs           s3r_conv_backward's: none: g = grad_y;  ReLU: g = (y > 0.f) ? grad_y : 0.f (a NaN y gives 0);  gs = g * scale[o], rounded
 *                   once; g itself when scale is NULL;
 *   grad_shift[o] = sum_{image, pos} g, bit for bit, in s3r_conv_backward's order (the head backward's) with S = m^2 positions per (image,
 *                   channel) row: chunks of 512 consecutive positions, lane L owns the 8 positions 256 j + 4 L + i and adds them in
 *                   ascending position to a partial that starts as +0.0, the halving tree over the 64 partials, the chunk sums in ascending
 *                   chunk order per image starting from chunk 0's, the images in ascending index starting from image 0's: the SAME bits
 *                   s3r_conv_backward returns on the converted, concatenated renders (it is a pass of its own over grad_y and y, run by
 *                   the same kernels);
 *   grad_w[o][ci][kh][kw] = sum_{image, oh, ow} gs[image][o][oh][ow] * X[image][ci][2 oh - 1 + kh][2 ow - 1 + kw], X = 0 outside the image,
 *                   on v_mfma_f32_32x32x2_f32 (M = the 32 channels, N = the 27 taps padded to 32, K = positions; each product rounded
 *                   once and added to the running sum, an fmaf chain).
 * Order of grad_w's sum, which IS the contract.  An image's output rows are cut into K slices of r = ceil(m / 32) consecutive rows (the
 * last may be short): a function of m only, never of n_images, n_left, the render type, the device or an address.  A slice never spans two
 * images; one wave owns it and adds its positions in ascending (oh, ow) to 32 x 27 sums that start as +0.0.  A finish launch adds, per
 * element, an image's slices in ascending slice order starting from slice 0's; a second adds the images' partials in ascending image index
 * starting from image 0's (either is skipped when it has one term).  So: no atomics; the same bits on every run, at every address the
 * alignment rule allows and with any scratch contents on entry; an image's partial is the same in every batch it appears in — grad_w of a
 * batch equals, bit for bit, the ascending fp32 sum of the single-image results; the result is the same whether the renders arrive as one
 * tensor or two, and the same for 8-bit renders and for their host conversion.  Positions beyond a row and elements outside an image are
 * loaded from clamped addresses and replaced by 0 in BOTH operands (0 * NaN would be NaN).
 * grad_w and grad_shift may each be NULL: that output is not computed, and the other keeps the bits of the full call; both NULL is
 * S3R_ERR_INVALID.  y may be NULL when act is none (y NULL with ReLU: S3R_ERR_INVALID).  Outputs are overwritten, never accumulated into.
 * Render pointers must be 16-byte aligned, as for the forward; every other pointer needs 4-byte alignment only.  n_images >= 0 (0 launches
 * nothing, writes nothing and returns S3R_OK; the query returns 0); n_left outside [1, n_images] with two tensors, or != n_images with one,
 * in_size < 1, an activation other than none / ReLU, a tensor >= 2^31 elements or >= 4 GiB: S3R_ERR_INVALID.
 * `scratch`: s3r_stem_backward_scratch_elems floats (the chunk sums, the slabs, the per-image partials), sized for the worst case over the
 * outputs asked for, independent of the device, monotone in n_images; a shorter (or NULL) one is S3R_ERR_WORKSPACE.  Nothing is enqueued
 * when the call is refused.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record, family 1 (stem), tag 1; `flops` = 2 n_images m^2 32 27 when grad_w is computed, else 0; `bytes` = the tensors the call
 * must read and write (grad_y; y unless act is none; the renders, scale and grad_w when grad_w is computed; grad_shift). */
int64_t s3r_stem_backward_scratch_elems(int n_images, int in_size);
int s3r_stem_backward(const void* images_left, const void* images_right, int n_left, int renders_u8, const float* y, const float* grad_y,
                      const float* scale, float* grad_w, float* grad_shift, int n_images, int in_size, int act, float* scratch,
                      int64_t scratch_elems, void* hip_stream);

/* Train-mode BatchNorm (batch statistics) + activation on z (B,C,S) fp32, plain and contiguous; S (`positions`) is the product of the
 * spatial extents, so one entry serves 2D and 3D layers.  gamma, beta, save_mean, save_var, save_invstd, grad_gamma, grad_beta are (C).
 * With N = B S and nf = (float)N (rounded to nearest when N > 2^24), per channel c, in fp32, EVERY operation rounded on its own — the
 * product is rounded, then the add: nothing is fused, so a numpy restatement is exact:
 *   mean[c]   = (sum_{b,s} z) / nf
 *   var[c]    = (sum_{b,s} d * d) / nf,  d = z - mean[c], d * d rounded before the add: the BIASED variance, in two passes over z — there
 *               is no sum of z^2, so data with |mean| >> std do not cancel;
 *   invstd[c] = 1.f / sqrtf(var[c] + eps)          (the division and the square root are IEEE-correct)
 *   xhat = (z - mean[c]) * invstd[c];  t = xhat * gamma[c];  u = t + beta[c];  y = act(u)
 *   act: S3R_ACT_NONE: u;  S3R_ACT_RELU: (u < 0.f) ? 0.f : u (a NaN stays a NaN);  S3R_ACT_SIGMOID: 1.f / (1.f + exp(-u)) with the fast
 *   exponential of the forward kernels (not correctly rounded: y is then NOT bit for bit against a restatement; the rest is).  Anything else
 *   is S3R_ERR_INVALID.
 * s3r_batchnorm_train_backward takes the forward's z, y, save_mean, save_invstd and the output gradient grad_y (B,C,S):
 *   g the pre-activation gradient, s3r_linear_backward's rule:  none: g = grad_y;  ReLU: g = (y > 0.f) ? grad_y : 0.f (a NaN y gives 0);
 *   sigmoid: t = 1 - y; u = y * t; g = grad_y * u;
 *   grad_beta[c]  = sum_{b,s} g
 *   grad_gamma[c] = sum_{b,s} g * xhat,  xhat = (z - mean[c]) * invstd[c] recomputed exactly as in the forward; the product is rounded, then added;
 *   m1 = grad_beta[c] / nf;  m2 = grad_gamma[c] / nf;  a = gamma[c] * invstd[c];  p = xhat * m2;  q = g - m1;  r = q - p;  grad_z = a * r.
 * Summation order of the four sums (z; d * d; g; g * xhat), which IS the contract (bit for bit) — s3r_head_backward's, with a (b, c) row in
 * place of a sample:
 *   - a row's S positions are cut into chunks of 512 consecutive positions (the last may be short; missing positions count as +0.0);
 *   - within a chunk, lane L (0..63) owns the 8 positions 256 j + 4 L + i (j = 0, 1; i = 0..3) and adds their terms in ascending position
 *     to a partial that starts as +0.0; the 64 partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o,
 *     o = 32, 16, 8, 4, 2, 1; v[0] is the chunk's sum;
 *   - per (b, c) row, the chunk sums are added in ascending chunk order into a partial that starts as chunk 0's sum: a function of S only;
 *   - per channel, the rows' partials are added into one accumulator in ascending b, starting from sample 0's.
 * The chunk sums go through `scratch`.  No atomics: the bits depend on the shape and the data only — not on the run, not on an address
 * (4-byte alignment suffices for every argument) and not on the scratch's contents on entry.  UNLIKE the other training entries, a sample's
 * result DOES depend on the batch it is in: mean and var are statistics of the whole batch, and y, grad_z and both sums inherit that.
 * Non-finite input: a NaN or +-inf in z poisons ITS channel's statistics — mean is NaN (+-inf for an inf), var and invstd are NaN — and with
 * them every y, grad_gamma and grad_z of that channel is NaN (grad_beta reads y and grad_y only); no other channel changes a bit.  It is not
 * an error.
 * The forward's five outputs are all required.  grad_z, grad_gamma and grad_beta may each be NULL: that output is not computed and costs no
 * write, and the computed ones keep the bits of the full call; grad_z needs both sums, which then live in scratch; all three NULL is
 * S3R_ERR_INVALID.  y may be NULL when act is none (y NULL with ReLU or sigmoid: S3R_ERR_INVALID); z, save_mean and save_invstd may be NULL
 * when grad_gamma and grad_z both are (z is then not read); gamma may be NULL when grad_z is.  Outputs are overwritten, never accumulated into.
 * batch >= 0 (0 launches nothing, writes nothing and returns S3R_OK); channels, positions >= 1; N >= 2 (one value per channel has no
 * variance: torch refuses it too); every tensor < 2^31 elements and < 4 GiB: anything else is S3R_ERR_INVALID before anything is enqueued.
 * `scratch`: s3r_batchnorm_train_forward_scratch_elems = channels * batch * ceil(positions / 512) floats (both statistics passes use them in
 * turn); s3r_batchnorm_train_backward_scratch_elems = 2 * channels * batch * ceil(positions / 512) + 2 * channels floats; functions of the
 * shape only — never of the device, the activation or the outputs asked for —, monotone in batch; a shorter (or NULL) one is
 * S3R_ERR_WORKSPACE.
 * Launches.  Forward 5: the z sums, their finish (mean), the d * d sums, their finish (var, invstd), the normalise pass — z is read three
 * times and y written once.  Backward 3: the two sums in one pass, their finish, the grad_z pass — z, y and grad_y are read twice and
 * grad_z written once; 2 launches without grad_z.  A finish is one wave per channel; it is not folded into the pass that consumes it (every
 * wave of that pass would re-add the channel's batch * ceil(positions / 512) chunk sums to stream 512 positions).
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record per call, family 2, tag 2 (forward) / 3 (backward), whose `launches` is the number of kernel launches above;
 * `flops` = 0; `bytes` = the tensor traffic the launches need: forward 4 N C * 4 B (+ the (C) vectors), backward 4 B * N C * (reads of
 * grad_y, y unless act is none, z unless only grad_beta is computed — twice with grad_z — + the grad_z write). */
int64_t s3r_batchnorm_train_forward_scratch_elems(int batch, int channels, int64_t positions);
int s3r_batchnorm_train_forward(const float* z, const float* gamma, const float* beta, float eps, int act, float* y, float* save_mean,
                                float* save_var, float* save_invstd, int batch, int channels, int64_t positions, float* scratch,
                                int64_t scratch_elems, void* hip_stream);
int64_t s3r_batchnorm_train_backward_scratch_elems(int batch, int channels, int64_t positions);
int s3r_batchnorm_train_backward(const float* z, const float* y, const float* grad_y, const float* gamma, const float* save_mean,
                                 const float* save_invstd, int act, float* grad_z, float* grad_gamma, float* grad_beta, int batch,
                                 int channels, int64_t positions, float* scratch, int64_t scratch_elems, void* hip_stream);

/* Disparity read-out: winner-take-all over the shift-and-diff costs of the cost volume (same features, same
 * |L - R shifted| costs, volume never materialised).  feat_* (B,C,H,W) fp32; disp_* (B,H,W) fp32, integer-valued,
 * in feature-resolution pixels:
 *   disp_l[b,h,w] = first argmin_{d in [0, min(max_disp-1, w)]}     sum_c |L[b,c,h,w] - R[b,c,h,w-d]|
 *   disp_r[b,h,w] = first argmin_{d in [0, min(max_disp-1, W-1-w)]} sum_c |R[b,c,h,w] - L[b,c,h,w+d]|   */
int s3r_disparity_wta(const float* feat_l, const float* feat_r, float* disp_l, float* disp_r, int batch, int channels,
                      int height, int width, int max_disp, void* stream);

/* per-sample end-point error mean|pred - gt| over the pixels with a valid ground truth (finite, >= 0), and that
 * pixel count; epe = 0 where no pixel is valid */
int s3r_disparity_epe(const float* pred, const float* gt, float* epe, int32_t* count, int batch, int64_t pixels,
                      void* stream);

/* Sub-pixel disparity read-out (a stand-in like the WTA: no learned head).  Per sample, direction and feature pixel (h, w):
 *   c(d) = the WTA's costs above, bit for bit (fp32, c ascending, |a-b| then add), d in [0, n-1], n = min(max_disp-1, w)+1 (left)
 *          or min(max_disp-1, W-1-w)+1 (right);
 *   e_d  = expf((min_d c(d) - c(d)) / temperature) (a weight that would be subnormal is 0), Z = sum e_d, S = sum d e_d, d ascending;
 *   disp = S / Z (feature pixels), conf = 1 / Z (the probability of the best disparity); max_disp = 1 gives exactly 0 and 1.
 * Output (batch, out_height, out_width) per map: at the feature size the values as they are, otherwise upsampled bilinearly with
 * torch's align_corners=False convention (src = (dst + 0.5) in / out - 0.5, clamped at 0, upper neighbour clamped at in - 1);
 * disp is then multiplied by disp_scale, conf is not.  Both directions, all samples, one kernel launch.
 * feat_dtype S3R_F32: feat_* fp32 (B,C,H,W); S3R_BF16: bf16 channels-last (B,H,W,C) as the bf16 encoder emits it, channels % 8 == 0,
 * 16-byte aligned — bf16 widens to fp32 exactly, so the result equals the S3R_F32 call on s3r_channels_last_to_f32's output bit for
 * bit.  Any of disp_l, disp_r, conf_l, conf_r may be NULL: it is not written.  LDS: 4 (2 C W + 2 W min(max_disp, W) + 12 W) bytes
 * must fit 64 KiB.  temperature finite and > 0; batch == 0 launches nothing.  Profiler: family 9, tag 2. */
int s3r_disparity_soft(const void* feat_l, const void* feat_r, int feat_dtype, float* disp_l, float* disp_r, float* conf_l,
                       float* conf_r, int batch, int channels, int height, int width, int max_disp, float temperature,
                       int out_height, int out_width, float disp_scale, void* stream);

/* Stereo metrics per sample over `pixels` elements; valid pixels as s3r_disparity_epe (ground truth finite and >= 0).
 * epe[b] equals s3r_disparity_epe's bit for bit (same fp64 order); counts[b][0..3] (int32, (B,4)) = valid pixels, |err| > 1,
 * |err| > 3, D1 (|err| > 3 and |err| > 0.05 gt, in fp64), all strict: integers, so rates pool exactly over samples and ranks.
 * batch == 0 launches nothing.  Profiler: family 9, tag 3. */
int s3r_disparity_metrics(const float* pred, const float* gt, float* epe, int32_t* counts, int batch, int64_t pixels,
                          void* stream);

/* Backward of s3r_disparity_soft: the gradient of  sum grad_disp_l * disp_l + sum grad_disp_r * disp_r  with respect to the two feature
 * maps.  feat_l, feat_r (B,C,H,W) fp32 (feat_dtype S3R_F32; S3R_BF16 is S3R_ERR_INVALID: no bf16 backward exists in the library);
 * grad_disp_l, grad_disp_r (B,OH,OW) fp32, the gradients of the two disparity maps; grad_left, grad_right (B,C,H,W).  max_disp,
 * temperature, out_height, out_width and disp_scale as in the forward call that produced the maps.  Nothing is saved by the forward: the
 * costs c(d), their minimum, the weights e_d (with the subnormal rule), Z, S and disp = S / Z are recomputed with the forward's operations
 * in the forward's order (ascending d; Z = Z + e_d, S = S + (float)d * e_d, the product rounded before the add).  The confidence maps get no
 * gradient, and there is no gradient with respect to the temperature.
 * All arithmetic is fp32, every operation rounded once, nothing contracted.  Per sample, direction X in {L, R} and feature pixel (h, w):
 *   G_X[h,w]  the feature-size gradient.  At out_height == H and out_width == W:  G = grad_disp_X[h,w] * disp_scale.  Otherwise the adjoint
 *             of the forward's bilinear blend, with the forward's source rule (i0, i1, lam)(o) = bilinear source of output index o (src =
 *             (o + 0.5) in / out - 0.5 clamped at 0, in / out one fp32 division, i0 = (int)src clamped at in - 1, i1 = i0 + 1 clamped at
 *             in - 1, lam = src - i0) and the weight with which output index o reads source index i
 *                 wt(o, i) = (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f)            (an edge-clamped i0 == i1 contributes both)
 *             gathered over the output pixels that read (h, w) — the rows oy with i0(oy) in {h - 1, h} and the columns ox with i0(ox) in
 *             {w - 1, w}, one contiguous window each — rows ascending, columns ascending within a row, into ONE accumulator that starts
 *             as +0.0:
 *                 acc = acc + ((grad_disp_X[oy,ox] * disp_scale) * wt(oy, h)) * wt(ox, w)
 *             A feature pixel that no output pixel reads (a downsample) has G = +0.0.  A NULL grad_disp_X is a tensor of zeros: G = +0.0.
 *   k = G / temperature;  p_d = e_d / Z;  t_d = p_d * (disp - (float)d);  q^X_d(h,w) = t_d * k          (IEEE divisions)
 *             (subtracting the minimum is a shift of the softmax: no term; a weight the subnormal rule flushed to 0 has p_d = 0 and q = 0)
 * and with n_L(w) = min(max_disp, w + 1), n_R(w) = min(max_disp, W - w):
 *   grad_left [b,c,h,w] = sum_{d = 0 .. n_L(w)-1} sgn(L[c,h,w] - R[c,h,w-d]) * (q^L_d(h,w) + q^R_d(h,w-d))
 *   grad_right[b,c,h,w] = sum_{d = 0 .. n_R(w)-1} sgn(R[c,h,w] - L[c,h,w+d]) * (q^R_d(h,w) + q^L_d(h,w+d))
 * Order, which IS the contract: per output element and per d the inner sum u_d is ONE add (the own direction's q first); the term is
 * (a > m) ? u_d : ((a < m) ? -u_d : 0.f) for the own feature a and the matched feature m — u_d, its negation, or 0 where the two are equal
 * (torch's abs backward; two features that do not compare, a NaN, give 0 as well); the accumulator starts AS the d = 0 term (not as +0.0)
 * and takes the others one at a time in ascending d.  Every output is its own sequential sum: no atomics, no cross-lane reduction, no
 * scratch — the same bits on every run, at every address and in every batch a sample appears in.  The sign of a zero is not part of the
 * contract.  expf is the device math library's, as in the forward (not correctly rounded: the values are not a bit-for-bit contract
 * against a restatement unless every cost of a pixel is equal — then every weight is expf(0) = 1 and all of the above is exact).
 * NaN / Inf: a non-finite value propagates through exactly this arithmetic (0.f * NaN is NaN: an output pixel with lam = 0 still hands a
 * NaN gradient to its upper neighbour, as the forward's blend hands it a NaN value); a NaN in a sample's grad_disp or features stays in
 * that sample.
 * grad_disp_l or grad_disp_r may be NULL (zeros, the same bits as a zero tensor); both NULL is S3R_ERR_INVALID.  grad_left or grad_right
 * may be NULL: that output is not computed and the other keeps the bits of the full call; both NULL is S3R_ERR_INVALID.  Outputs are
 * overwritten, never accumulated into.  Limits: the forward's, refused with the forward's messages — temperature finite and > 0, dims
 * >= 1 (batch >= 0; 0 launches nothing and returns S3R_OK), LDS 4 (2 C W + 2 W min(max_disp, W) + 12 W) bytes within 64 KiB (this kernel
 * needs 4 (2 C W + 2 W min(max_disp, W) + 2 W)), every tensor < 2^31 elements, batch x out_height < 2^24 — and batch x height < 2^24.
 * 4-byte alignment for every argument.  Nothing is enqueued when the call is refused.  One kernel launch, one workgroup per (sample,
 * feature row).
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record of family 9, tag 4; `flops` = 0; `bytes` = the features read once, each gradient given read once, each output asked
 * for written once: 4 (2 B C H W + [1 or 2] B OH OW + [1 or 2] B C H W). */
int s3r_disparity_soft_backward(const void* feat_l, const void* feat_r, int feat_dtype, const float* grad_disp_l,
                                const float* grad_disp_r, float* grad_left, float* grad_right, int batch, int channels, int height,
                                int width, int max_disp, float temperature, int out_height, int out_width, float disp_scale,
                                void* hip_stream);

/* Smooth-L1 (Huber) loss of a disparity map against a ground truth with invalid pixels.  pred, gt (B, P) fp32; a pixel is VALID exactly as
 * for s3r_disparity_metrics: its ground truth is finite and >= 0 (the EXR maps mark background as inf or a negative value; NaN is invalid).
 * Per valid element, fp32, every operation rounded once, nothing contracted, with e = pred - gt and a = |e|:
 *   a < beta:   h = 0.5f * e;  s = h * e;  l = s / beta           (IEEE division)
 *   otherwise:  l = a - 0.5f * beta                                (beta == 0: l = |e|, plain L1; a == beta takes this branch)
 * An invalid element counts as +0.0 by a SELECT: its pred and gt never enter arithmetic (not a multiplication by a mask: 0 * NaN is NaN),
 * so a NaN or an infinity of pred at an invalid pixel changes no bit.  A NaN pred at a VALID pixel compares false, takes the second branch
 * and gives a NaN l: it propagates through exactly this arithmetic into that sample's loss_sum — that sample only; it is not an error.
 * loss_sum (B): the fp32 sum of the sample's P values in s3r_voxel_bce_forward's order, a function of P only — never of B, the device or
 * an address: chunks of 1024 consecutive elements (the last may be short; missing elements count as +0.0); within a chunk lane L (0..63)
 * owns the 16 elements 256 j + 4 L + i (j = 0..3, i = 0..3) and adds them in ascending element order to a partial that starts as +0.0;
 * the 64 partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1; the chunk sums are added in
 * ascending chunk order into one accumulator that starts as chunk 0's sum.  count (B) int32: the sample's valid pixels, exact.
 * loss_elem (B, P) may be NULL; otherwise it receives every l (+0.0 at invalid pixels), and passing it changes no bit of loss_sum.
 * pred, gt, loss_sum and count non-NULL.  beta finite and >= 0; batch >= 0 (0 launches nothing and returns S3R_OK); pixels > 0; the
 * tensors < 2^31 elements and < 4 GiB; 4-byte alignment for every argument, the same bits at every address.  Outputs are overwritten.
 * Nothing is enqueued when the call is refused.  One kernel launch, one workgroup per sample, no atomics, no scratch.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record of family 9, tag 5; `bytes` = pred, gt, loss_elem when given, loss_sum and count. */
int s3r_disparity_loss_forward(const float* pred, const float* gt, float beta, float* loss_sum, int32_t* count, float* loss_elem,
                               int batch, int64_t pixels, void* hip_stream);

/* Gradient of sum_b grad_scale[b] * loss_sum[b] with respect to pred: grad_pred (B, P), grad_scale (B); for the mean over the valid pixels
 * of the batch a caller passes grad_output / max(sum_b count[b], 1) in every grad_scale[b].  Per VALID element, fp32, each operation
 * rounded once, with e = pred - gt:
 *   beta > 0:   v = e / beta;  c = (v < -1.f) ? -1.f : ((v > 1.f) ? 1.f : v);  grad_pred = grad_scale[b] * c       (clamp(e / beta, -1, 1))
 *   beta == 0:  c = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : ((e == 0.f) ? 0.f : e));  grad_pred = grad_scale[b] * c   (sgn(e))
 * and exactly +0.0 at an invalid element, by a select.  Elementwise: bit for bit against a restatement.  The clamp is two compare-and-
 * selects, so a NaN pred at a valid pixel propagates through it into that element's gradient and no other.  All four pointers non-NULL;
 * beta, dims, limits, alignment and batch == 0 as the forward.  Outputs are overwritten.  Nothing is enqueued when the call is refused.
 * One kernel launch.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new data in the same buffers).
 * Profiler: ONE record of family 9, tag 6; `bytes` = pred, gt, grad_pred and grad_scale. */
int s3r_disparity_loss_backward(const float* pred, const float* gt, const float* grad_scale, float beta, float* grad_pred, int batch,
                                int64_t pixels, void* hip_stream);

/* The optimizer step: SGD (momentum, Nesterov, L2 decay) and Adam / AdamW over a LIST of fp32 tensors, with an optional global gradient
 * norm in a fixed order (clip to max_norm; skip the step on a non-finite norm).  Deterministic, atomics-free, nothing read on the host.
 *
 * Host array.  `t` (n_tensors entries) is read during the call only.  Its pointers and sizes travel to the device BY VALUE in kernel
 * arguments, at most S3R_OPTIM_TENSORS_PER_LAUNCH tensors per launch; there is no pointer table in device memory, so nothing the device
 * dereferences can go stale, and a captured call replays as long as the tensors stay where they were.  1 <= n_tensors <=
 * S3R_OPTIM_MAX_TENSORS; more than S3R_OPTIM_TENSORS_PER_LAUNCH tensors means more launches of the same kernels.
 *
 * Device state.  `state` is S3R_OPTIM_STATE_DWORDS = 8 dwords of device memory, written by s3r_optim_state_init:
 *   0 step (int32)   1 beta1_pow   2 beta2_pow   3 lr   4 grad_norm (written)   5 clip_coef (written)   6 skipped (int32 count)   7 reserved
 * lr, the step count and the two running powers live ON THE DEVICE: a replayed graph advances its own bias correction and follows a
 * learning-rate schedule written into state[3] between replays (s3r_optim_set_lr, or any 4-byte copy).  A step that is not skipped does
 * step = step + 1 and, for Adam, beta1_pow = beta1_pow * beta1 and beta2_pow = beta2_pow * beta2 — ONE rounded fp32 multiplication per
 * step, no powf (its result is not correctly rounded and could not be restated bit for bit) — BEFORE the update reads them.
 * beta1, beta2, eps, weight_decay, max_norm, kind and flags are BAKED at enqueue time: a captured call replays with the values it was
 * captured with.  s3r_optim_state_init writes step 0, both powers 1.f, lr, grad_norm 0.f, clip_coef 1.f, skipped 0, reserved 0.
 *
 * Arithmetic.  Everything is fp32, every operation is rounded on its own (nothing contracted into a fused multiply-add), division and
 * sqrtf are the correctly rounded IEEE ones, denormals are kept.  Per element, one rounded operation per statement, with p the
 * parameter, g the gradient as read (grad is never written), mu = beta1 for SGD:
 *   with S3R_OPT_CLIP, first:      g = g * clip_coef
 *   S3R_OPT_SGD
 *     weight_decay != 0:           t = weight_decay * p;  g = g + t
 *     mu != 0, the first step:     m = g                                        (step == 1 after the advance: as torch, not mu * 0 + g)
 *     mu != 0, later steps:        a = mu * m;  m = a + g
 *     mu != 0, S3R_OPT_NESTEROV:   t = mu * m;  g = g + t;      without it: g = m
 *     then:                        t = lr * g;  p = p - t
 *     (mu == 0: m is neither read nor written and may be NULL; v is never touched by SGD)
 *   S3R_OPT_ADAM
 *     weight_decay != 0, coupled (L2, torch.optim.Adam):                t = weight_decay * p;  g = g + t
 *     weight_decay != 0, S3R_OPT_DECOUPLED_DECAY (torch.optim.AdamW):   w = lr * weight_decay;  s = w * p;  p = p - s
 *     a = beta1 * m;  b = (1.f - beta1) * g;  m = a + b
 *     a = beta2 * v;  q = g * g;  b = (1.f - beta2) * q;  v = a + b
 *     mh = m / (1.f - beta1_pow);  vh = v / (1.f - beta2_pow);  r = sqrtf(vh);  d = r + eps;  u = mh / d
 *     t = lr * u;  p = p - t
 * weight_decay == 0 skips its statements (it is not a multiplication by zero).  Elementwise: bit for bit against a restatement
 * (tests/_optim64.py), the same bits on every run and at every 4-byte-aligned address.  Without the norm, a NaN gradient propagates
 * through exactly this arithmetic and poisons only its own element (that it is a NaN is promised; its sign and payload are not).
 *
 * Gradient norm, only with S3R_OPT_CLIP or S3R_OPT_SKIP_NONFINITE: the order of s3r_head_backward's sums with a tensor in place of a row.
 * Each tensor is cut into chunks of 512 consecutive elements (the last may be short: missing elements count as +0.0); within a chunk lane
 * L (0..63) owns the eight elements 256 j + 4 L + i (j = 0, 1; i = 0..3) and adds its g * g (the product rounded, then added) in ascending
 * element order to a partial that starts as +0.0; the 64 partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o,
 * o = 32, 16, 8, 4, 2, 1.  Each tensor's chunk sums are added in ascending chunk order into a partial that starts as its chunk 0's sum; the
 * tensor totals are added in ascending tensor order into ONE accumulator that starts as tensor 0's.  grad_norm = sqrtf(total).  With
 * S3R_OPT_CLIP: d = grad_norm + 1e-6f;  c = max_norm / d;  clip_coef = (c > 1.f) ? 1.f : c (torch's clamp: a NaN stays a NaN and then
 * poisons every element, as torch.nn.utils.clip_grad_norm_ does); without it clip_coef = 1.f.  Both are written to `state` by every step
 * that computes the norm, skipped or not; a step without the norm leaves them as they were.  The norm's bits depend on the tensor list
 * only — not on how it was cut into launches, on `scratch`'s contents on entry or on any address.  A denormal g * g is kept (it is not
 * flushed to zero).
 * With S3R_OPT_SKIP_NONFINITE and a grad_norm that is not finite (NaN or infinity): no parameter, moment, step count, power or lr changes
 * by a bit; `skipped` grows by one (grad_norm and clip_coef show the offending norm).
 *
 * scratch: s3r_optim_scratch_elems(t, n_tensors) floats = sum_i ceil(elems_i / 512) + n_tensors (the chunk sums, and per tensor where
 * its chunk sums start, written by the device on every call); its contents on entry do not matter.  A step WITHOUT the norm uses no
 * scratch (it may be NULL); with the norm a shorter (or NULL) one is refused.  The query returns S3R_ERR_INVALID for a list it would refuse.
 *
 * Refused with S3R_ERR_INVALID and a message, host-side, before anything is enqueued: a NULL d, t or state; a NULL param or grad; a NULL
 * m where SGD's momentum or Adam needs it, a NULL v for Adam; elems <= 0 or >= 2^31; n_tensors <= 0 or > S3R_OPTIM_MAX_TENSORS; with the
 * norm, scratch NULL or scratch_elems below the query; a non-finite hyper-parameter, beta1 or beta2 outside [0, 1), a negative eps,
 * weight_decay or max_norm; an unknown kind or flag bit, S3R_OPT_NESTEROV without SGD momentum, S3R_OPT_DECOUPLED_DECAY without Adam;
 * param, m and v ranges of one tensor that overlap, or the same param twice in the list.  Pointers need 4-byte alignment only.
 * Launches: with the norm, one chunk-sum launch per S3R_OPTIM_TENSORS_PER_LAUNCH tensors; ONE advance launch (one wave: the ordered
 * totals, norm, coefficient, finite test, step and powers); one update launch per S3R_OPTIM_TENSORS_PER_LAUNCH tensors — three launches
 * for a list of up to 64 tensors.  Every node is a kernel (no memset, no copy).
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new gradients in the same buffers, the state advancing on the device).
 * Profiler: no record (the step is meant to be captured, and the event profiler must be off while capturing). */
#define S3R_OPTIM_TENSORS_PER_LAUNCH 64      /* 64 x (4 pointers + size) + the prefix table fit the 4 KB kernel-argument block */
#define S3R_OPTIM_MAX_TENSORS 4096
#define S3R_OPTIM_STATE_DWORDS 8
#define S3R_OPT_SGD 0
#define S3R_OPT_ADAM 1
#define S3R_OPT_DECOUPLED_DECAY 1            /* flags: AdamW's weight decay */
#define S3R_OPT_NESTEROV 2
#define S3R_OPT_CLIP 4                       /* scale the gradients by clip_coef = min(max_norm / (grad_norm + 1e-6f), 1) */
#define S3R_OPT_SKIP_NONFINITE 8             /* skip the step when grad_norm is NaN or infinite */
typedef struct s3r_optim_tensor {
    float* param;
    const float* grad;
    float* m;          /* SGD: the momentum buffer (NULL when beta1 == 0); Adam: the first moment */
    float* v;          /* Adam: the second moment; SGD: unused, may be NULL */
    int64_t elems;
} s3r_optim_tensor;
typedef struct s3r_optim_desc {
    int32_t kind;      /* S3R_OPT_SGD, S3R_OPT_ADAM */
    int32_t flags;     /* S3R_OPT_DECOUPLED_DECAY | S3R_OPT_NESTEROV | S3R_OPT_CLIP | S3R_OPT_SKIP_NONFINITE */
    float beta1;       /* SGD: momentum (0 = none; then m may be NULL) */
    float beta2, eps, weight_decay, max_norm;
} s3r_optim_desc;
int64_t s3r_optim_scratch_elems(const s3r_optim_tensor* t, int n_tensors);
/* Writes the eight dwords of a fresh state (step 0, powers 1.f, lr, grad_norm 0.f, clip_coef 1.f, skipped 0, reserved 0): one kernel
 * launch on `hip_stream` (the hipStream_t of the Conventions above; capturable).  A NULL state or a non-finite or negative lr is refused
 * with S3R_ERR_INVALID before anything is enqueued. */
int s3r_optim_state_init(float* state, float lr, void* hip_stream);
/* Writes lr into state[3], the learning rate of the steps enqueued behind it: one kernel launch on `hip_stream`, ordered like a step
 * (between two replays of a captured step it is how a schedule reaches the graph).  Refusals as s3r_optim_state_init. */
int s3r_optim_set_lr(float* state, float lr, void* hip_stream);
int s3r_optim_step(const s3r_optim_desc* d, const s3r_optim_tensor* t, int n_tensors, float* state, float* scratch,
                   int64_t scratch_elems, void* hip_stream);

/* Training-time augmentation of a stereo batch: 8-bit renders in, fp32 network inputs in [0, 1] out, with the ground-truth disparity maps
 * shifted by the same call.  Deterministic, atomics-free, nothing drawn or read on the host: a sample's result is a function of (seed,
 * sample_ids[b]) and its own pixels only — not of its batch, its position in the batch, an address or the launch shape — and a captured
 * call replays with fresh augmentation from the ids in the device buffer.  The transform set and its constants are INVENTED by this build
 * (the reference's own transforms are on unmounted branches), to be overwritten from the reference the day it is mounted.
 *
 * Tensors.  left, right (B, channels, H, W) uint8 codes at any byte alignment; channels = 3 (RGB) or 4 (RGBA, alpha composited in the
 * kernel over the drawn background).  sample_ids (B) int64 ON THE DEVICE.  out_left, out_right (B, 3, H, W) fp32, 4-byte aligned.
 * disp_left, disp_right, out_disp_left, out_disp_right: all NULL or all given, (B, H, W) fp32 maps in render pixels.  H and W are general.
 *
 * Random numbers.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), key = (seed low, seed
 * high), counter = (id low, id high, purpose, index) with id = sample_ids[b]; w0..w3 are its four output words.
 * u(w) = (float)(w >> 8) * 2^-24 (exact).  range(u, lo, hi):  t = hi - lo;  t = u * t;  lo + t.
 * Every draw is made whether or not its op is enabled: switching one op on never changes another op's draw.
 *   purpose 0, index 0:   dy = w0 % (2 max_shift + 1) - max_shift;  dx likewise from w1;  perm = w2 % 6, an index into the lexicographic
 *                         permutations of (0, 1, 2).  The modulo's bias (below 2^-18 for max_shift <= 4096) is accepted.
 *   purpose 0, index 1:   brightness = range(u(w0), ...), contrast = range(u(w1), ...), saturation = range(u(w2), ...)
 *   purpose 0, index 2:   bg[c] = bg_lo + w_c % (bg_hi - bg_lo + 1), c = 0..2
 *   purpose 1 + 3 side + c (side 0 left, 1 right; c the source channel), index y W + x:  the four noise words of that output pixel
 * All per-pair parameters are shared by the two views (the epipolar geometry and the disparity survive); only the noise is per view.
 *
 * Arithmetic.  Everything is fp32, every operation is rounded on its own (nothing contracted into a fused multiply-add), division is
 * the correctly rounded IEEE one; clamp(v) = fminf(fmaxf(v, 0), 1).  Per output pixel (y, x) of one view, over the three source channels c:
 *   1. source pixel:   sy = y - dy, sx = x - dx.  Outside the image: code = bg[c].  Inside, 3 channels: code = src[c].  Inside, 4
 *                      channels, with a = src[3]: code = (src[c] * a + bg[c] * (255 - a) + 127) / 255 in unsigned integers
 *   2. scale:          v = (float)code / 255.f
 *   3. brightness      (unless brightness_lo == brightness_hi == 1):  v = brightness * v;  v = clamp(v)
 *   4. contrast        (unless contrast_lo == contrast_hi == 1), m the pair's mean luma (below):
 *                      a = contrast * v;  t = 1.f - contrast;  b = t * m;  v = a + b;  v = clamp(v)
 *   5. saturation      (unless saturation_lo == saturation_hi == 1), l = (0.299f * v0 + 0.587f * v1) + 0.114f * v2 of the pixel after step 4:
 *                      a = saturation * v;  t = 1.f - saturation;  b = t * l;  v = a + b;  v = clamp(v)
 *   6. noise           (unless noise_sigma == 0):  s = u(w0) + u(w1);  s = s + u(w2);  s = s + u(w3);  s = s - 2.f;  s = s * 1.7320508f;
 *                      s = noise_sigma * s;  v = v + s;  v = clamp(v)      (an Irwin-Hall sum of unit variance: no logf, no cosf)
 *   7. store:          out[c'] = v[perm[c']] with S3R_AUG_PERMUTE_RGB, out[c] = v[c] without it
 * Disparity: out_disp(y, x) = disp(sy, sx) copied bit for bit inside the image (NaNs and their payloads included), +inf — the loaders'
 * invalid marker — outside it.
 *
 * The mean luma m is ONE value per pair: both views are blended towards the same grey.  The lumas l (step 5's formula) of the left and
 * of the right view after step 3 form two rows of S = H W positions, summed in the order of s3r_head_backward's sums with B = 2 rows:
 * chunks of 512 consecutive positions (the last may be short: missing positions count as +0.0); within a chunk lane L (0..63) owns the
 * eight positions 256 j + 4 L + i (j = 0, 1; i = 0..3) and adds its lumas in ascending position to a partial that starts as +0.0; the 64
 * partials are combined by the halving tree v[L] = v[L] + v[L + o] for L < o, o = 32, 16, 8, 4, 2, 1; each view's chunk sums are added in
 * ascending chunk order into a partial that starts as its chunk 0's sum; total = left + right;  m = total / (float)(2 S).
 *
 * scratch: s3r_augment_scratch_elems(d, batch, height, width) floats = 2 B ceil(S / 512) + B with contrast (the chunk sums and the
 * means), 0 without (it may be NULL); its contents on entry do not matter.  The query returns S3R_ERR_INVALID for what the call refuses.
 * Refused with S3R_ERR_INVALID and a message, host-side, before anything is enqueued: a NULL d, left, right, sample_ids, out_left or
 * out_right; disparity pointers partly given; channels not 3 or 4; batch, height or width <= 0, H W >= 2^31 or a tensor of 2^31
 * elements or more; max_shift < 0 or > 4096; an unknown flag bit; bg_lo or bg_hi outside 0..255 or bg_lo > bg_hi; a range with lo > hi,
 * negative or non-finite; noise_sigma negative or non-finite; with contrast, scratch NULL or scratch_elems below the query; outputs
 * (and the scratch) that overlap an input or each other.
 * Launches: without contrast ONE (apply); with contrast three — the chunk sums, one wave per pair writing m, then apply, which
 * recomputes steps 1-3 and stores no intermediate image.  Every node is a kernel (no memset, no copy).
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new renders and ids in the same buffers).
 * Profiler: no record (the call is meant to be captured, and the event profiler must be off while capturing). */
#define S3R_AUG_PERMUTE_RGB 1
#define S3R_AUG_MAX_SHIFT 4096
typedef struct s3r_augment_desc {
    uint64_t seed;
    int32_t  channels;            /* 3 = RGB codes, 4 = RGBA codes (alpha composited in the kernel) */
    int32_t  max_shift;           /* 0 = off */
    int32_t  flags;               /* S3R_AUG_PERMUTE_RGB = 1 */
    int32_t  bg_lo, bg_hi;        /* background codes, 0 <= lo <= hi <= 255 */
    float    brightness_lo, brightness_hi, contrast_lo, contrast_hi, saturation_lo, saturation_hi;
    float    noise_sigma;         /* in [0,1] units; 0 = off */
} s3r_augment_desc;
int64_t s3r_augment_scratch_elems(const s3r_augment_desc* d, int batch, int height, int width);
int s3r_augment_pair(const s3r_augment_desc* d, const uint8_t* left, const uint8_t* right, const int64_t* sample_ids,
                     const float* disp_left, const float* disp_right, float* out_left, float* out_right,
                     float* out_disp_left, float* out_disp_right, int batch, int height, int width,
                     float* scratch, int64_t scratch_elems, void* hip_stream);

/* Ground-truth point clouds from occupancy grids: n_points points per sample, drawn on the exposed faces of the grid's occupied voxels.
 * It is how Stereo2Point trains and validates on a StereoShapeNet tree, which holds 32^3 grids and no clouds.  Deterministic, atomics-free,
 * nothing drawn or read on the host: a sample's bits are a function of (seed, sample_ids[b], its grid, threshold, n_points) only — not of
 * its batch, its position in the batch, an address, the scratch contents on entry or the launch shape — and a captured call replays with
 * fresh clouds from the grids and ids in the device buffers.  The sampling rule is INVENTED by this build (the reference's own Stereo2Point
 * code is on unmounted branches), to be overwritten from the reference the day it is mounted.
 *
 * Tensors.  occupancy (B, D, H, W) fp32.  sample_ids (B) int64 ON THE DEVICE (8-byte aligned, as s3r_augment_pair reads them).  points
 * (B, n_points, 3) fp32, 4-byte aligned.  n_faces (B) int32, or NULL.
 *
 * Occupancy and faces.  A voxel is occupied iff v > threshold: a NaN is empty.  Face f = 2 a + side of voxel (i0, i1, i2): a is the axis
 * (0 = D, 1 = H, 2 = W), side 0 faces the lower neighbour along a, side 1 the upper one.  A face is exposed iff its voxel is occupied and
 * that neighbour is outside the grid or empty.  Exposed faces are numbered in ascending e = 6 * ((i0 * H + i1) * W + i2) + f; N is their
 * count for the sample, written to n_faces[b].
 *
 * Draws.  Point j of sample b takes Philox4x32-10 with s3r_augment_pair's multipliers, Weyl constants and u(w) = (float)(w >> 8) * 2^-24:
 * key = (seed low, seed high), counter = (id low, id high, purpose 0x100, j) with id = sample_ids[b]; w0..w3 are its output words.
 * k = (uint64)w0 * N >> 32 is the index of the point's face in the numbering above.  A prefix of a larger n_points is the smaller cloud.
 *
 * Coordinates.  inv_c = 1.f / (float)size_c (correctly rounded).  On the normal axis a:  t = (float)(i_a + side).  On the two in-plane
 * axes, in ascending axis order, with u(w1) then u(w2):  t = (float)i_c + u.  On every axis:  t = t * inv_c;  p_c = t - 0.5f.  Every
 * operation is rounded on its own (nothing contracted into a fused multiply-add).  The cloud lies in [-0.5, 0.5]^3 and component c of a
 * point is grid axis c.  A cubic grid is sampled uniformly by area; a non-cubic one uniformly by face count (its faces differ in area).
 * Empty grid: with N = 0 every point of that sample is (+0.0, +0.0, +0.0) and n_faces[b] = 0.
 * The result is integers plus three rounded operations per component: it contains no floating-point sum, so any launch structure gives
 * the same bits.
 *
 * scratch: s3r_voxel_surface_points_scratch_elems(batch, depth, height, width) floats = B (17 ceil(D H W / 64) + 1) (per 64-voxel chunk
 * its face count, then prefix, and 64 mask bytes; per sample N); its contents on entry do not matter.  The query returns S3R_ERR_INVALID
 * for the geometries the call refuses.
 * Refused with S3R_ERR_INVALID and a message, host-side, before anything is enqueued: a NULL occupancy, sample_ids or points; batch or
 * n_points <= 0; an edge outside 1..256; D H W > 2^21; batch * n_points * 3 >= 2^31; a scratch of 2^31 elements or more; a non-finite
 * threshold; scratch NULL or scratch_elems below the query; points, n_faces or scratch overlapping an input or each other.
 * Launches: three — the exposure masks with per-chunk face counts, one workgroup per sample for the prefix and N, one lane per point.
 * Every node is a kernel (no memset, no copy), there are no atomics and nothing is read on the host.
 * `hip_stream` is the hipStream_t of the Conventions above (NULL = the default stream; work is enqueued, not waited for; the call can be
 * stream-captured into a HIP graph and replayed on new grids and ids in the same buffers).
 * Profiler: no record (the call is meant to be captured, and the event profiler must be off while capturing). */
int64_t s3r_voxel_surface_points_scratch_elems(int batch, int depth, int height, int width);
int s3r_voxel_surface_points(const float* occupancy, float threshold, const int64_t* sample_ids, uint64_t seed,
                             float* points, int32_t* n_faces, int batch, int depth, int height, int width,
                             int n_points, float* scratch, int64_t scratch_elems, void* hip_stream);

/* Kernel-level profiler: when enabled, every kernel the library launches is bracketed by HIP events
 * on the launch stream.  s3r_profile_read synchronises those events and returns, per launch, the
 * kernel family (0 mfma conv, 1 stem, 2 head (tag 1: its backward), 3 cost volume, 4 linear, 5 chamfer, 6 iou (tags 1, 2: voxel BCE), 7 pack, 8 pad copy, 9 disparity read-out / epe (tag 4: the soft read-out's backward; 5, 6: the disparity loss),
 * 10 aux: ONE transform / difference / finish / split-K-combine pass of a convolution layer — no matrix work, `bytes` = what it must
 * read and write — recorded INSIDE that layer's family-0 record, same tag: the layer's record includes its aux passes' time),
 * the caller's tag, milliseconds, and the algorithmic flops / bytes of that launch. */
typedef struct s3r_prof_record {
    int32_t family;
    int32_t tag;
    float ms;
    int32_t launches;   /* kernel launches bracketed by this record (a conv layer may be 1-3 launches) */
    double flops;       /* algorithmic (direct-form) FLOPs of the layer: SURVEY 8d's count */
    double bytes;
    double exec_flops;  /* FLOPs the kernel that ran EXECUTES on the matrix cores (= flops for the direct kernels; 1/2 .. 9/16 of it
                           for the Winograd forms) */
    int32_t algo;       /* what ran: 0 direct, 1 Winograd serial form, 2 class-parallel form, 3 dual form, 4 two-axis form, 5 three-axis
                           form (transposed layers), 6 its class-parallel launch form */
    int32_t launch_form; /* how launch_conv_mfma sent a direct fp32 layer out (it picks these forms itself; no tile code or descriptor field
                           forces them).  bit 0: a tail cut was planned (the layer's own tile over [0, n_cut), the rest re-tiled 64 x 64);
                           bit 1: bulk and remainder went out as ONE launch (so a cut layer may report launches == 1); bit 2: a launch of
                           this layer ran the 64 x 64 tile's six-stage ring (at most 384 workgroups).  A record that brackets several
                           direct launches (sub-batches, residue classes) carries the OR of theirs.  0 for one plain launch and for
                           every other family and algorithm: the field was `reserved`, always 0, before. */
} s3r_prof_record;
int s3r_profile_enable(int max_records);   /* 0 disables and frees the event pool */
int s3r_profile_reset(void);
/* ABI 8.  level 1: the aux passes of the convolution layers (record family 10) get records of their own, nested inside their layer's;
 * 0 (default): layer records only — an event pair between two kernels of a layer costs queue time, which a profile taken for the
 * layers' durations must not carry (bench.py runs one pass of each kind) */
int s3r_profile_detail(int level);
int s3r_profile_read(s3r_prof_record* out, int max_records);   /* returns the number of records */

#ifdef __cplusplus
}
#endif
#endif /* S3R_H */
