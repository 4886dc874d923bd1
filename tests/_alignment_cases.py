"""The cases of tests/test_alignment_gpu.py: skew patterns, the exception list, and one case per kernel and launch form.

The contract (include/s3r.h, Conventions): an fp32 / int32 tensor needs 4-byte alignment at every entry point and the result bits
do not depend on the address; a bf16 tensor (and the scratch / workspace of S3R_BF16 layers) needs 16 bytes, host-checked; renders
need 16 bytes.  The bodies are tests/_abi_bodies.py's (shared with tests/test_buffers_gpu.py); a pattern moves their guarded
allocations (tests/_guard.py, `skew`).

Skew patterns (fp32 / int32 arguments, in elements):

  all1, all3   every argument by 1 / by 3 (4 B, 12 B)
  mixed        argument i of the call (in order of first construction) by [1, 2, 3, 4, 33][i % 5]: 4, 8, 12, 16, 132 B
  in1          only the inputs (weights, scale / shift / bias included) by 1
  out1, out4   only the outputs by 1 / by 4 (out4: 16-byte aligned and nothing more, the other side of the finish kernels' address
               branches)
  ws1          only scratch / ws / packed weights by 1

A bf16 argument of a launched case takes 8 elements where an fp32 one takes 1, 4 or 2 and 72 where it takes 3 or 33 (16 B, 144 B);
the fp32-typed scratch / ws of a bf16 call 4 and 36 floats; an argument of the exception list (renders) 16 B and 144 B.  No case
launches a kernel on a bf16 or 8-bit tensor that is less than 16-byte aligned: those are refusals (tests/test_abi_cpu.py, and the
stem cases here, which assert the refusal on the device before the call proper).

Which case takes which side of the four address-dependent branches of the Winograd units (s3r_wino_*.hip):

  launch_wino_diff (the two-column kernel iff x and the difference scratch are 8-byte aligned and Wp is even; the scalar
      wino_diff_kernel otherwise): dwino-tile0-d2, dwino-tile1-d1, dwino-tile2-d2, wino3-tile6/7/8-deconv3d-64to32-e8 (Wp = n + 2 is
      even in all of them).  Two-column side: skew 0, out1, out4.  Scalar side: all1, all3, mixed, in1 (x at 4 or 12 B) and ws1 (the
      scratch at 4 B)
  wino2_copy_out / wino2_zero_out (16-byte stores iff the destination is 16-byte aligned and count % 4 == 0): the 2D finish of
      wino2-tile3/4/5-conv2d-64to96-e20 (out_halo 2: whole padded planes of 24 x 24 floats) and the finishes of wino2-tile3/4-v3, -v6
  wino2s_finish_kernel (the same on y and a slice): the semi-fused 3D form, wino2-tile5-v3 (slices of 14 x 14 floats)
      16-byte side of the three: skew 0, out4 (y 16-byte aligned and nothing more), in1, ws1.  Scalar side: all1, all3, out1 (y at
      4 / 12 B); under mixed y takes whichever skew its position in the call gives it
"""
from __future__ import annotations

import torch

from tests import _buffer_cases as BC
from tests import _exact_cases as X

PATTERNS = ("all1", "all3", "mixed", "in1", "out1", "out4", "ws1")
MIXED = (1, 2, 3, 4, 33)
WS_NAMES = ("scratch", "ws", "packed")

# The (entry, argument) pairs whose fp32 / int32 / 8-bit pointer needs more than its element size:
# (entry, argument in include/s3r.h, its name in the test bodies, bytes, the sentence of include/s3r.h that documents it, the reason)
_RENDERS = "Render tensors must be 16-byte aligned, fp32 and 8-bit alike (the stems fetch whole render rows 16 bytes at a time)."
_STAGE = "images_left and images_right must be 16-byte aligned (also for s3r_chain_forward and s3r_conv_forward on the stem)."
_WHY = "stem_kernel / stem_wino_kernel / stem_bf16_kernel fetch a render row by 16-byte LDS-DMA from base + row x width x element size: " \
       "with 8-bit renders the address is byte-granular, below the 4 bytes an LDS-DMA needs"
EXCEPTIONS = [
    ("s3r_encoder_forward", "images_left", "left", 16, _STAGE, _WHY),
    ("s3r_encoder_forward", "images_right", "right", 16, _STAGE, _WHY),
    ("s3r_encoder_forward_u8", "images_left", "left", 16, _STAGE, _WHY),
    ("s3r_encoder_forward_u8", "images_right", "right", 16, _STAGE, _WHY),
    ("s3r_chain_forward", "x (a chain that starts with the stem)", "x", 16, _RENDERS, _WHY),
    ("s3r_conv_forward", "x (the stem descriptor)", "x", 16, _RENDERS, _WHY),
]


def exception_names(entry, stem=True):
    """the test-body names of `entry`'s arguments in the exception list (the conv / chain rows apply to stem descriptors only)"""
    return {name for e, _, name, _, _, _ in EXCEPTIONS if e == entry and (stem or name != "x")}


class Pattern:
    """callable (name, dtype, role) -> skew in elements, for tests/_guard.py::skews"""

    def __init__(self, pid, sixteen=(), bf16_call=False):
        assert pid in PATTERNS or pid == "aligned", pid
        self.pid, self.sixteen, self.bf16_call = pid, set(sixteen), bf16_call
        self.index = {}

    def side(self, name, role):
        if name.startswith(WS_NAMES):
            return "ws"
        return "in" if role == "in" else "out"                  # (the plane sets a cost volume writes are a "scratch" role: an output)

    def fp32_skew(self, name, role):
        i = self.index.setdefault(name, len(self.index))
        side = self.side(name, role)
        return {"aligned": 0, "all1": 1, "all3": 3, "mixed": MIXED[i % 5], "in1": int(side == "in"), "out1": int(side == "out"),
                "out4": 4 * int(side == "out"), "ws1": int(side == "ws")}[self.pid]

    def __call__(self, name, dtype, role):
        s = self.fp32_skew(name, role)
        wide = s in (3, 33)                                     # -> 144 B where 16 bytes are required, else 16 B
        if s == 0:
            return 0
        if dtype == torch.bfloat16:
            return 72 if wide else 8
        if dtype == torch.uint8:
            return 144 if wide else 16
        if name in self.sixteen or (self.bf16_call and self.side(name, role) == "ws" and not name.startswith("packed")):
            return 36 if wide else 4
        return s


# ---------------------------------------------------------------- s3r_conv_pack_weights + s3r_conv_forward
_X = {c.id: c for c in X.ALL_CASES}
_B = {c.id: c for c in BC.CONV_CASES}

# on the integer lattice (tests/_exact_cases.py): the reference is the exact fp64 result, bit for bit
EXACT_CONV = [_X[i] for i in (
    "e1-relu-B1",                                  # stem, fp32 output
    "e1-bf16-B1",                                  # stem, bf16 output
    "tile1-vec1-conv3d_s1_w8",                     # direct MFMA, dword gather
    "tile1-vec0-conv3d_s1_w8",                     # direct MFMA, 16-byte gather
    "tile3-vec0-conv2d_s1_w12",                    # ... 2D
    "e3-relu-B1", "e6-relu-B1",                    # bulk + remainder in one launch (the library's own tiling)
    "tile2-vec0-conv3d_s2", "tile0-vec0-conv2d_s2",              # stride 2
    "tile1-vec0-deconv_w4", "tile4-vec1-deconv",                 # transposed k4 s2 p1: 16-byte and dword gather
    "tile1-vec0-conv3d_k4_valid",
    "splitk2-conv3d_k4_valid", "splitk4-deconv", "splitk4-conv3d_s2", "leaky-half-splitk2-finish",      # forced split-K: the combine pass
    "d4-none-B1", "g-head-conv2d-48to1-sigmoid-e6",              # the head kernel
    "wino1-serial-conv2d-32to48-e40", "wino1-class-parallel-conv3d-64to64-e12", "wino1-dual-conv2d-32to48-e40",
    "wino1-class-parallel-conv2d-32to48-e40", "wino1-serial-conv3d-64to64-e12",
    "wino2-tile3-conv2d-64to96-e20", "wino2-tile4-conv2d-64to96-e20", "wino2-tile5-conv2d-64to96-e20",
    "wino2-tile3-v3", "wino2-tile4-v3", "wino2-tile5-v3",
    "wino2-tile3-v6", "wino2-tile4-v6",                          # the k4 valid layer (F(2, 4) x F(2, 4))
    "dwino-tile0-d2", "dwino-tile1-d1", "dwino-tile2-d2",        # transposed F(2, 2) classes: the difference pass
    "wino3-tile6-deconv3d-64to32-e8", "wino3-tile7-deconv3d-64to32-e8", "wino3-tile8-deconv3d-64to32-e8",
    "g-staged-conv2d-20to33-k5-e9",                # staged cin % 16 != 0
    "g-unfolded-conv2d-3to16-k7s2-e33",            # unfolded RGB
    "g-tclass-deconv2d-32to33-k4s2-e7", "g-tclass-inplace-h1-deconv2d-64to32-k4s2-e16",      # residue-class transposed
    "g-d2s-deconv2d-32to24-k3s3-e7",               # k == stride: depth-to-space
    "g-dilated-deconv2d-16to16-k3s2p2d2-e6", "g-dilated-conv2d-32to32-d2-e16",               # zero-stuffed dilation
    "leaky-2-pass-conv3d",                         # the activation pass
    "bf16-tile1-conv3d_s2", "bf16-tile18-conv2d_s2", "bf16-tile2-conv3d_k4_valid_ks2",       # bf16 per-tap gather (the last: split-K)
    "bf16-tile3-conv3d_s1_c64", "bf16-tile4-deconv",
    "bf16-tile9-conv3d_s1", "bf16-tile10-conv2d_s1_w28",                                     # bf16 row-reuse gather
    "bf16-tile5-conv3d_s1_c64", "bf16-tile22-conv3d_s1_w14", "bf16-tile21-deconv_c64", "bf16-tile23-c128_cout128_ks2",   # plane-reuse
    "e8-bf16-B1", "d3-bf16-B1", "d4-bf16-B1",                    # the library's picks; the bf16 head
)]
assert not [c.id for c in EXACT_CONV if c.refused]

# transcendental activations: tests/_ref64.py's bound at HALF, as tests/test_buffers_gpu.py
BOUND_CONV = [_B[i] for i in ("tanh-pass-conv2d-32to16-e8", "elu-pass-conv3d-32to32-e8", "unfolded-conv3d-2to24-k4s2-elu-e10",
                              "d2s-deconv2d-16to40-k4s4-sigmoid-e5", "head-conv2d-48to1-sigmoid-e6", "d4-fp32-B1-oh0", "d4-bf16-B1-oh0")]

# ---------------------------------------------------------------- chains: one per hand-off kind
CHAIN_PAIRS = [(n, p, c) for n, p, c, refused in BC.CHAIN_PAIRS if not refused and n in (
    "direct->direct-p1",               # plain halo
    "wino2-2d->wino2-2d",              # WINO_HW: the producer's finish writes the consumer's plane sets
    "wino2-3d->wino2-3d",
    "wino1-e40->wino1",
    "linear->tclass-h1",               # reshape behind a linear layer
    "direct->linear",                  # ... and in front of one
    "reshape-conv->d2s",
    "direct->head-2d", "tuned-deconv3d-e16->head-3d-e32",      # fused head: direct and Winograd producer
    "unfolded->staged",
)]
assert len(CHAIN_PAIRS) == 10, [n for n, _, _ in CHAIN_PAIRS]

# ---------------------------------------------------------------- everything else
CV_CASES = [((2, 32, 28, 28, 28), 0), ((2, 32, 28, 28, 28), 1), ((2, 3, 9, 4, 7), 1), ((1, 5, 7, 6, 10), 0)]
CV_BF16_CASES = [((3, 32, 28, 28, 28), 1), ((1, 8, 7, 6, 10), 0)]
CV_PLANE_CASES = [((2, 32, 28, 28, 28), "wino"), ((2, 32, 28, 28, 28), "wino2"), ((1, 5, 8, 8, 10), "wino"), ((3, 4, 8, 4, 9), "wino2")]
LINEAR_CASES = [((32, 8192, 1024), "relu"), ((5, 1024, 6144), "none"), ((70, 4096, 100), "sigmoid"), ((33, 96, 40), "none"),
                ((3, 50, 7), "relu"), ((7, 7, 7), "none")]
CHAMFER_SIZES = [(n, m) for n in (1025, 2048) for m in (1025, 2048)]
IOU_SHAPES = [(3, 4097), (2, 77), (5, 32768)]
WTA_SHAPES = [(2, 5, 7, 13, 40), (1, 7, 3, 5, 3), (3, 32, 28, 28, 28)]
EPE_SHAPES = [(3, 1025), (2, 7), (6, 784)]
METRICS_SHAPES = [(5, 1000), (5, 1001), (5, 77)]      # (tests/_abi_bodies.py::metric_case marks samples 0 .. 4)
CL_SHAPES = [(3, 32, 784), (1, 40, 35), (2, 512, 64)]
# (id, feature dtype, (B, C, H, W, D), output size, confidence maps or NULL)
SOFT_CASES = [("fp32-upsample", 0, (2, 32, 28, 28, 28), (224, 224), True), ("fp32-feature", 0, (3, 5, 7, 13, 4), (7, 13), True),
              ("bf16-upsample", 1, (2, 16, 9, 11, 6), (23, 40), True), ("fp32-no-confidence", 0, (2, 8, 12, 41, 40), (61, 81), False),
              ("bf16-feature-no-confidence", 1, (1, 32, 28, 28, 28), (28, 28), False)]
