"""Which memory every C-ABI entry point touches, and every element it must write, checked per element against fp64.

Every argument lives in its own guarded allocation (tests/_guard.py): guards around each buffer, poison in what must be written, a
sentinel in output halos, NaN in scratch and workspaces, and a bitwise snapshot of every input.  Convolution and linear values are
checked element by element against the float64 layer with the bounds of tests/_ref64.py, and no case may use more than HALF its
bound.  The cost volume, Chamfer, IoU and winner-take-all read-out stay bit-exact against the oracle.

Largest |got - ref| / bound measured on an MI355X, per family (the seeds are fixed and every kernel is deterministic): direct fp32
0.30 (staged-conv3d-5to7-k1-e6: K = 5, where a few ulp are a third of the bound), Winograd 0.055 (v1-fp32-B3-oh3), bf16 0.43
(v5-bf16-B1-oh1, tests/test_bf16_gpu.py's tolerance), chains 0.035 (unfolded->unfolded-c1).  The file runs in about 10 s.
The 26 Winograd cases at ragged shapes and LDS limits (tests/_buffer_cases.py::_wino_shape_cases) stay below 0.042
(ws2-tile5-conv3d-k3-32to2-e60-B1-oh2) and add 0.1 s.

The call bodies live in tests/_abi_bodies.py: tests/test_alignment_gpu.py runs the same bodies with every payload moved off its
256-byte boundary.
"""
import pytest

from tests import _abi_bodies as AB
from tests import _buffer_cases as BC
from tests import _linear_cases as LC

pytestmark = pytest.mark.gpu
HALF = AB.HALF


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


# ---------------------------------------------------------------- s3r_conv_pack_weights + s3r_conv_forward
@pytest.mark.parametrize("case", BC.CONV_CASES, ids=[c.id for c in BC.CONV_CASES])
def test_conv_forward(s3r, lib, case):
    AB.conv_forward_ref64(s3r, lib, case)


# ---------------------------------------------------------------- s3r_chain_forward: the composition matrix
PLANNED = [(n, p, c) for n, p, c, refused in BC.CHAIN_PAIRS if not refused]


@pytest.mark.parametrize("pair", PLANNED, ids=[n for n, _, _ in PLANNED])
def test_chain_forward(s3r, lib, pair):
    AB.chain_forward(s3r, lib, pair)


# ---------------------------------------------------------------- the network's stage entries
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("u8", [False, True], ids=["f32-renders", "u8-renders"])
def test_encoder_forward(s3r, lib, B, precision, u8):
    AB.encoder_forward(s3r, lib, B, precision, u8)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("in_halo", [0, 1])
def test_decoder_forward(s3r, lib, B, precision, in_halo):
    AB.decoder_forward(s3r, lib, B, precision, in_halo)


# ---------------------------------------------------------------- cost volume
CV_SHAPES = [(2, 32, 28, 28, 28), (1, 5, 7, 6, 10), (3, 4, 12, 5, 8), (2, 3, 9, 4, 7)]


@pytest.mark.parametrize("oh", [0, 1, 2])
@pytest.mark.parametrize("shape", CV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cost_volume(s3r, lib, oracle, shape, oh):
    AB.cost_volume(s3r, lib, oracle, shape, oh)


@pytest.mark.parametrize("oh", [0, 1, 2])
@pytest.mark.parametrize("shape", [(3, 32, 28, 28, 28), (1, 8, 7, 6, 10), (2, 16, 12, 5, 8)], ids=lambda s: "x".join(map(str, s)))
def test_cost_volume_bf16(s3r, lib, oracle, shape, oh):
    AB.cost_volume_bf16(s3r, lib, oracle, shape, oh)


@pytest.mark.parametrize("kind", ["wino", "wino2"])
@pytest.mark.parametrize("shape", [(2, 32, 28, 28, 28), (1, 5, 8, 8, 10), (3, 4, 8, 4, 9)], ids=lambda s: "x".join(map(str, s)))
def test_cost_volume_planes(s3r, lib, shape, kind):
    """plane layouts: guards, and the same bits as the call into a plain zero-initialised buffer"""
    AB.cost_volume_planes(s3r, lib, shape, kind)


# ---------------------------------------------------------------- linear
# (the bound sees a dropped TAP; single terms, and test_linear_layer's (32, 32768, 1024) at its full K, are held bit for bit on
# the integer lattice by tests/test_exact_gpu.py)
LIN_SHAPES = [(32, 8192, 1024), (5, 1024, 6144), (33, 96, 40), (3, 50, 7), (70, 4096, 100), (4, 1, 9), (3, 7, 1), (2, 64, 7),
              (7, 7, 7), (1, 256, 1)]


# ... and every branch of the launch plan: tests/_linear_cases.py::SWEEP holds the reason for each shape
@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
@pytest.mark.parametrize("shape", LIN_SHAPES + LC.SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_linear_forward(s3r, lib, shape, act):
    AB.linear_forward(s3r, lib, shape, act)


@pytest.mark.parametrize("kernel", list(LC.PER_KERNEL))
def test_linear_forward_null_bias(s3r, lib, kernel):
    """bias = NULL, once per kernel of the plan that applies it (linear_wgk_kernel, linear_finish_kernel behind the ring and behind
    the naive kernel, linear_finish4_kernel): guards, poison, the fp64 bound at HALF"""
    AB.linear_forward(s3r, lib, LC.PER_KERNEL[kernel], "relu", bias=False)


@pytest.mark.parametrize("kernel", list(LC.PER_KERNEL))
def test_linear_descriptor_with_a_scale(s3r, lib, kernel):
    """the same kernels behind an S3R_OP_LINEAR descriptor with a folded BatchNorm: their scale[o] branch on a real vector"""
    AB.linear_descriptor(s3r, lib, LC.PER_KERNEL[kernel], "relu")


# ---------------------------------------------------------------- Chamfer, IoU, disparity, channels-last hand-off
@pytest.mark.parametrize("m", [1, 7, 2047, 2049])
@pytest.mark.parametrize("n", [1, 7, 2047, 2049])
def test_chamfer_forward(s3r, lib, oracle, n, m):
    AB.chamfer_forward(s3r, lib, oracle, n, m)


@pytest.mark.parametrize("shape", [(5, 32768), (1, 1), (3, 4097), (2, 77)], ids=lambda s: "x".join(map(str, s)))
def test_voxel_iou(s3r, lib, oracle, shape):
    AB.voxel_iou(s3r, lib, oracle, shape)


@pytest.mark.parametrize("shape", [(3, 32, 28, 28, 28), (2, 5, 7, 13, 40), (1, 64, 9, 57, 16), (4, 3, 1, 1, 4), (1, 7, 3, 5, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_disparity_wta(s3r, lib, oracle, shape):
    AB.disparity_wta(s3r, lib, oracle, shape)


@pytest.mark.parametrize("shape", [(6, 784), (1, 1), (3, 1025), (2, 7)], ids=lambda s: "x".join(map(str, s)))
def test_disparity_epe(s3r, lib, oracle, shape):
    AB.disparity_epe(s3r, lib, oracle, shape)


@pytest.mark.parametrize("shape", [(3, 32, 784), (2, 512, 64), (1, 40, 35), (5, 8, 1), (1, 1, 1), (2, 7, 13)], ids=lambda s: "x".join(map(str, s)))
def test_channels_last_to_f32(s3r, lib, shape):
    AB.channels_last_to_f32(s3r, lib, shape)
