"""8-bit render ingestion, the bf16 -> fp32 hand-off kernel, the soak (race screen of the counted-vmcnt pipelines) and
the one-rank RCCL rehearsal.

8-bit renders: the reference decodes its PNG renders with OpenCV (/root/reference/requirements.txt:5, README.md:73-74),
so the source data is uint8; `s3r_encoder_forward_u8` takes it as it is and the stem scales by 1/255 as it reads, with
the single rounding of the host conversion float32(u) / 255.  What is tested: the u8 entry equals the fp32 entry on the
host-converted renders BIT FOR BIT (both precisions, both stems of the bf16 path, many images per persistent workgroup),
and the oracle within the usual tolerance.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8_pairs(n, seed):
    g = torch.Generator().manual_seed(seed)
    left = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8)
    left[0, :, :2, :] = 0                      # extremes on the image border (zero padding next to 0 and 255)
    left[0, :, :, :2] = 255
    right[0, :, -2:, :] = 255
    return left, right


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_u8_entry_equals_fp32_entry_bitwise_and_the_oracle(s3r, oracle, precision):
    hip = s3r.Stereo2Voxel(precision)
    s3r.seed_module(hip, 4)
    ref = oracle.OracleStereo2Voxel().eval()
    ref.load_state_dict(hip.state_dict())
    hip.to(DEV)
    left, right = _u8_pairs(3, 21)
    fl, fr = s3r.data.renders_to_float(left), s3r.data.renders_to_float(right)
    got8 = hip(left.to(DEV), right.to(DEV)).clone()
    got32 = hip(fl.to(DEV), fr.to(DEV))
    assert torch.equal(got8, got32)                                   # same bits: one rounding, the same one
    with torch.no_grad():
        want = ref(fl, fr)
    err = ((got8.cpu() - want).norm() / want.norm()).item()
    assert err < (1e-5 if precision == "fp32" else 2e-2), err          # fp32: north_star's 1e-4 with margin
    # every 8-bit value through the stem alone (all 256 codes appear thousands of times in a random image)
    feats8 = hip.encoder(left.to(DEV), upto="e1")
    feats32 = hip.encoder(fl.to(DEV), upto="e1")
    assert torch.equal(feats8, feats32)
    # the conversion made ON THE DEVICE is the same correctly rounded quotient (a scalar divisor would multiply by 1/255 there)
    assert torch.equal(s3r.data.renders_to_float(left.to(DEV)).cpu(), fl)
    # an 8-bit view at an odd storage offset: the stems' 16-byte row fetches need an aligned base, so the module copies it once
    buf = torch.zeros(left.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:].copy_(left.to(DEV).flatten())
    odd = buf[1:].view(left.shape)
    assert odd.data_ptr() % 16 and torch.equal(hip.encoder(odd, upto="e1"), feats8)
    # mixed dtypes are refused, not converted behind the caller's back
    with pytest.raises(RuntimeError, match="dtype"):
        hip(left.to(DEV), fr.to(DEV))


def test_u8_stem_many_images_per_persistent_workgroup(s3r):
    """The bf16 path's MFMA stem runs persistent workgroups over two alternating row slabs: 80 images = 2240 passes on
    <= 512 resident workgroups, rows of 224 bytes in 256-byte slots — against its own fp32-input form, bitwise."""
    spec = s3r.arch_spec
    g = torch.Generator().manual_seed(12)
    x8 = torch.randint(0, 256, (80, 3, spec.IMG_HW, spec.IMG_HW), generator=g, dtype=torch.uint8)
    enc = s3r.Encoder("bf16")
    s3r.seed_module(enc, 5)
    enc.to(DEV)
    got = enc(x8.to(DEV), upto="e1")
    want = enc(s3r.data.renders_to_float(x8).to(DEV), upto="e1")
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    assert torch.equal(enc(x8.to(DEV), upto="e1"), got)                # deterministic across launches
    # an odd image count through the single-tensor entry, and the pair entry on two tensors
    assert torch.equal(enc(x8[:5].to(DEV), upto="e1"), got[:5])
    pair = enc.forward_pair(x8[:3].to(DEV), x8[3:6].to(DEV))
    assert torch.equal(pair, enc(x8[:6].to(DEV)))


def test_u8_fallback_stem_in_a_child_process(tmp_path):
    """S3R_STEM_MFMA=0 selects the bf16 path's VALU stem (read once per process): u8 entry == fp32 entry there too."""
    code = (
        "import torch, s3r\n"
        "g = torch.Generator().manual_seed(3)\n"
        "x8 = torch.randint(0, 256, (5, 3, 224, 224), generator=g, dtype=torch.uint8)\n"
        "enc = s3r.Encoder('bf16'); s3r.seed_module(enc, 5); enc.to('cuda:0')\n"
        "a = enc(x8.to('cuda:0'), upto='e1'); b = enc(s3r.data.renders_to_float(x8).to('cuda:0'), upto='e1')\n"
        "assert torch.equal(a, b)\n"
        "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, S3R_STEM_MFMA="0"))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_u8_through_graph_point_model_and_eval_drivers(s3r, tmp_path):
    from tests.test_data_cpu import _make_tree
    left, right = _u8_pairs(4, 33)
    # HIP-graph replay with 8-bit static inputs
    hip = s3r.Stereo2Voxel("bf16")
    s3r.seed_module(hip, 1)
    hip.to(DEV)
    want = hip(left.to(DEV), right.to(DEV)).clone()
    g = s3r.GraphedForward(hip, 4, DEV, input_dtype=torch.uint8)
    assert torch.equal(g(left.to(DEV), right.to(DEV)), want)
    with pytest.raises(RuntimeError):
        g(left.float().to(DEV), right.float().to(DEV))                # captured for uint8 renders
    # Stereo2Point (bf16 convolutions, fp32 head: the latent crosses through s3r_channels_last_to_f32)
    pt = s3r.Stereo2Point("bf16")
    s3r.seed_module(pt, 2)
    pt.to(DEV)
    assert torch.equal(pt(left.to(DEV), right.to(DEV)),
                       pt(s3r.data.renders_to_float(left).to(DEV), s3r.data.renders_to_float(right).to(DEV)))
    # dataset driver: uint8 items (default) and float32 items give the same per-sample metric, bit for bit
    fp = s3r.Stereo2Voxel()
    s3r.seed_module(fp, 0)
    fp.to(DEV)
    _make_tree(str(tmp_path), n_models=3, views=(0,), size=224)
    a = s3r.evaluate.test_dataset(fp, s3r.data.StereoShapeNet(str(tmp_path)), batch=2, device=DEV)
    b = s3r.evaluate.test_dataset(fp, s3r.data.StereoShapeNet(str(tmp_path), render_dtype="float32"), batch=2, device=DEV)
    assert a["samples"] == 3 and torch.equal(a["per_sample"], b["per_sample"])
    # tensor driver on a host list of uint8 renders (page-locked in place, prefetched as uint8)
    gt = torch.zeros(4, 32, 32, 32)
    gt[:, 4:20, 4:20, 4:20] = 1
    c = s3r.evaluate.test_net(fp, left, right, gt, batch=3, device=DEV)
    d = s3r.evaluate.test_net(fp, s3r.data.renders_to_float(left), s3r.data.renders_to_float(right), gt, batch=3, device=DEV)
    assert torch.equal(c["per_sample"], d["per_sample"])


def test_channels_last_to_f32_is_exact(s3r):
    g = torch.Generator().manual_seed(9)
    for shape in ((3, 32, 28, 28), (2, 512, 4, 4, 4), (1, 40, 5, 7), (5, 8, 1, 1)):
        x = torch.randn(shape, generator=g).to(torch.bfloat16)
        phys = x.permute(0, *range(2, x.dim()), 1).contiguous().to(DEV)          # channels-last memory
        logical = phys.permute(0, x.dim() - 1, *range(1, x.dim() - 1))
        got = s3r.modules.channels_last_to_f32(logical)
        assert got.is_contiguous() and got.dtype == torch.float32 and torch.equal(got.cpu(), x.float())
    assert s3r.modules.channels_last_to_f32(torch.zeros(0, 32, 28, 28, dtype=torch.bfloat16, device=DEV)).shape == (0, 32, 28, 28)


# ------------------------------------------------------------------ soak: a race screen for the counted-vmcnt pipelines
SOAK = [("fp32", "voxel", (32, 3, 1)), ("bf16", "voxel", (64, 7)), ("fp32", "point", (8,))]


@pytest.mark.parametrize("precision,variant,batches", SOAK, ids=[f"{p}-{v}" for p, v, _ in SOAK])
def test_soak_repeated_forwards_are_bitwise_stable(s3r, precision, variant, batches):
    """The kernels carry hand-counted `s_waitcnt vmcnt(N)` rings (the six-stage conv ring, the four-deep linear ring, the
    stem's row slabs, the bf16 three-slot weight ring, the fused front's row rings): a misplaced wait shows up as a RARE
    wrong tile.  40 forwards per configuration, batch sizes alternating on ONE module (so the arena is re-laid-out and
    re-zeroed between them), every output compared bitwise with the first one for that batch."""
    model = (s3r.Stereo2Voxel if variant == "voxel" else s3r.Stereo2Point)(precision)
    s3r.seed_module(model, 5)
    model.to(DEV)
    data = {b: tuple(t.to(DEV) for t in s3r.synthetic_pairs(b, seed=100 + b)) for b in batches}
    ref = {b: model(*data[b]).clone() for b in batches}
    bad = 0
    for i in range(40):
        b = batches[i % len(batches)]
        bad += int(not torch.equal(model(*data[b]), ref[b]))
    assert bad == 0


def test_graph_replay_beside_an_eager_forward_on_a_second_stream(s3r):
    """A captured graph of one module instance replayed while ANOTHER instance runs eager forwards on a second stream:
    both share the chip (and the library's process-wide state) and must produce their stand-alone bits."""
    a = s3r.Stereo2Voxel("bf16")
    b = s3r.Stereo2Voxel("fp32")
    s3r.seed_module(a, 7), s3r.seed_module(b, 8)
    a.to(DEV), b.to(DEV)
    la, ra = (t.to(DEV) for t in s3r.synthetic_pairs(16, seed=61))
    lb, rb = (t.to(DEV) for t in s3r.synthetic_pairs(5, seed=62))
    want_a, want_b = a(la, ra).clone(), b(lb, rb).clone()
    g = s3r.GraphedForward(a, 16, DEV)
    g.left.copy_(la), g.right.copy_(ra)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    bad = 0
    for _ in range(10):
        with torch.cuda.stream(s1):
            ya = g()
        with torch.cuda.stream(s2):
            yb = b(lb, rb)
        s1.synchronize(), s2.synchronize()
        bad += int(not torch.equal(ya, want_a)) + int(not torch.equal(yb, want_b))
    assert bad == 0


# ------------------------------------------------------------------ RCCL rehearsal with one rank
@pytest.mark.timeout(500)
def test_bench_force_dist_builds_an_rccl_communicator_of_one_rank():
    """`python bench.py --gpus 1 --force-dist --backend nccl`: the N>1 code path (self-launched child torchrun,
    init_process_group('nccl'), warm-up all-gather, all-reduce, per-step collation, version query) with WORLD_SIZE = 1 —
    what a 1-GPU box can rehearse of BASELINE configs[4].  (A one-rank communicator exchanges no peer buffers: the
    HSA_ENABLE_IPC_MODE_LEGACY default stays unverified until N > 1 ranks run.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--backend", "nccl",
                          "--steps", "3", "--warmup", "1", "--batch", "4"], capture_output=True, text=True, timeout=450,
                         cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["collective_backend"] == "nccl" and d["n_ranks_seen"] == 1 and d["rccl_version"]
    assert d["n_gpus"] == 1 and d["value"] > 0 and "RCCL all-gather" in d["config"]["parallelism"]


@pytest.mark.timeout(500)
def test_bench_global_batch_flag_and_runner_force_dist():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--global-batch", "6", "--steps", "2", "--warmup",
                          "1", "--full", "--no-secondary", "--no-cpu-baseline", "--renders", "u8"], capture_output=True, text=True,
                         timeout=450, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["global_batch"] == 6 and d["config"]["per_gpu_batch"] == 6 and "8-bit" in d["config"]["workload"]
    assert d["roofline"]["traffic"] is None                     # not the configuration the committed counters were taken on
    out = subprocess.run([sys.executable, os.path.join(ROOT, "runner.py"), "--test", "--force-dist", "--samples", "6",
                          "--batch", "4"], capture_output=True, text=True, timeout=450, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["collective_backend"] == "nccl" and r["n_ranks_seen"] == 1 and r["rccl_version"] and r["samples"] == 6
    assert r["renders"] == "uint8"
