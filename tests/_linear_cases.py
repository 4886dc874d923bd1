"""The launch plan of the linear forward, restated on the host, and the shapes that reach every branch of it.

s3r_linear_forward (and an S3R_OP_LINEAR descriptor) is five kernels behind a plan that depends on (B, Cin, Cout) alone
(s3r_pointwise.hip: linear_wgk_ok, linear_split, linear_streams, launch_linear).  `plan` restates it from the kernels' comments:

  wgk     ONE launch, K split over the four waves of a workgroup that owns 32 outputs x 32 batch rows: Cin a multiple of 128 and at
          most 4096, both tensors below 2 GiB, and at least 128 workgroups ceil(Cout / 32) x ceil(B / 32).  Each wave walks
          nblk = Cin / 128 blocks of 32 k behind a 3-slot ring (the prologue issues min(2, nblk) of them).  Scratch: 1 float.
  stream  Cin a multiple of 32, both tensors below 2 GiB: workgroups of 128 outputs x 32 batch rows x one K slice of `kper`
          = Cin / ks, nblk = kper / 32 blocks behind a 4-slot ring (prologue min(3, nblk)).  ks doubles while there are fewer than
          512 workgroups and the halved slice stays a whole number of 32-k blocks of at least 128 k.
  naive   every other Cin: one thread per output, ks = 1, ceil(B Cout / 256) workgroups.
  The slabs [ks][B][Cout] of stream / naive (the scratch: ks B Cout floats) are summed by linear_finish4_kernel when ks >= 16 (four
  waves x q = ks / 4 slabs each, eight at a time from q >= 9 on) and by linear_finish_kernel otherwise (ks <= 8).

tests/test_linear_plan_cpu.py pins the restatement to s3r_linear_scratch_elems (which fixes the kernel and ks) and requires SWEEP
plus the shapes the suite already had to reach every label of `labels`; the GPU files run every shape of SWEEP.
"""
from __future__ import annotations

from dataclasses import dataclass

TWO31 = 1 << 31

# (B, cin, cout): the branch each shape is here for.  Every one is the smallest found that reaches its label
SWEEP = [
    (1, 128, 4096),       # wgk nblk 1 (a prologue shorter than the ring), whole cout tiles, one batch tile
    (33, 256, 2049),      # wgk nblk 2, two batch tiles (the second holds one row), a ragged last cout tile of one output
    (2, 384, 4099),       # wgk nblk 3, ragged
    (3, 4096, 4065),      # wgk at the Cin limit (nblk 32), ragged
    (65, 512, 2017),      # wgk, three batch tiles
    (3, 32, 5),           # stream nblk 1
    (2, 160, 130),        # stream nblk 5, two cout tiles
    (40, 512, 200),       # ks 4, two batch tiles
    (3, 2048, 33),        # ks 16: finish4 with q = 4
    (2, 4096, 129),       # ks 32: q = 8
    (1, 16384, 3),        # ks 128: q = 32, several unrolled batches of eight slabs
    (2, 65536, 2),        # ks 512: q = 128
    (9, 33, 100),         # naive on four workgroups
    (5, 1056, 70),        # kper 1056 (not a power of two), nblk 33
]


@dataclass(frozen=True)
class Plan:
    kernel: str            # "wgk" | "stream" | "naive"
    ks: int                # K slices over workgroups (wgk: 1; its four waves split K inside the workgroup)
    kper: int              # k per slice (wgk: per wave)
    nblk: int              # 32-k blocks a wave walks (naive: 0)
    otiles: int            # output tiles (wgk 32 wide, stream 128 wide; naive: workgroups of 256 outputs over B x Cout)
    btiles: int            # batch tiles of 32 rows (naive: 1)
    ragged: bool           # the last output tile is partial
    finish: str            # None | "finish" | "finish4"
    q: int                 # slabs per wave of finish4 (0 otherwise)
    scratch: int           # floats of scratch


def wgk_ok(B, cin, cout):
    return cin % 128 == 0 and cin <= 4096 and cin * cout * 4 < TWO31 and B * cin * 4 < TWO31 and -(-cout // 32) * -(-B // 32) >= 128


def streams(B, cin, cout):
    return cin % 32 == 0 and cin * cout * 4 < TWO31 and B * cin * 4 < TWO31


def split(B, cin, cout):
    if not streams(B, cin, cout):
        return 1
    wgs = -(-cout // 128) * -(-B // 32)
    ks = 1
    while wgs * ks < 512 and cin // (2 * ks) >= 128 and (cin // (2 * ks)) % 32 == 0:
        ks *= 2
    return ks


def plan(B, cin, cout):
    if wgk_ok(B, cin, cout):
        return Plan("wgk", 1, cin // 4, cin // 128, -(-cout // 32), -(-B // 32), cout % 32 != 0, None, 0, 1)
    ks = split(B, cin, cout)
    four = ks >= 16 and ks % 4 == 0
    fin, q = ("finish4", ks // 4) if four else ("finish", 0)
    if streams(B, cin, cout):
        return Plan("stream", ks, cin // ks, cin // ks // 32, -(-cout // 128), -(-B // 32), cout % 128 != 0, fin, q, ks * B * cout)
    return Plan("naive", 1, cin, 0, -(-(B * cout) // 256), 1, (B * cout) % 256 != 0, fin, q, B * cout)


def _bucket(v, top):
    return str(v) if v < top else f">={top}"


def labels(B, cin, cout):
    """the names of the plan's branches this shape takes"""
    p = plan(B, cin, cout)
    out = set()
    if p.kernel == "wgk":
        out.add(f"wgk-nblk-{_bucket(p.nblk, 4)}")
        out.add("wgk-ragged-cout" if p.ragged else "wgk-whole-cout")
        out.add("wgk-one-batch-tile" if p.btiles == 1 else "wgk-batch-tiles")
        if cin == 4096:
            out.add("wgk-cin-limit")
        return out
    if p.kernel == "stream":
        out.add(f"stream-nblk-{_bucket(p.nblk, 4)}")
        if p.kper & (p.kper - 1):
            out.add("stream-kper-not-a-power-of-two")
        out.add(f"ks-{_bucket(p.ks, 128)}")
    else:
        out.add("naive-one-workgroup" if p.otiles == 1 else "naive-workgroups")
    if p.finish == "finish4":
        out.add(f"finish4-q-{_bucket(p.q, 32)}")
    else:
        out.add(f"finish-ks-{p.ks}")
    return out


ALL_LABELS = (
    {f"wgk-nblk-{n}" for n in ("1", "2", "3", ">=4")} | {"wgk-ragged-cout", "wgk-whole-cout", "wgk-one-batch-tile", "wgk-batch-tiles", "wgk-cin-limit"}
    | {f"stream-nblk-{n}" for n in ("1", "2", "3", ">=4")} | {"stream-kper-not-a-power-of-two"}
    | {f"ks-{k}" for k in ("1", "2", "4", "8", "16", "32", "64", ">=128")}
    | {f"finish4-q-{q}" for q in ("4", "8", "16", ">=32")} | {f"finish-ks-{k}" for k in (1, 2, 4, 8)}
    | {"naive-one-workgroup", "naive-workgroups"}
)

# one shape per kernel for the runs with bias = NULL and, through an S3R_OP_LINEAR descriptor, with a real scale: the smallest
# sweep shape that ends in linear_wgk_kernel, linear_finish_kernel (behind stream and behind naive) and linear_finish4_kernel
PER_KERNEL = {"wgk": (1, 128, 4096), "stream-finish": (3, 32, 5), "naive-finish": (9, 33, 100), "stream-finish4": (3, 2048, 33)}
