"""numpy restatement of s3r_augment_pair (include/s3r.h) for tests/test_augment_{cpu,gpu}.py: one rounded fp32 operation per line, no
notion of launches.  The pair's mean luma is tests/_head64.reduce32 on the (2, S) array of the two views' lumas.

  philox(c, k)                 Philox4x32-10 on uint32 arrays: counter (c0..c3), key (k0, k1) -> four words
  unit(w)                      (float)(w >> 8) * 2^-24
  draws(cfg, id)               what a pair shares: dy, dx, perm, brightness, contrast, saturation, bg[3]
  augment32(cfg, left, right, ids, disp_left, disp_right, mutant)
                               (out_left, out_right[, out_disp_left, out_disp_right]); `mutant` builds the wrong versions the cases
                               must tell from the right one (MUTANTS)
  CASES / inputs(case)         the device test's shapes, configurations and data; COVERAGE_IDS its sample ids

`cfg` is anything with AugmentConfig's attributes (seed, max_shift, permute_rgb, background, brightness, contrast, saturation,
noise_sigma).
"""
import collections

import numpy as np

from tests._head64 import chunk_sums32, reduce32

F = np.float32
U = np.uint32
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]        # lexicographic
MUTANTS = ("fma_blend", "mean_per_view", "descending_chunks", "shared_noise", "truncating_composite")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85

Cfg = collections.namedtuple("Cfg", "seed max_shift permute_rgb background brightness contrast saturation noise_sigma")
IDENTITY = Cfg(0, 0, False, (255, 255), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), 0.0)


def philox(c, k):
    c = [np.asarray(x, np.uint64) for x in c]
    k = [int(x) & 0xFFFFFFFF for x in k]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & mask]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return [x.astype(U) for x in c]


def unit(w):
    return ((np.asarray(w, U) >> U(8)).astype(F) * F(2.0 ** -24)).astype(F)


def _range(u, lo, hi):
    t = F(hi) - F(lo)
    t = F(u) * t
    return F(F(lo) + t)


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def _id(i):
    i = int(i) & (2 ** 64 - 1)
    return i & 0xFFFFFFFF, i >> 32


Draws = collections.namedtuple("Draws", "dy dx perm brightness contrast saturation bg")


def draws(cfg, sample_id):
    key, (i0, i1) = _key(cfg.seed), _id(sample_id)
    g = [int(w) for w in philox((i0, i1, 0, 0), key)]
    span = 2 * int(cfg.max_shift) + 1
    j = philox((i0, i1, 0, 1), key)
    b = [int(w) for w in philox((i0, i1, 0, 2), key)]
    lo, hi = (int(v) for v in cfg.background)
    return Draws(g[0] % span - int(cfg.max_shift), g[1] % span - int(cfg.max_shift), g[2] % 6,
                 _range(unit(j[0]), *cfg.brightness), _range(unit(j[1]), *cfg.contrast), _range(unit(j[2]), *cfg.saturation),
                 [lo + b[c] % (hi - lo + 1) for c in range(3)])


def _clamp(v):
    return np.minimum(np.maximum(v, F(0)), F(1)).astype(F)


def _luma(v):
    a = (F(0.299) * v[0]).astype(F)
    b = (F(0.587) * v[1]).astype(F)
    c = (F(0.114) * v[2]).astype(F)
    s = (a + b).astype(F)
    return (s + c).astype(F)


def _on(r):
    return not (F(r[0]) == F(1) and F(r[1]) == F(1))


def _blend(k, v, target, fma):
    """a = k * v;  t = 1 - k;  b = t * target;  v = a + b;  clamp"""
    t = F(F(1) - k)
    b = (t * target).astype(F)
    if fma:                                                              # the mutant: k * v + b rounded once
        return _clamp((np.float64(k) * v.astype(np.float64) + np.asarray(b, np.float64)).astype(F))
    a = (k * v).astype(F)
    return _clamp((a + b).astype(F))


def _view(cfg, d, img, mutant):
    """steps 1 - 3 of one view: ((3, H, W) fp32, inside (H, W), clipped source rows and columns)"""
    ch, H, W = img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    sy, sx = ys - d.dy, xs - d.dx
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    syc, sxc = np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)
    src = img[:, syc, sxc].astype(U)
    v = np.empty((3, H, W), F)
    for c in range(3):
        code = src[c]
        if ch == 4:
            code = (src[c] * src[3] + U(d.bg[c]) * (U(255) - src[3]) + U(0 if mutant == "truncating_composite" else 127)) // U(255)
        code = np.where(inside, code, U(d.bg[c]))
        t = (code.astype(F) / F(255)).astype(F)
        if _on(cfg.brightness):
            t = (d.brightness * t).astype(F)
            t = _clamp(t)
        v[c] = t
    return v, inside, syc, sxc


def _mean(lumas, mutant):
    """lumas (2, S): the pair's mean luma"""
    S = lumas.shape[1]
    if mutant == "descending_chunks":
        cs = chunk_sums32(lumas)
        p = cs[:, -1].copy()
        for k in range(cs.shape[1] - 2, -1, -1):
            p = (p + cs[:, k]).astype(F)
        total = F(p[0] + p[1])
    else:
        total = F(reduce32(lumas))
    return F(total / F(2 * S))


def augment32(cfg, left, right, ids, disp_left=None, disp_right=None, mutant=None):
    assert mutant is None or mutant in MUTANTS
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    B, ch, H, W = left.shape
    S = H * W
    key = _key(cfg.seed)
    out = [np.empty((B, 3, H, W), F), np.empty((B, 3, H, W), F)]
    with_disp = disp_left is not None
    if with_disp:
        dsrc = [np.asarray(disp_left, F).view(np.int32), np.asarray(disp_right, F).view(np.int32)]
        odisp = [np.empty((B, H, W), np.int32), np.empty((B, H, W), np.int32)]
    index = np.arange(S, dtype=U).reshape(H, W)                          # y W + x of the OUTPUT pixel
    with np.errstate(all="ignore"):
        for b in range(B):
            d = draws(cfg, ids[b])
            i0, i1 = _id(ids[b])
            views = [_view(cfg, d, img[b], mutant) for img in (left, right)]
            if _on(cfg.contrast):
                lumas = np.stack([_luma(v).reshape(S) for v, _, _, _ in views])
                m = _mean(lumas, mutant)
            for side, (v, inside, syc, sxc) in enumerate(views):
                if _on(cfg.contrast):
                    mm = F(reduce32(lumas[side:side + 1]) / F(S)) if mutant == "mean_per_view" else m
                    v = np.stack([_blend(d.contrast, v[c], mm, mutant == "fma_blend") for c in range(3)])
                if _on(cfg.saturation):
                    l = _luma(v)
                    v = np.stack([_blend(d.saturation, v[c], l, mutant == "fma_blend") for c in range(3)])
                if F(cfg.noise_sigma) != F(0):
                    v = v.copy()
                    for c in range(3):
                        w = philox((i0, i1, 1 + 3 * (0 if mutant == "shared_noise" else side) + c, index), key)
                        s = (unit(w[0]) + unit(w[1])).astype(F)
                        s = (s + unit(w[2])).astype(F)
                        s = (s + unit(w[3])).astype(F)
                        s = (s - F(2)).astype(F)
                        s = (s * F(1.7320508)).astype(F)
                        s = (F(cfg.noise_sigma) * s).astype(F)
                        v[c] = _clamp((v[c] + s).astype(F))
                perm = PERMS[d.perm] if cfg.permute_rgb else (0, 1, 2)
                for co in range(3):
                    out[side][b, co] = v[perm[co]]
                if with_disp:
                    odisp[side][b] = np.where(inside, dsrc[side][b][syc, sxc], np.float32(np.inf).view(np.int32))
    if with_disp:
        return out[0], out[1], odisp[0].view(F), odisp[1].view(F)
    return out[0], out[1]


# ---------------------------------------------------------------- the device test's table
# the ids of the device test's 64-sample batch: under seed 0 with max_shift 3 they must draw every permutation, every sign of dy and dx
# and a window that leaves the image on each side (tests/test_augment_cpu.py checks it, so that the device test cannot pass vacuously)
COVERAGE_IDS = list(range(64))
SEED, MAX_SHIFT = 0, 3

# one op alone, then all together
CONFIGS = {
    "identity": IDENTITY,
    "shift": IDENTITY._replace(max_shift=MAX_SHIFT, background=(0, 255)),
    "permute": IDENTITY._replace(permute_rgb=True),
    "brightness": IDENTITY._replace(brightness=(0.5, 1.5)),
    "contrast": IDENTITY._replace(contrast=(0.5, 1.5)),
    "saturation": IDENTITY._replace(saturation=(0.0, 2.0)),
    "noise": IDENTITY._replace(noise_sigma=0.05),
    "all": Cfg(SEED, MAX_SHIFT, True, (0, 255), (0.5, 1.5), (0.5, 1.5), (0.0, 2.0), 0.05),
}

# (H, W): a short quad, rows that are no multiple of 4, one lane row, a chunk, chunks with a ragged end, two and more chunks
SHAPES = [(1, 3), (2, 2), (5, 7), (16, 16), (16, 32), (17, 31), (33, 31), (32, 32), (25, 41)]
BIG = (224, 224)                                                         # once, at B = 2


def renders(B, ch, H, W, seed):
    """(left, right) uint8 renders with every alpha regime (0, 255 and between) and a right view that differs from the left"""
    r = np.random.default_rng(seed)
    left = r.integers(0, 256, (B, ch, H, W), dtype=np.uint8)
    right = r.integers(0, 256, (B, ch, H, W), dtype=np.uint8)
    if ch == 4:
        for x in (left, right):
            a = x[:, 3]
            pick = r.integers(0, 3, a.shape)
            a[pick == 0] = 0
            a[pick == 1] = 255
    return left, right


def disparities(B, H, W, seed):
    """(disp_left, disp_right) with NaN payloads, both infinities, negatives and zeros of both signs, as int32 bit patterns viewed fp32"""
    r = np.random.default_rng(seed + 1000)
    out = []
    for _ in range(2):
        d = (r.standard_normal((B, H, W)) * 20).astype(F)
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32)
        pick = r.integers(0, 3 * len(special), d.shape)
        bits = d.view(np.uint32).copy()
        hit = pick < len(special)
        bits[hit] = special[pick[hit]]
        out.append(bits.view(F))
    return out


def to_cfg(s3r, c):
    """a table row as the package's AugmentConfig"""
    return s3r.AugmentConfig(**c._asdict())
