"""csrc/s3r_cv_live.h — the rule by which v1's class GEMM leaves out K tiles — held against the cost volume itself: the header is
compiled into a host program (tests/c_abi/cv_live_dump.c), the masked, halo-padded volume and its 36 S3R_LAYOUT_WINO_DH plane sets are
rebuilt in numpy from random features, and every K tile the header calls dead must read nothing but zeros in all 36 sets."""
import numpy as np
import pytest

from tests import _cv_live as CV


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [20, 24, 28])
def test_dead_k_tiles_read_only_zeros(n, B):
    C = 2
    rng = np.random.default_rng(100 * n + B)
    fl, fr = rng.standard_normal((2, B, C, n, n))
    V = CV.plane_sets(CV.cost_volume_padded(fl, fr, n), n)                   # (36, B, 2C, n/4, n+2, n/4)
    assert np.count_nonzero(V) > 0.3 * V.size
    zero = ~np.any(V != 0.0, axis=0)                                         # [B, 2C, sd, wp, sh]: zero in every plane set
    zero_half = np.stack([zero[:, :C].all(axis=1), zero[:, C:].all(axis=1)])  # [half, B, sd, wp, sh]
    dead = CV.dead_table(n, B)
    tiles = CV.position_tiles(n, B)                                          # [B, sd, w, sh]
    checked = 0
    for half in range(2):
        for tw in range(3):
            reads_zero = zero_half[half][:, :, tw:tw + n, :]                 # position column w reads padded column w + tw
            flagged = dead[tiles, half, tw]
            assert np.all(reads_zero[flagged]), (n, B, half, tw)
            checked += int(dead[:, half, tw].sum())
    assert checked == int(dead.sum())
    if n == 28:
        assert checked > 0
    # a tile that straddles two depth groups or samples, and every tile of depth group 0, is live
    sg = n // 4
    first = np.arange(dead.shape[0]) * CV.TILE
    last = np.minimum(first + CV.TILE, B * sg * n * sg) - 1
    per = n * sg
    straddles = first // per != last // per
    assert not dead[straddles].any()
    assert not dead[(first // per) % sg == 0].any()


def test_dead_share_at_the_benchmark_shape():
    """the share of v1's K tiles the rule leaves out at edge 28, B = 32 (docs/LAB_NOTES.md records it)"""
    d = CV.dead_table(28, 32)
    share = d.mean()
    per_half = d.mean(axis=(0, 2))
    print(f"dead K tiles at edge 28, B = 32: {int(d.sum())} of {d.size} = {share:.4f} (half 0 {per_half[0]:.4f}, half 1 {per_half[1]:.4f})")
    # structural zeros: padded columns wp < 4 sd (half 0) or wp >= 30 - 4 sd (half 1) of depth groups sd = 1..6, 84 of the 7 x 30 cells
    # of a half; a tile-granular rule finds less than that, never more
    assert 0.0 < share < 84 / 210
