/* Which K tiles of v1's class GEMM read nothing but the cost volume's structural zeros: the ONE statement of the rule, shared by the
 * class kernel (s3r_wino_gemm.hip, wino_body<.., CVL>) and by the host test that checks it against a volume rebuilt in numpy
 * (tests/test_cv_live_cpu.py compiles this header as plain C).
 *
 * The cost volume of edge n (D = H = W = n, n % 4 == 0) is masked by construction (s3r_pointwise.hip, cost_volume_wino2_kernel):
 *     half 0 (channels [0, C))   L - R(w - d)  where w >= d,     +0 elsewhere
 *     half 1 (channels [C, 2C))  R - L(w + d)  where w + d < n,  +0 elsewhere
 * Its S3R_LAYOUT_WINO_DH plane sets are (36, B, 2C, n/4, n+2, n/4): depth group sd, PADDED column wp = w + 1, row group sh, the row
 * group fastest.  Depth group sd transforms the padded depths 4 sd .. 4 sd + 5, that is d = 4 sd - 1 .. 4 sd + 4, so all 36 of its
 * class values are +0 wherever every d of the window is masked: for sd >= 1, half 0 at wp < 4 sd and half 1 at wp >= n + 2 - 4 sd
 * (sd = 0 holds d = 0, which masks nothing).
 *
 * The GEMM's positions run (sample, depth group, column w, row group): `per_group` = n * (n / 4) positions per (sample, depth
 * group), `rows` = n / 4 of them per column.  A K tile is (a tile of consecutive positions [first, last], a channel half, a column tap
 * tw = 0..2); position column w reads padded column w + tw.  It is DEAD when the whole tile lies in one (sample, depth group),
 * sd >= 1, and every padded column it reads is in that half's zero region.  Everything else is live. */
#ifndef S3R_CV_LIVE_H
#define S3R_CV_LIVE_H

#if defined(__HIPCC__)
#define S3R_CV_HD __host__ __device__ __forceinline__
#else
#define S3R_CV_HD static inline
#endif

/* The rule on a decoded tile.  n: the edge; half: 0 / 1; tw: the column tap; one_group: the tile's first and last position lie in one
 * (sample, depth group); sd: that depth group; w_lo, w_hi: the columns of the first and the last position.  Returns 1: dead, 0: live */
S3R_CV_HD int s3r_cv_ktile_dead_at(int n, int half, int tw, int one_group, int sd, int w_lo, int w_hi) {
    if (!one_group || sd < 1) return 0;                  /* a straddling tile and depth group 0 are live */
    if (half == 0) return w_hi + tw < 4 * sd;
    return w_lo + tw - 1 >= n + 1 - 4 * sd;
}

/* ... and from the tile's first and last position (0 <= first <= last).  groups: depth groups per sample (n / 4); rows: row groups per
 * column (n / 4); per_group = n * rows.  (The class kernel decodes the two positions with its launch-invariant fast divisions and
 * calls the function above; tests/test_cv_live_gpu.py shows that it leaves out no tile this one calls live.) */
S3R_CV_HD int s3r_cv_ktile_dead(int n, int half, int tw, int first, int last, int per_group, int groups, int rows) {
    const int g = first / per_group;                     /* (sample, depth group) of the first position */
    const int r0 = first - g * per_group, r1 = last - g * per_group;
    return s3r_cv_ktile_dead_at(n, half, tw, last / per_group == g, g % groups, r0 / rows, r1 / rows);
}

#endif
