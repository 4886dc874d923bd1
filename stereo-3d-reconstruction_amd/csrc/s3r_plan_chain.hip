// Planner, unit 4 of 4 (s3r_host.h): the chain planner.  A chain gives every intermediate activation its own region of the
// caller's workspace, with the zero halo the NEXT layer's gather wants; regions are written interior-only, so the halos stay zero
// from the one zero fill that initialises the workspace (ws_fresh: s3r::launch_zero_fill, a kernel).  Nothing here enqueues anything.
#include "s3r_host.h"

#include <cstdlib>

namespace s3rh {

// S3R_WINO_HANDOFF (A/B switch, read once): 0 no hand-off at all; unset / 1 all of them; any other value a mask — bit 1 (2) the 2D
// pair e6 -> e7, bit 2 (4) split-K direct -> two-axis 3D (v4 -> v5), bit 3 (8) two-axis 3D -> two-axis 3D (v5 -> v6), bit 4 (16)
// two-axis 3D -> transposed (v6 -> d1), bit 5 (32) transposed -> transposed (d1 -> d2)
static int handoff_mask() {
    static const int m = getenv("S3R_WINO_HANDOFF") ? atoi(getenv("S3R_WINO_HANDOFF")) : 1;
    return m == 1 ? ~0 : m;
}

// 3D hand-off of the pair (a, b) — a's finish pass writing b's operand (s3r_wino_handoff.hip, wino_handoff_kernel).  Returns the layout
// the pair's ALGORITHMS allow (PLAIN: none) — a function of the descriptors alone, which sizes the region — and through *take
// whether the launch forms planned for this batch on this device take it (both routes give the same bits, so that may follow the
// batch): the producer must leave whole-range raw sums in slabs (split-K; class-parallel), the consumer's operand must fit one call
static int handoff3d(const s3r_conv_desc& a, const s3r_conv_desc& b, bool* take) {
    *take = false;
    if (a.dtype != S3R_F32 || b.dtype != S3R_F32 || a.ndim != 3 || b.ndim != 3 || a.cout != b.cin || out_size(&a) != b.in_size ||
        a.batch != b.batch || a.out_halo != b.in_halo || a.act > S3R_ACT_RELU || a.cout % s3r::wino_bk() != 0 || staged_layer(&a) ||
        staged_layer(&b))
        return S3R_LAYOUT_PLAIN;
    const int op = b.in_size + 2 * b.in_halo;
    if (op * op * op > 8192) return S3R_LAYOUT_PLAIN;                 // (a block of padded volumes in 32 KiB of LDS)
    int alg_a, form_a, alg_b, form_b;
    if (resolve_algo(&a, &alg_a, &form_a) != S3R_OK || resolve_algo(&b, &alg_b, &form_b) != S3R_OK) return S3R_LAYOUT_PLAIN;
    int lay = S3R_LAYOUT_PLAIN, bit = 0;
    bool forms = true;
    // (what follows the batch but not the device — one call's worth of planes, materialised differences — decides the layout itself)
    if (alg_b == ALG_WINO2 && wino2_ax(&b) <= 1 && b.in_halo == b.pad && b.in_size >= (b.pad ? 4 : 5) && fits_one_call(&b, ALG_WINO2))
        lay = S3R_LAYOUT_WINO_3D;
    else if (alg_b == ALG_WINO && b.op == S3R_OP_DECONV && b.in_halo == 1 && dwino_materialise(&b))
        lay = S3R_LAYOUT_DIFF;
    else return S3R_LAYOUT_PLAIN;
    if (alg_a == ALG_WINO2 && wino2_ax(&a) <= 1) {
        bit = lay == S3R_LAYOUT_DIFF ? 16 : 8;
        if (!fits_one_call(&a, ALG_WINO2)) return S3R_LAYOUT_PLAIN;
        forms = wino2_form_of(&a, (int)(wino2_geo(&a).pos_sample * a.batch), form_a) == 0;
    } else if (alg_a == ALG_WINO && a.op == S3R_OP_DECONV && lay == S3R_LAYOUT_DIFF) {
        bit = 32;
        forms = s3r::wino_plan(2, a.cout, wino_kcls(&a), (int)wino_positions(&a, a.batch), false, form_a).mode == s3r::WINO_CP;
    } else if (alg_a == ALG_DIRECT && a.op == S3R_OP_CONV && lay == S3R_LAYOUT_WINO_3D && a.out_layout == S3R_LAYOUT_PLAIN) {
        bit = 4;
        Geo ga;
        int ksplit;
        if (geometry(&a, &ga) != S3R_OK || direct_ksplit(&a, ga, &ksplit) != S3R_OK || ksplit <= 1) return S3R_LAYOUT_PLAIN;
    } else return S3R_LAYOUT_PLAIN;
    if (!(handoff_mask() & bit)) return S3R_LAYOUT_PLAIN;
    // with the layouts set both layers must still resolve to the algorithms (and forced forms) they have without
    s3r_conv_desc a2 = a, b2 = b;
    a2.out_layout = lay; b2.in_layout = lay;
    int alg2, form2;
    Geo g2;
    if (geometry(&a2, &g2) != S3R_OK || geometry(&b2, &g2) != S3R_OK) return S3R_LAYOUT_PLAIN;
    if (resolve_algo(&a2, &alg2, &form2) != S3R_OK || alg2 != alg_a || form2 != form_a) return S3R_LAYOUT_PLAIN;
    if (resolve_algo(&b2, &alg2, &form2) != S3R_OK || alg2 != alg_b || form2 != form_b) return S3R_LAYOUT_PLAIN;
    *take = forms;
    return lay;
}

// conv -> pointwise head fusion: a <=64-cout MFMA conv that does not split K, followed by the
// 1x1 single-channel head, runs the head inside its epilogue; its own output is never materialised
static void plan_head_fusion(Plan* pl, int n) {
    for (int i = 0; i + 1 < n; ++i) {
        const s3r_conv_desc& d = pl->d[i];
        if (pl->r[i] != R_MFMA || pl->r[i + 1] != R_HEAD || d.cout > 64) continue;
        if (pl->d[i + 1].cin != d.cout || d.out_halo != 0 || d.act >= S3R_ACT_SIGMOID || staged_layer(&d)) continue;
        if (d.op == S3R_OP_CONV && resolves_to_wino(&d)) continue;     // (the Winograd conv kernel has no fused-head epilogue)
        int alg = ALG_DIRECT, form, ksplit;
        if (d.dtype != S3R_BF16 && resolve_algo(&d, &alg, &form) != S3R_OK) continue;
        // (a Winograd form's `tile` is a launch-form code, not a tile of the direct kernel)
        if (alg == ALG_DIRECT && (direct_ksplit(&d, pl->g[i], &ksplit) != S3R_OK || ksplit != 1)) continue;
        pl->fuse_head[i] = 1;
    }
}

// the arena: [padded chain input] [each intermediate, or the larger form of a hand-off region] [the scratch all layers share]
static int plan_arena(Plan* pl, int n, int user_in_halo, int need0) {
    int64_t off = 0;
    if (pl->pad_input && pl->d[0].in_layout != S3R_LAYOUT_PLAIN)
        return fail(S3R_ERR_INVALID, "a transformed chain input must come with its halo (in_halo = 1)");
    if (pl->pad_input) {
        if (user_in_halo != 0) return fail(S3R_ERR_INVALID, "chain input halo %d is smaller than the %d its first layer needs",
                                           user_in_halo, need0);
        pl->pad_off = 0;
        off = align_up(pl->g[0].x_store, 256);
    }
    for (int i = 0; i + 1 < n; ++i) {
        pl->off[i] = off;
        if (i == 0 && pl->stem_wino) off = align_up(off + pl->g[1].x_store, 256);      // layer 1's transformed planes
        else if (!pl->fuse_head[i]) off = align_up(off + (pl->region[i] > pl->g[i].y_store ? pl->region[i] : pl->g[i].y_store), 256);   // a fused conv's output does not exist
    }
    for (int i = 0; i < n; ++i) {
        // (a 3D hand-off pair is sized for its two-pass route, the larger: the route taken follows the launch forms, the size must not)
        s3r_conv_desc t = pl->d[i];
        if (i > 0 && pl->region[i - 1]) t.in_layout = S3R_LAYOUT_PLAIN;
        if (pl->region[i]) t.out_layout = S3R_LAYOUT_PLAIN;
        const int64_t sc = s3r_conv_scratch_elems(&t);
        if (sc < 0) return (int)sc;
        if (sc > pl->scratch_elems) pl->scratch_elems = sc;
    }
    pl->scratch_off = off;
    off = align_up(off + pl->scratch_elems, 256);
    pl->total = off;
    return S3R_OK;
}

int plan_chain(const s3r_layer* layers, int n, Plan* pl) {
    if (!layers || n <= 0) return fail(S3R_ERR_INVALID, "empty chain");
    pl->d.resize(n); pl->r.resize(n); pl->g.resize(n); pl->off.assign(n, -1); pl->fuse_head.assign(n, 0); pl->region.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        pl->d[i] = layers[i].desc;
        if (i > 0) pl->d[i].in_layout = S3R_LAYOUT_PLAIN;            // intermediates: the library's plan, not the caller's
        if (i + 1 < n) pl->d[i].out_layout = S3R_LAYOUT_PLAIN;
        int rc = route(&pl->d[i], &pl->r[i]);
        if (rc) return rc;
    }
    const int need0 = need_halo(&pl->d[0], pl->r[0]);
    pl->pad_input = pl->d[0].in_halo < need0;
    const int user_in_halo = pl->d[0].in_halo;
    if (pl->pad_input) pl->d[0].in_halo = need0;
    for (int i = 0; i < n; ++i) {
        if (i > 0) pl->d[i].in_halo = pl->d[i - 1].out_halo;
        if (i + 1 < n) {
            // the wider halo a residue-class consumer reads in place only where the producer can carry it: a linear or head layer
            // writes no halo, and a reshaped output has none in the consumer's geometry — such a consumer stages its own copy
            const s3r_conv_desc& a = pl->d[i];
            const s3r_conv_desc& b = pl->d[i + 1];
            const bool carries = pl->r[i] != R_LINEAR && pl->r[i] != R_HEAD && out_size(&a) == b.in_size && a.cout == b.cin;
            pl->d[i].out_halo = carries ? want_halo(&b, pl->r[i + 1]) : need_halo(&b, pl->r[i + 1]);
        }
        if (i == 1 && pl->r[0] == R_STEM && pl->r[1] == R_MFMA && pl->d[1].dtype == S3R_F32 && pl->d[1].op == S3R_OP_CONV) {
            // a stem feeding the one-axis Winograd kernel writes that kernel's planes itself (the same bits: the stem's values
            // through wino_input_kernel's transform): no plain activation, no transform launch
            static const int fuse = getenv("S3R_STEM_WINO") ? atoi(getenv("S3R_STEM_WINO")) : 1;      // A/B switch, read once
            int alg, form;
            // (launch_stem_wino's own limits: 13 input rows of three channels staged in LDS by at most 9 pieces per thread)
            const bool fits = pl->d[0].in_size % 16 == 0 && pl->d[0].in_size <= 236;
            if (fuse && fits && resolve_algo(&pl->d[1], &alg, &form) == S3R_OK && alg == ALG_WINO &&
                pl->d[1].in_size % wino_r(&pl->d[1]) == 0 && fits_one_call(&pl->d[1], ALG_WINO)) {
                pl->stem_wino = true;
                pl->d[1].in_layout = S3R_LAYOUT_WINO_H;
            }
        }
        if (i > 0 && pl->r[i - 1] == R_MFMA && pl->r[i] == R_MFMA && pl->d[i].dtype == S3R_F32) {
            // two-axis Conv2d -> two-axis Conv2d over the same edge: the first one's finish kernel writes the second one's plane sets
            // (S3R_LAYOUT_WINO_HW: the bits wino2p_input_kernel makes of the plain activation)
            const int fuse = handoff_mask() & 2;
            s3r_conv_desc& a = pl->d[i - 1];
            s3r_conv_desc& b = pl->d[i];
            int alg_a, alg_b, form;
            if (fuse && wino2_ax(&a) == 2 && wino2_ax(&b) == 2 && a.cout == b.cin && out_size(&a) == b.in_size && b.in_size % 4 == 0 &&
                resolve_algo(&a, &alg_a, &form) == S3R_OK && alg_a == ALG_WINO2 && resolve_algo(&b, &alg_b, &form) == S3R_OK &&
                alg_b == ALG_WINO2 && fits_one_call(&a, ALG_WINO2) && fits_one_call(&b, ALG_WINO2)) {
                a.out_layout = S3R_LAYOUT_WINO_HW;
                b.in_layout = S3R_LAYOUT_WINO_HW;
                const int rg = geometry(&a, &pl->g[i - 1]);              // (its output is now the plane sets)
                if (rg) return rg;
            }
            // ... and the small 3D layers: the producer's finish pass writes the consumer's plane sets / difference tensors
            bool take = false;
            const int lay = b.ndim == 3 ? handoff3d(a, b, &take) : S3R_LAYOUT_PLAIN;
            if (lay != S3R_LAYOUT_PLAIN) {
                s3r_conv_desc a2 = a;
                a2.out_layout = lay;
                Geo ga;
                const int rg = geometry(&a2, &ga);
                if (rg) return rg;
                // the region holds either form: its size must not follow the launch forms (they count the device's compute units)
                pl->region[i - 1] = ga.y_store > pl->g[i - 1].y_store ? ga.y_store : pl->g[i - 1].y_store;
                if (take) {
                    a = a2;
                    b.in_layout = lay;
                    pl->g[i - 1] = ga;
                }
            }
        }
        int rc = geometry(&pl->d[i], &pl->g[i]);
        if (rc) return rc;
        if ((rc = check_halos(&pl->d[i], pl->r[i]))) return rc;
        if (pl->d[i].dtype != pl->d[0].dtype) return fail(S3R_ERR_INVALID, "all layers of a chain must share one dtype");
        if (i > 0) {   // shapes must chain
            const s3r_conv_desc& a = pl->d[i - 1];
            const int64_t prev_out = (int64_t)a.cout * pl->g[i - 1].out_sp, cur_in = (int64_t)pl->d[i].cin * pl->g[i].in_sp;      // (logical sizes)
            if (prev_out != cur_in || a.batch != pl->d[i].batch)
                return fail(S3R_ERR_INVALID, "layer %d input (%lld/sample) does not match layer %d output (%lld/sample)", i,
                            (long long)cur_in, i - 1, (long long)prev_out);
            if (pl->d[i].in_halo && (pl->g[i - 1].out != pl->g[i].in || a.cout != pl->d[i].cin))
                return fail(S3R_ERR_INVALID, "layer %d needs a halo but reshapes layer %d's output", i, i - 1);
        }
    }
    plan_head_fusion(pl, n);
    return plan_arena(pl, n, user_in_halo, need0);
}

}  // namespace s3rh

extern "C" int64_t s3r_chain_workspace_elems(const s3r_layer* layers, int n_layers) {
    s3rh::Plan pl;
    const int rc = s3rh::plan_chain(layers, n_layers, &pl);
    return rc ? rc : pl.total;
}
