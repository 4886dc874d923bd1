"""Kernel mutants: subtly wrong copies of the HIP kernels that the GPU suite must fail on.  Plain data.

Each entry: `id`; `file` under csrc/ (a translation unit of the Makefile's SRCS, or a header, which rebuilds its users);
`anchor`, a span of that file's text that occurs exactly once; `replacement` for it; `kills`, pytest arguments (node ids, at most
one `-k` expression) naming the tests meant to catch the defect, the likeliest first (the child stops at the first failure);
`models`, one sentence on the defect.  An entry with `equivalent` (a written argument) changes no observable bit: it still runs
and must survive.  tools/build_mutants.py builds build/mutants/<id>.so from a copy, tests/test_mutants_cpu.py keeps the table
honest without a GPU, tests/test_mutants_gpu.py runs each entry's kills on its library (S3R_LIB) and wants an assertion to fail.

Mutants change VALUES only: a constant, a sign, which already loaded element is used, a comparison's strictness, a rounding, a
sum's association, which math function is called, or one loop iteration less.  None touches an address computation so that it
could leave its range, a bound or mask that guards an address, a barrier, a wait count, an LDS-DMA call, a launch configuration,
a store's guard or inline assembly; none raises a trip count.  Summation-order mutants exist only where the order is the
contract (the backward kernels, s3r_ordered.h), never for the forward conv and linear kernels.
"""

EX = "tests/test_exact_gpu.py"

MUTANTS = [
    # ---- s3r_conv_glds.hip
    dict(id="glds_shift_dropped_ss", file="s3r_conv_glds.hip",
         anchor="ep_sf[tid] = (p.shift && m < p.Cout) ? p.shift[mc] : 0.f;",
         replacement="ep_sf[tid] = (p.shift && !p.scale && m < p.Cout) ? p.shift[mc] : 0.f;",
         kills=[EX + "::test_epilogue_forms", "-k", "ep-direct-epilogue or ep-tclass or ep-d2s"],
         models="The direct kernel's epilogue drops `shift` in the one NULL form where `scale` is given too."),
    dict(id="glds_splitk_last_slab", file="s3r_conv_glds.hip",
         anchor="for (; z < p.ksplit; ++z) {",
         replacement="for (; z < p.ksplit - 1; ++z) {",
         kills=[EX, "-k", "splitk2"],
         models="The split-K finish skips the last slab when the slabs are not a multiple of four."),
    dict(id="glds_tail_cut_one_tile_late", file="s3r_conv_glds.hip",
         anchor="(int)gridDim.x - p.big_wgs, p.n_cut, p.n_end, 0,",
         replacement="(int)gridDim.x - p.big_wgs, p.n_cut + 64, p.n_end, 0,",
         kills=["tests/test_launch_forms_gpu.py::test_launch_form_is_exact_and_is_the_planned_one"],
         models="The tail cut's re-tiled remainder starts one 64-position tile late: the first tile's outputs are never written "
                "(the tile past the end stores nothing: every store is guarded by n < n_end, every fetch clamped to it)."),
    dict(id="glds_leaky_is_relu", file="s3r_conv_glds.hip",
         anchor="MODE == 2 ? fmaxf(t, t * slope) : fmaxf(t, lo)",
         replacement="MODE == 2 ? fmaxf(t, 0.f * slope) : fmaxf(t, lo)",
         kills=["tests/test_general_gpu.py::test_rgb_first_layers_are_unfolded_and_leaky_relu_is_fused",
                EX + "::test_direct_fp32[leaky-half-fused-epilogue]"],
         models="The fused LeakyReLU of the direct epilogue is a plain ReLU."),
    # ---- s3r_wino.h and its units (s3r_wino_axis1 / _axis2 / _handoff.hip)
    dict(id="wino_bt_coefficient", file="s3r_wino_axis1.hip",
         anchor="        wino_rows_to_classes<R>(r, v);\n",
         replacement="        wino_rows_to_classes<R>(r, v);\n        v[3] = fmaf(3.f, r[3] - r[1], r[4] - r[2]);\n",
         kills=[EX + "::test_winograd_fp32", "-k", "wino1-serial"],
         models="One coefficient of the F(4,3) input transform (wino_rows_to_classes<4>, class 3: 2 -> 3) in the one-axis "
                "transform kernel."),
    dict(id="wino_at_coefficient", file="s3r_wino.h",
         anchor="y[3] = fmaf(8.f, d34, d12) + m[5];",
         replacement="y[3] = fmaf(6.f, d34, d12) + m[5];",
         kills=[EX + "::test_winograd_fp32", "-k", "wino1-class-parallel or wino1-serial"],
         models="One coefficient of the F(4,3) output transform that wino_finish_kernel and the serial form share (8 -> 6)."),
    dict(id="wino_f24_coefficient", file="s3r_wino.h",
         anchor="y[1] = fmaf(2.f, m[3], m[1] - m[2]) + m[4];",
         replacement="y[1] = fmaf(3.f, m[3], m[1] - m[2]) + m[4];",
         kills=[EX + "::test_winograd_fp32", "-k", "v6"],
         models="One coefficient of the F(2,4) output transform (2 -> 3)."),
    dict(id="wino2s_finish_drops_class", file="s3r_wino_axis2.hip",
         anchor="for (int a = 0; a < N; ++a) m[a] = src[(a * M + v) * 64];",
         replacement="for (int a = 0; a < N; ++a) m[a] = a == N - 1 ? 0.f : src[(a * M + v) * 64];",
         kills=[EX + "::test_winograd_fp32", "-k", "wino2-tile and (v1 or v3 or v5)"],
         models="The semi-fused two-axis finish (wino2s_finish_kernel) drops its last depth class; the class-parallel form stays right."),
    dict(id="wino_handoff_neighbour_class", file="s3r_wino_handoff.hip",
         anchor="p.y[(size_t)(a * N + c) * total + base + t] = v[a];",
         replacement="p.y[(size_t)(a * N + c) * total + base + t] = v[(a == 2 && c == 3) ? 1 : a];",
         kills=["tests/test_handoff3d_gpu.py::test_pair_equals_the_two_layers_run_singly"],
         models="wino_handoff_kernel writes plane set (2, 3) of its consumer's operand with the neighbouring depth class's value."),
    # ---- s3r_deconv_wino3.hip
    dict(id="dwino3_sum_sign", file="s3r_deconv_wino3.hip",
         anchor="z[1][0][r] = d3_put(d3_get(z[1][0][r]) - (acc[0][r] + acc[1][r]));",
         replacement="z[1][0][r] = d3_put(d3_get(z[1][0][r]) + (acc[0][r] + acc[1][r]));",
         kills=[EX + "::test_winograd_fp32", "-k", "wino3-tile"],
         models="One term of the three-axis kernel's running H-transform sums enters with the wrong sign."),
    dict(id="dwino3_head_last_channel", file="s3r_deconv_wino3.hip",
         anchor="ep[128 + tid] = (HEAD && p.head_w && m < p.Cout) ? p.head_w[m] : 0.f;",
         replacement="ep[128 + tid] = (HEAD && p.head_w && m < p.Cout - 1) ? p.head_w[m] : 0.f;",
         kills=[EX + "::test_chain_handoff", "-k", "dwino3"],
         models="The three-axis kernel's fused head skips its last input channel."),
    # ---- s3r_conv_bf16.hip
    dict(id="bf16_store_truncates", file="s3r_conv_bf16.hip",
         anchor="    const bf16x2 v = {(__bf16)lo, (__bf16)hi};      // one v_cvt_pk_bf16_f32 (round to nearest even)\n"
                "    return __builtin_bit_cast(unsigned, v);\n",
         replacement="    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);\n",
         kills=[EX + "::test_bf16", "-k", "tile22-conv3d_s1 or tile6-conv3d_s1 or tile1-conv3d_s1"],
         models="The bf16 epilogue's fp32 -> bf16 conversion truncates instead of rounding to nearest even."),
    dict(id="bf16_rowreuse_neighbour_tap", file="s3r_conv_bf16.hip",
         anchor="const int row = lr[pt] + tw;",
         replacement="const int row = lr[pt] + (tw == 1 ? 0 : tw);",
         kills=[EX + "::test_bf16", "-k", "mfma32x32x16 and (tile9 or tile10) and (conv3d_s1 or conv2d_s1)"],
         models="Tap 1 of the row-reuse kernel reads tap 0's LDS row of the gathered input."),
    # ---- s3r_pointwise.hip
    dict(id="stem_u8_scale_256", file="s3r_pointwise.hip",
         anchor="const float xv = v ? render_f32(xrow[iw]) : 0.f;",
         replacement="const float xv = v ? render_f32(xrow[iw]) * (sizeof(TI) == 1 ? 255.f / 256.f : 1.f) : 0.f;",
         kills=["tests/test_ingest_soak_gpu.py::test_u8_entry_equals_fp32_entry_bitwise_and_the_oracle",
                "tests/test_buffers_gpu.py::test_encoder_forward"],
         models="The stem scales 8-bit renders by 1/256 instead of 1/255."),
    dict(id="cvw2_right_half_sign", file="s3r_pointwise.hip",
         anchor="((in && w + d < W) ? sr[hw] - sl[hw + d] : 0.f)",
         replacement="((in && w + d < W) ? sr[hw] - sl[(d == 1 && w >= d) ? hw - d : hw + d] : 0.f)",
         kills=[EX + "::test_cost_volume_planes_feed_v1", "tests/test_wino_gpu.py::test_cost_volume_writes_the_transformed_planes_bitwise"],
         models="cost_volume_wino2_kernel shifts the right-view half with the left view's sign at disparity 1."),
    dict(id="head_sigmoid_unsymmetric", file="s3r_pointwise.hip",
         anchor="if (act == ACT_SIGMOID) return 1.f / (1.f + __expf(-v));",
         replacement="if (act == ACT_SIGMOID) return __expf(v) / (1.f + __expf(v));",
         kills=["tests/test_pointwise_math_gpu.py::test_sigmoid_per_element_over_the_whole_range"],
         models="The head's sigmoid in the form e^v / (1 + e^v): the same fast exponential the stock kernel already calls, but "
                "inf / inf past v = 88.7 and a cancelling 1 + e^v below."),
    dict(id="wta_last_minimum", file="s3r_pointwise.hip",
         anchor="if (cost < best) { best = cost; arg = d; }",
         replacement="if (cost <= best) { best = cost; arg = d; }",
         kills=["tests/test_selection_gpu.py::test_wta_takes_the_first_of_a_partly_shared_minimum"],
         models="The winner-take-all read-out takes the last of equal minima."),
    # ---- s3r_general.hip
    dict(id="elu_expf_minus_one", file="s3r_general.hip",
         anchor="param * expm1f(v)",
         replacement="param * (expf(v) - 1.f)",
         kills=["tests/test_pointwise_math_gpu.py::test_elu_per_element"],
         models="act_kernel's ELU as expf(v) - 1, which cancels for small |v|."),
    dict(id="tclass_unflipped_w", file="s3r_general.hip",
         anchor="const int tw = rw + stride * (krw - 1 - jw),",
         replacement="const int tw = rw + stride * ((krw == 2 && rw == 0) ? jw : krw - 1 - jw),",
         kills=[EX + "::test_epilogue_forms", "tests/test_general_gpu.py::test_transposed_layers_run_as_residue_classes", "-k",
                "ep-tclass or test_transposed_layers_run_as_residue_classes"],
         models="pack_tclass_kernel leaves the two-tap class of residue 0 unflipped along W."),
    # ---- s3r_ordered.h (rebuilds every translation unit that includes it)
    dict(id="ordered_wave_tree_ascending", file="s3r_ordered.h",
         anchor="for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);",
         replacement="for (int o = 1; o < 64; o <<= 1) v = v + __shfl_down(v, o, 64);",
         kills=["tests/test_head_backward_gpu.py", "tests/test_voxel_loss_gpu.py"],
         models="wave_tree walks its offsets 1, 2, .. 32: lane 0 still holds all 64 terms, in another association."),
    dict(id="ordered_row_total_descending", file="s3r_ordered.h",
         anchor="        for (int l = 0; l < n; ++l) {\n"
                "            const float v = __shfl(p, l, 64);\n"
                "            acc = (b0 + l == 0) ? v : acc + v;\n",
         replacement="        for (int l = n - 1; l >= 0; --l) {\n"
                     "            const float v = __shfl(p, l, 64);\n"
                     "            acc = (b0 == 0 && l == n - 1) ? v : acc + v;\n",
         kills=["tests/test_conv_backward_gpu.py", "tests/test_batchnorm_train_gpu.py"],
         models="row_total adds the samples of a wave in descending order."),
    dict(id="ordered_act_grad_reassociated", file="s3r_ordered.h",
         anchor="        const float u = y * t;\n        return gy * u;\n",
         replacement="        return (gy * y) * t;\n",
         kills=["tests/test_linear_backward_gpu.py", "tests/test_head_backward_gpu.py"],
         models="act_grad's sigmoid branch as (grad_y * y) * t instead of grad_y * (y * t)."),
    # ---- s3r_chamfer.hip
    dict(id="chamfer_tail_takes_last", file="s3r_chamfer.hip",
         anchor="if (dd < best[k]) { best[k] = dd; besti[k] = j0 + t; }",
         replacement="if (dd <= best[k]) { best[k] = dd; besti[k] = j0 + t; }",
         kills=["tests/test_selection_gpu.py", "-k", "chamfer"],
         models="The Chamfer search's tail loop takes the last of equal distances."),
    dict(id="chamfer_bwd_descending", file="s3r_chamfer.hip",
         anchor="                    for (int e = 0; e < BW_BLK; ++e)\n"
                "                        if (id[e] == tid[k]) bw_add(",
         replacement="                    for (int e = BW_BLK - 1; e >= 0; --e)\n"
                     "                        if (id[e] == tid[k]) bw_add(",
         kills=["tests/test_chamfer_backward_gpu.py"],
         models="The Chamfer backward adds the scattered terms of a block of eight sources in descending order."),
    # ---- s3r_disparity.hip
    dict(id="soft_flush_removed", file="s3r_disparity.hip",
         anchor="                if (e < FLT_MIN) e = 0.f;\n",
         replacement="",
         kills=["tests/test_disparity_soft_gpu.py::test_feature_resolution_matches_fp64",
                "tests/test_disparity_soft_gpu.py::test_cold_limit_is_the_wta_bit_for_bit",
                "tests/test_disparity_soft_gpu.py::test_a_weight_below_flt_min_counts_as_zero"],
         models="The soft read-out keeps subnormal weights instead of taking them as 0."),
    dict(id="metrics_bad3_not_strict", file="s3r_disparity.hip",
         anchor="n[2] += e > 3.f;",
         replacement="n[2] += e >= 3.f;",
         kills=["tests/test_selection_gpu.py::test_metrics_on_signed_zero_subnormal_and_overflowing_values",
                "tests/test_disparity_soft_gpu.py::test_metrics_match_numpy"],
         models="The metrics' 3-pixel count takes an error of exactly 3."),
    # ---- the backward kernels
    dict(id="bn_invstd_rsqrt", file="s3r_batchnorm.hip",
         anchor="o1[r] = 1.f / sqrtf(e);",
         replacement="o1[r] = rsqrtf(e);",
         kills=["tests/test_batchnorm_train_gpu.py"],
         models="BatchNorm's inverse standard deviation through rsqrtf instead of 1 / sqrtf."),
    dict(id="bce_clamp_99", file="s3r_voxel_loss.hip",
         anchor="return (v < -100.f) ? -100.f : v; }",
         replacement="return (v < -99.f) ? -99.f : v; }",
         kills=["tests/test_voxel_loss_gpu.py"],
         models="The BCE loss clamps its logarithms at -99 instead of -100."),
    dict(id="convbwd_slices_descending", file="s3r_conv_bwd.hip",
         anchor="for (int z = 1; z < nsl; ++z) p = p + src[(size_t)z * total];",
         replacement="for (int z = nsl - 1; z >= 1; --z) p = p + src[(size_t)z * total];",
         kills=["tests/test_conv_backward_gpu.py::test_k_slices_are_added_in_ascending_order"],
         models="The conv backward adds a sample's K slices in descending order."),
    dict(id="cvbwd_descending", file="s3r_cost_volume_bwd.hip",
         anchor="for (int d = 1; d < Dn; ++d) {",
         replacement="for (int d = Dn - 1; d >= 1; --d) {",
         kills=["tests/test_cost_volume_backward_gpu.py"],
         models="The cost-volume backward sums in descending disparity."),
]
