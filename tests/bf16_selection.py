"""The cases tests/test_gpu_bf16_flavour.py runs against libladiff_hip_bf16.so.  TEST INFRASTRUCTURE ONLY: plain data.

For each split-mode kernel family the smallest existing cases at which the family can still go wrong (the f16x3-parametrised ids: every
split-mode name selects the loaded library's pairs), and the range cases of tests/test_gpu_range.py - operands beyond fp16's range,
the reason the bf16-pair library exists.  Node ids are relative to the repository root."""

K = "tests/test_gpu_kernels.py::"
TL = "tests/test_gpu_trained_like.py::"
DP = "tests/test_gpu_dec_post.py::"
ENC = "tests/test_gpu_encoder_shapes.py::"
CLIP = "tests/test_gpu_clip_shapes.py::"
NT = "tests/test_gpu_ntext_shapes.py::"
RG = "tests/test_gpu_range.py::"

FAMILIES = {
    "format": [
        K + "test_split_format_round_trip",
        K + "test_split_operands_saturate_instead_of_overflowing",
    ],
    "K-resident split GEMM": [
        K + "test_gemm_resident_split[77-1024-256-relu]",            # K = 256 with bias, residual, activation; M = 77
        K + "test_gemm_resident_split[1280-256-1024-none]",          # split-K planes at K = 1024
        K + "test_gemm_resident_split[90-256-512-none]",             # K = 512, M = 90
        K + "test_gemm_resident_split_k_and_combine[90-512-True]",   # concat at K = 512
        K + "test_split_products_of_small_operands_per_element[resident]",
    ],
    "large-M split GEMM": [
        K + "test_gemm_split_large_m[4100-256-256-none-False-True]",
        K + "test_gemm_split_large_m[4099-256-1024-none-False-True]",
        K + "test_gemm_split_large_m[4160-256-512-none-True-False]",
        K + "test_gemm_split_large_m[300-768-768-qgelu-False-True]",
        K + "test_gemm_split_large_m[1-128-64-lrelu-False-False]",
        K + "test_split_products_of_small_operands_per_element[large_m]",
    ],
    "combine rows + LayerNorm / Stylization": [
        K + "test_gemm_resident_split_k_and_combine[45-1024-False]",
        K + "test_gemm_resident_split_k_and_combine[90-512-True]",
        K + "test_combine_rows_offset_rows[40-2]",
        K + "test_combine_rows_offset_rows[45-4]",
    ],
    "split self-attention": [
        K + "test_self_attention_split[lengths1-4-0]",               # [1, 33, 32, 31, 101]
        K + "test_self_attention_split[lengths5-12-1]",              # causal, [20, 20] x 12 heads
        K + "test_self_attention_split_key_bitmap_matches_fp32_kernel",
    ],
    "in_proj inside the attention kernel": [
        K + "test_attention_with_in_proj_inside_matches_two_launches[lens2]",      # [1]
        K + "test_attention_with_in_proj_inside_matches_two_launches[lens1]",      # the 12-length mixed batch
    ],
    "fused feed-forward": [K + f"test_fused_mlp_layernorm[{m}-{v}]" for m in ("1-False", "17-True") for v in range(4)] + [
        K + "test_fused_mlp_layernorm_offset_rows[40-False-x]",
        K + "test_fused_mlp_layernorm_offset_rows[45-True-b2]",
    ],
    "one-launch layer tail": [
        DP + "test_one_launch_layer_tail[two-False-1-196]",             # lengths [17, 15], T = 1
        DP + "test_one_launch_layer_tail[two-True-1-196]",
        DP + "test_one_launch_layer_tail_251_features[False]",
        DP + "test_one_launch_layer_tail_251_features[True]",
    ],
    "decoder routing switches": [TL + f"test_decoder_every_kernel_routing[{f}-f16x3]" for f in (0, 1, 2, 5, 9, 17, 33, 65)],
    "decoder memory-token counts": [TL + f"test_decoder_memory_token_counts[{t}-f16x3]" for t in ("1-224", "3-80", "8-25")],
    "trained-like denoiser forward": [TL + f"test_denoiser_forward[{bt}-{m}-981-f16x3]" for bt in ("1-1", "7-3", "37-5")
                                      for m in (True, False)],
    "linear_ca": [
        TL + "test_denoiser_forward_many_text_tokens[4]",
        TL + "test_denoiser_forward_many_text_tokens[77]",
        NT + "test_token_counts[tokens4-trained-f16x3]",
        NT + "test_token_counts[tokens77-trained-f16x3]",
    ],
    "sampling loop": [TL + f"test_sampling_loop[{form}-{b}-f16x3]" for b in (3, 7) for form in (
        "launches-True", "pipeline32-True", "pipeline16-True", "pipeline16-False", "pipeline-True", "None-True")] + [
        TL + "test_sampling_loop_without_guidance[f16x3]",
    ],
    "encoder shapes": [ENC + f"test_length_edges[{n}-263-trained-f16x3]" for n in (
        "len1", "one_wave_S32", "S33", "S33_B3", "M64", "M65")] + [
        ENC + f"test_sequences_of_at_most_8_rows[{n}-trained-f16x3]" for n in ("T1-F1", "T1-F5", "T2-F3", "T3-F1", "T3-F2")],
    "CLIP shapes": [
        CLIP + "test_one_row_prompts_and_narrow_ids[S1-trained-f16x3]",
        CLIP + "test_one_row_prompts_and_narrow_ids[S33-trained-f16x3]",
        CLIP + "test_routes_by_row_count[ragged256-trained-f16x3]",
    ],
    "attention maps": ["tests/test_gpu_att_maps.py::test_maps_against_the_fp64_restatement[a_ragged_small-trained_like-f16x3]"],
    "trajectory": ["tests/test_gpu_trajectory.py::test_every_row_matches_the_oracle_and_not_its_neighbours[launches-f16x3-ddim]"],
    "DPM-Solver++": ["tests/test_gpu_dpm_solver.py::test_loop_matches_the_oracle_and_not_its_first_order_run[launches-f16x3]"],
    # (test_every_prompt_matches_the_oracle_restarted_at_its_own_start computes a 6 s CPU reference for its module in a process of its own)
    "edit": ["tests/test_gpu_edit.py::test_edit_from_a_motion_matches_the_oracle_chain[f16x3]"],
    "per-prompt parameters": [
        "tests/test_gpu_prompt_params.py::test_per_prompt_guidance_matches_the_oracle_prompt_by_prompt[launches-f16x3]"],
    "operands beyond fp16's range": (
        [RG + f"test_range_case[{n}-{p}]" for n in (
            "decode_1e5", "decode_1e5_trained", "decode_1e8", "decode_1e8_trained", "denoiser_sample_1e5", "denoiser_text_1e5",
            "denoiser_both_1e5", "denoiser_both_1e5_trained", "denoiser_both_1e5_ntext4", "encode_1e5") for p in ("fp32", "f16x3")] +
        [RG + f"test_gemm_resident_split_beyond_fp16[{s}-{a}]" for s in ("77-256-256", "90-256-512")
         for a in ("300000.0-1.0", "1e+30-1e-10")] +
        [RG + f"test_gemm_split_large_m_beyond_fp16[{s}-{a}]" for s in ("130-128-256", "1-128-64")
         for a in ("300000.0-1.0", "1e+30-1e-10")] +
        [RG + "test_self_attention_split_values_beyond_fp16"]),
}

SELECTION = []                      # (family, node id), every id once (a case that serves two families is listed under the first)
for _family, _ids in FAMILIES.items():
    for _i in _ids:
        if all(_i != s for _, s in SELECTION):
            SELECTION.append((_family, _i))
