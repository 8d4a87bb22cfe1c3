"""Ledger of direct tests per entry point of include/autovc_hip.h (CPU; no compute).

Every declared symbol maps either to the tests that call it directly -- through _lib.call / lib(), its
autoformer_amd.kernels wrapper, or the thin autograd op around that wrapper -- as "file::function", or to a
string saying why it has none.  A new entry point fails here until it has a direct test or a stated reason;
a renamed or deleted test fails here until the ledger follows."""
import ast
import os

from .conftest import ROOT
from .test_abi import declared_symbols

K_ = "test_gpu_kernels.py::"
E_ = "test_gpu_elem_direct.py::"
R_ = "test_gpu_reduce_direct.py::"
N_ = "test_gpu_norm_paths.py::"
G_ = "test_gpu_melgan_glue.py::"
M_ = "test_gpu_metaformer.py::"
I_ = "test_gpu_lstm_infer.py::"
P_ = "test_gpu_lstm_paths.py::"

EVENT = ("host-side event helper: no kernel; the ordering it gives is what tests/test_gpu_replay.py checks "
         "end to end")
SIZE_QUERY = "size query: no launch; its value sizes the workspace of every direct test of %s"

LEDGER = {
    # version / error channel
    "avc_abi_version": ["test_abi.py::test_abi_version_and_error_channel", E_ + "test_abi_version_unchanged"],
    "avc_last_error": ["test_abi.py::test_abi_version_and_error_channel",
                       "test_abi.py::test_argument_validation_without_gpu"],
    "avc_ring_reserve_test": ["test_abi.py::test_counter_ring_reservations_never_overlap"],
    # GEMM family
    "avc_gemm": [K_ + "test_gemm_plain_all_layouts", K_ + "test_gemm_bias_accumulate_splitk_batch",
                 K_ + "test_conv_gemm_fwd_dgrad_wgrad"],
    "avc_gemm_bn": [K_ + "test_gemm_bn_fused_finalize", K_ + "test_conv_bn_fused_finalize"],
    "avc_gemm_bnb": [K_ + "test_gemm_bnb_matches_separate_bn_backward"],
    "avc_gemm_bnb_ws": SIZE_QUERY % "avc_gemm_bnb",
    "avc_gemm_set_ring": ["test_gpu_ring.py::test_gelu_epilogues", "test_gpu_ring.py::test_conv_utterance_tile"],
    "avc_gemm_ring_last": ["test_gpu_ring.py::test_conv_utterance_tile"],
    "avc_gemm_last_path": ["test_gpu_gemm_paths.py::test_gemm_path", "test_gpu_gemm_paths.py::test_refusals_launch_nothing",
                           "test_abi.py::test_argument_validation_without_gpu"],
    # BatchNorm
    "avc_bn_finalize": [K_ + "test_bn_stats_epilogue_and_finalize", K_ + "test_bn_stats_plain"],
    "avc_bn_eval": [E_ + "test_bn_eval"],
    "avc_bn_stats": [K_ + "test_bn_stats_plain"],
    "avc_bn_apply": [K_ + "test_bn_act_forward_backward", K_ + "test_bn_apply_forms"],
    "avc_bn_bwd": [K_ + "test_bn_act_forward_backward", K_ + "test_bn_bf16_storage"],
    "avc_bn_bwd_ws": SIZE_QUERY % "avc_bn_bwd",
    "avc_bn_bwd_apply": [K_ + "test_gemm_bnb_matches_separate_bn_backward", K_ + "test_bn_apply_forms"],
    "avc_colsum": [R_ + "test_colsum"],
    "avc_colsum_ws": SIZE_QUERY % "avc_colsum",
    # LSTM
    "avc_lstm_fwd": [P_ + "test_lstm_per_step_forward_bf16", K_ + "test_lstm_persistent_forward_matches_per_step",
                     "test_gpu_bilstm_mfma.py::test_bilstm_mfma_matches_fp64"],
    "avc_lstm_bwd": [P_ + "test_lstm_per_step_backward_bf16", K_ + "test_lstm_persistent_backward_under_load",
                     "test_gpu_bilstm_mfma.py::test_bilstm_mfma_matches_fp64"],
    "avc_lstm_bwd_scratch_bytes": SIZE_QUERY % "avc_lstm_bwd",
    "avc_lstm_fwd_fold": ["test_gpu_fold.py::test_lstm_fold_kernels_match_expanded_launch"],
    "avc_lstm_bwd_fold": ["test_gpu_fold.py::test_lstm_fold_kernels_match_expanded_launch"],
    "avc_lstm2_persistent": [K_ + "test_lstm2_wavefront_forward"],
    "avc_lstm2_scratch_bytes": SIZE_QUERY % "avc_lstm2_fwd",
    "avc_lstm2_fwd": [K_ + "test_lstm2_wavefront_forward"],
    "avc_lstm2_bwd_persistent": ["test_gpu_lstm2_bwd.py::test_lstm2_wavefront_backward_matches_two_launches"],
    "avc_lstm2_bwd_scratch_bytes": SIZE_QUERY % "avc_lstm2_bwd",
    "avc_lstm2_bwd": ["test_gpu_lstm2_bwd.py::test_lstm2_wavefront_bias_partials_and_bf16_only_outputs"],
    "avc_lstm_persistent": ["test_gpu_fault.py::test_persistent_path_query_matches_occupancy"],
    "avc_lstm_infer_persistent": [I_ + "test_lstm_infer_matches_cpu_loop"],
    "avc_lstm_infer_scratch_bytes": SIZE_QUERY % "avc_lstm_infer",
    "avc_lstm_infer": [I_ + "test_lstm_infer_matches_cpu_loop", I_ + "test_lstm_infer_single_outputs",
                       I_ + "test_lstm_infer_refuses_bad_lens_on_the_host"],
    "avc_lstm_small_mfma": ["test_gpu_bilstm_mfma.py::test_bilstm_mfma_selection"],
    "avc_lstm_set_small_mfma": ["test_gpu_bilstm_mfma.py::test_bilstm_mfma_selection"],
    "avc_lstm_trace": "diagnostic hook: records clock samples of the persistent recurrences, computes nothing",
    "avc_set_fault_word": "hook: registered by every persistent LSTM launch; its effect is what "
                          "test_gpu_fault.py::test_forced_spin_timeout_raises_at_loss_read reads",
    "avc_lstm_set_spin": ["test_gpu_fault.py::test_forced_spin_timeout_raises_at_loss_read"],
    "avc_dvec_head": [I_ + "test_dvec_head_matches_fp64"],
    # glue / packs
    "avc_enc_concat": [K_ + "test_glue_kernels", E_ + "test_enc_concat_reads_a_column_slice_of_a_wider_buffer"],
    "avc_codes_gather": [K_ + "test_glue_kernels"],
    "avc_codes_scatter": [K_ + "test_glue_kernels"],
    "avc_dec_concat": [K_ + "test_glue_kernels"],
    "avc_dec_concat_bwd": [E_ + "test_dec_concat_bwd"],
    "avc_expand_codes": ["test_gpu_fold.py::test_lstm_fold_kernels_match_expanded_launch"],
    "avc_code_cat": [E_ + "test_code_cat"],
    "avc_conv_pack": [K_ + "test_conv_pack_matches_permute", K_ + "test_conv_pack_writes_inside_its_output"],
    "avc_conv_grad_unpack": [K_ + "test_conv_gemm_fwd_dgrad_wgrad"],
    "avc_conv_pack_slice": [K_ + "test_fold_kernels", K_ + "test_conv_pack_slice_output_padded"],
    "avc_conv_edge_table": [K_ + "test_fold_kernels"],
    "avc_conv_edge_colsum": [K_ + "test_fold_kernels"],
    "avc_conv_grad_unpack_slice": [K_ + "test_fold_kernels"],
    "avc_disc_dense_fwd": [K_ + "test_disc_dense_head"],
    "avc_disc_dense_bwd": [K_ + "test_disc_dense_head"],
    "avc_convert": [K_ + "test_pack_batch_matches_individual_packs"],
    "avc_transpose": [K_ + "test_pack_batch_matches_individual_packs"],
    "avc_add": [E_ + "test_add"],
    "avc_pack_batch": [K_ + "test_pack_batch_matches_individual_packs"],
    # losses / optimizer / activations
    "avc_mse_loss": [E_ + "test_mse_l1_loss"],
    "avc_l1_loss": [E_ + "test_mse_l1_loss"],
    "avc_loss_grad": [E_ + "test_loss_grad"],
    "avc_vc_loss_ws": SIZE_QUERY % "avc_vc_loss",
    "avc_vc_loss": [K_ + "test_vc_loss_block_matches_torch"],
    "avc_vc_loss_grad": [K_ + "test_vc_loss_block_matches_torch"],
    "avc_adam": [E_ + "test_adam_plain_entry_point"],
    "avc_adam_blocks": [E_ + "test_adam_sizes_default_blocks", E_ + "test_adam_one_block_paired_loop_single_vector_and_tail",
                        E_ + "test_adam_misaligned_views_take_the_scalar_form",
                        E_ + "test_adam_without_advance_uses_the_stored_step_size",
                        E_ + "test_adam_empty_slice_only_advances_the_state"],
    "avc_act_fwd": [E_ + "test_act_fwd", E_ + "test_gelu_dense_grid_seam_and_tails",
                    E_ + "test_act_fwd_refuses_unknown_codes"],
    "avc_act_bwd": [E_ + "test_act_bwd_from_output", E_ + "test_act_bwd_refuses_codes_without_a_from_output_derivative"],
    "avc_bce_loss": [E_ + "test_bce_loss"],
    "avc_bce_grad": [E_ + "test_bce_grad"],
    # MetaFormer blocks
    "avc_norm_ws": [N_ + "test_group_norm_bwd_stays_inside_its_workspace"],
    "avc_group_norm_fwd": [N_ + "test_group_norm_fwd_without_workspace"],
    "avc_group_norm_fwd2": [N_ + "test_group_norm_paths", N_ + "test_group_norm_bf16_twin"],
    "avc_group_norm_bwd": [N_ + "test_group_norm_paths", N_ + "test_group_norm_bwd_stays_inside_its_workspace",
                           N_ + "test_group_norm_bwd_refuses_what_its_workspace_cannot_hold"],
    "avc_layer_norm_fwd": [N_ + "test_layer_norm_plain_entry_points"],
    "avc_layer_norm_bwd": [N_ + "test_layer_norm_plain_entry_points"],
    "avc_layer_norm_fwd2": [N_ + "test_layer_norm_paths", N_ + "test_layer_norm_vector_only_forms"],
    "avc_layer_norm_bwd2": [N_ + "test_layer_norm_paths", N_ + "test_layer_norm_vector_only_forms",
                            N_ + "test_layer_norm_many_rows_grow_the_backward_block"],
    "avc_gelu_bwd": [E_ + "test_gelu_dense_grid_seam_and_tails", M_ + "test_gelu_fwd_bwd"],
    "avc_pool3_mixer": [M_ + "test_pool_mixer_fwd_bwd"],
    "avc_patchify": [M_ + "test_patchify_roundtrip"],
    "avc_patchify16": [M_ + "test_patchify_roundtrip"],
    "avc_transpose_batched": [M_ + "test_transpose_batched"],
    "avc_transpose_batched2": [M_ + "test_transpose_pad_bf16_source"],
    # AdaIN / Adjust variants
    "avc_moments_ws": SIZE_QUERY % "avc_moments",
    "avc_moments": [R_ + "test_moments_adain_tails_and_block_cap", R_ + "test_moments_of_one_element"],
    "avc_moments_bwd": [R_ + "test_moments_adain_tails_and_block_cap", R_ + "test_moments_of_one_element"],
    "avc_adain_fwd": [R_ + "test_moments_adain_tails_and_block_cap", R_ + "test_moments_adain_large_mean_small_spread"],
    "avc_adain_bwd": [R_ + "test_moments_adain_tails_and_block_cap", R_ + "test_moments_of_one_element"],
    "avc_segsum": [R_ + "test_segsum"],
    "avc_step_select": ["test_variants.py::test_gpu_rownorm_step_select_segsum_match_torch"],
    "avc_rownorm_fwd": [R_ + "test_rownorm_fwd_bwd"],
    "avc_rownorm_bwd": [R_ + "test_rownorm_fwd_bwd"],
    "avc_pad_cols": [E_ + "test_pad_cols"],
    "avc_crop_add": [E_ + "test_crop_add"],
    "avc_gelu_twin": [E_ + "test_gelu_twin"],
    # MelGAN
    "avc_mg_gather": [G_ + "test_mg_gather"],
    "avc_mg_act": [G_ + "test_mg_act"],
    "avc_mg_wn_pack": [G_ + "test_mg_wn_pack_conv", G_ + "test_mg_wn_pack_transposed"],
    "avc_mg_conv_out": [G_ + "test_mg_conv_out"],
    # events
    "avc_event_create": EVENT,
    "avc_event_record": EVENT,
    "avc_stream_wait_event": EVENT,
}


def _test_functions(path):
    tree = ast.parse(open(path).read())
    return {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}


def test_ledger_covers_exactly_the_declared_symbols():
    declared = set(declared_symbols())
    assert set(LEDGER) == declared, (sorted(declared - set(LEDGER)), sorted(set(LEDGER) - declared))


def test_ledger_entries_name_existing_tests_or_give_a_reason():
    cache, bad = {}, []
    for sym, entry in LEDGER.items():
        if isinstance(entry, str):
            if len(entry) < 20:
                bad.append((sym, "exemption without a reason"))
            continue
        if not entry:
            bad.append((sym, "no test listed"))
        for ref in entry:
            fname, func = ref.split("::")
            path = os.path.join(ROOT, "tests", fname)
            if not os.path.exists(path):
                bad.append((sym, ref, "no such file"))
                continue
            if fname not in cache:
                cache[fname] = _test_functions(path)
            if not func.startswith("test_") or func not in cache[fname]:
                bad.append((sym, ref, "no such test function"))
    assert not bad, bad
