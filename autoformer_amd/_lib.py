"""ctypes binding of libautovc_hip.so (the C-ABI declared in include/autovc_hip.h).

The library is loaded lazily, *after* ``import torch``, so the process has exactly one
HIP runtime (torch's libamdhip64.so.7 satisfies the .so's NEEDED entry).  There is no
fallback: if the library is missing or fails to load, every op raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

import torch  # noqa: F401  (must precede the HIP library)

HERE = os.path.dirname(os.path.abspath(__file__))
# AVC_LIB_PATH: another build of the same ABI (same-box A/B timing of two builds, tools/ only)
LIB_PATH = os.environ.get("AVC_LIB_PATH") or os.path.join(HERE, "libautovc_hip.so")
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["gemm_ring.hip", "conv_ring.hip", "gemm_conv.hip", "gemm_nt.hip", "gemm_tt.hip", "gemm.hip", "bn.hip", "lstm.hip", "lstm_small.hip", "lstm_persist.hip", "lstm_infer.hip", "lstm2.hip", "elem.hip", "norm.hip", "variants.hip", "melgan.hip", "fold.hip", "disc.hip", "events.hip", "metadv.hip", "audio.hip", "resample.hip", "bn_seg.hip", "seg_moments.hip", "ragged.hip", "melgan_ragged.hip", "ge2e.hip", "xent.hip", "critic_loss.hip", "cycle_loss.hip"]
ABI_VERSION = 31

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_TANH, ACT_LEAKY, ACT_GELU, ACT_SIGMOID = 0, 1, 2, 3, 4, 5

c_void_p, c_int, c_ll, c_float, c_size = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t


class Operand(ctypes.Structure):
    _fields_ = [("ptr", c_void_p), ("dtype", c_int), ("kstrided", c_int), ("ld", c_ll), ("batch_stride", c_ll),
                ("taps", c_int), ("pad", c_int), ("t_out", c_int), ("t_in", c_int), ("chans", c_int)]


class GemmDesc(ctypes.Structure):
    _fields_ = [("M", c_int), ("N", c_int), ("K", c_int), ("batch", c_int), ("a", Operand), ("b", Operand),
                ("c", c_void_p), ("ldc", c_ll), ("c_batch_stride", c_ll), ("bias", c_void_p),
                ("accumulate", c_int), ("split_k", c_int), ("bn_partial", c_void_p), ("compute", c_int),
                ("c_bf16", c_void_p), ("residual", c_void_p), ("cperm", c_int), ("row_bias", c_void_p),
                ("rb_t", c_int), ("rb_pad", c_int), ("c_bf16_act", c_int), ("act_grad_of", c_void_p),
                ("col_sum", c_void_p), ("col_sum_n", c_int), ("c_pre_bf16", c_void_p), ("act_grad_dtype", c_int),
                ("c_trans_rows", c_int)]


class BnFin(ctypes.Structure):
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("num_batches_tracked", c_void_p), ("momentum", c_float), ("eps", c_float), ("nupd", c_int),
                ("mean", c_void_p), ("rstd", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("apply_bf16", c_void_p), ("apply_act", c_int)]


class BnbArgs(ctypes.Structure):
    _fields_ = [("y", c_void_p), ("y_dtype", c_int), ("mean", c_void_p), ("rstd", c_void_p), ("gamma", c_void_p),
                ("beta", c_void_p), ("act", c_int), ("coef", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("dbias", c_void_p), ("accumulate", c_int), ("ws", c_void_p), ("dy_bf16", c_void_p)]


class PackOp(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("src2", c_void_p), ("dst", c_void_p), ("kind", c_int), ("out_dtype", c_int),
                ("d0", c_int), ("d1", c_int), ("d2", c_int), ("pad_", c_int), ("ld_out", c_ll),
                ("ci0", c_int), ("cn", c_int), ("cpad", c_int), ("mode", c_int)]


PACK_COPY, PACK_TRANSPOSE, PACK_CONV_F, PACK_CONV_D, PACK_ADD, PACK_CONV_SLICE = 0, 1, 2, 3, 4, 5


_SIGS = {
    "avc_abi_version": (c_int, []),
    "avc_last_error": (ctypes.c_char_p, []),
    "avc_ring_reserve_test": (ctypes.c_uint, [ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.c_uint]),
    "avc_gemm": (c_int, [ctypes.POINTER(GemmDesc), c_void_p]),
    "avc_expand_codes": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_code_cat": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_gemm_bn": (c_int, [ctypes.POINTER(GemmDesc), ctypes.POINTER(BnFin), c_void_p]),
    "avc_bn_finalize": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_bn_eval": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "avc_bn_stats": (c_int, [c_void_p, c_ll, c_int, c_int, c_void_p, c_void_p]),
    "avc_bn_apply": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                              c_void_p]),
    "avc_gemm_bnb_ws": (c_size, [c_int, c_int]),
    "avc_gemm_bnb": (c_int, [ctypes.POINTER(GemmDesc), ctypes.POINTER(BnbArgs), c_void_p]),
    "avc_bn_bwd_apply": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p]),
    "avc_bn_bwd_ws": (c_size, [c_int, c_int]),
    "avc_bn_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                           c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                           c_void_p]),
    "avc_colsum_ws": (c_size, [c_int, c_int]),
    "avc_colsum": (c_int, [c_void_p, c_ll, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "avc_lstm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_int, c_void_p]),
    "avc_lstm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "avc_lstm_fwd_fold": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "avc_lstm_bwd_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_lstm_bwd_scratch_bytes": (c_size, [c_int, c_int, c_int]),
    "avc_lstm2_persistent": (c_int, [c_int, c_int, c_int, c_int]),
    "avc_lstm2_scratch_bytes": (c_size, [c_int, c_int]),
    "avc_lstm2_fwd": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 10),
    "avc_lstm_trace": (c_int, [c_void_p]),
    "avc_set_fault_word": (c_int, [c_void_p]),
    "avc_lstm_set_spin": (c_int, [ctypes.c_uint]),
    "avc_gemm_set_ring": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "avc_gemm_ring_last": (c_int, []),
    "avc_gemm_last_path": (c_int, []),
    "avc_lstm2_bwd_persistent": (c_int, [c_int, c_int, c_int]),
    "avc_lstm2_bwd_scratch_bytes": (c_size, [c_int, c_int]),
    "avc_lstm2_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                              c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_lstm_persistent": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "avc_lstm_infer_persistent": (c_int, [c_int, c_int, c_int]),
    "avc_lstm_infer_scratch_bytes": (c_size, [c_int, c_int, c_int]),
    "avc_lstm_infer": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "avc_lstm_small_mfma": (c_int, [c_int, c_int]),
    "avc_lstm_set_small_mfma": (c_int, [c_int]),
    "avc_enc_concat": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_codes_gather": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_codes_scatter": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_dec_concat": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_dec_concat_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_conv_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_conv_grad_unpack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_event_create": (c_int, [c_void_p]),
    "avc_event_record": (c_int, [c_void_p, c_void_p]),
    "avc_stream_wait_event": (c_int, [c_void_p, c_void_p]),
    "avc_conv_pack_slice": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p]),
    "avc_conv_edge_table": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "avc_conv_edge_colsum": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "avc_conv_grad_unpack_slice": (c_int, [c_void_p, c_ll, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p]),
    "avc_disc_dense_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "avc_disc_dense_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "avc_convert": (c_int, [c_void_p, c_void_p, c_int, c_ll, c_void_p]),
    "avc_transpose": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_ll, c_void_p]),
    "avc_add": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    "avc_mse_loss": (c_int, [c_void_p, c_void_p, c_ll, c_void_p, c_void_p]),
    "avc_l1_loss": (c_int, [c_void_p, c_void_p, c_ll, c_void_p, c_void_p]),
    "avc_loss_grad": (c_int, [c_void_p, c_void_p, c_ll, c_void_p, c_int, c_void_p, c_float, c_void_p]),
    "avc_vc_loss_ws": (c_size, []),
    "avc_vc_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_float, c_void_p, c_void_p,
                            c_void_p]),
    "avc_vc_loss_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_float, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_pack_batch": (c_int, [c_void_p, c_void_p, c_int, c_ll, c_void_p]),
    "avc_adam_blocks": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                c_void_p, c_int, c_int, c_void_p]),
    "avc_adam": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_void_p,
                         c_int, c_void_p]),
    "avc_act_fwd": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_void_p]),
    "avc_act_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p]),
    "avc_bce_loss": (c_int, [c_void_p, c_ll, c_float, c_void_p, c_void_p]),
    "avc_bce_grad": (c_int, [c_void_p, c_ll, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "avc_norm_ws": (c_size, [c_int, c_int]),
    "avc_group_norm_fwd": (c_int, [c_void_p, c_int, c_ll, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "avc_group_norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll, c_int, c_void_p,
                                   c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "avc_layer_norm_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "avc_layer_norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "avc_group_norm_fwd2": (c_int, [c_void_p, c_int, c_ll, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_layer_norm_fwd2": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    "avc_layer_norm_bwd2": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "avc_gelu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    "avc_pool3_mixer": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_patchify": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_patchify16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_transpose_batched": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_transpose_batched2": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "avc_moments_ws": (c_size, []),
    "avc_moments": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, c_void_p]),
    "avc_moments_bwd": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_adain_fwd": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_adain_bwd": (c_int, [c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p]),
    "avc_segsum": (c_int, [c_void_p, c_ll, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "avc_mg_gather": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                              c_void_p, c_int, c_void_p]),
    "avc_mg_act": (c_int, [c_void_p, c_ll, c_float, c_void_p, c_void_p, c_void_p]),
    "avc_mg_wn_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                               c_int, c_void_p, c_void_p]),
    "avc_mg_conv_out": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                c_void_p]),
    "avc_step_select": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_rownorm_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "avc_rownorm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "avc_dvec_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "avc_crop_add": (c_int, [c_void_p, c_ll, c_void_p, c_int, c_int, c_void_p]),
    "avc_pad_cols": (c_int, [c_void_p, c_ll, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "avc_gelu_twin": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p]),
}

# avc_gemm_last_path's encoding (the AVC_PATH_* enum of include/autovc_hip.h): family in bits 0-3,
# variant in bits 4-7 (fast / nt: 1 = 64-column tiles, 2 = 128; tt: 1 plain, 2 window stream, 3 halo;
# ring: avc_gemm_ring_last's 1 gemm / 2 halo conv / 3 one-utterance conv), then the flag bits.
PATH_GENERIC, PATH_FAST, PATH_NT, PATH_CONV, PATH_TT, PATH_RING = 1, 2, 3, 4, 5, 6
PATH_VARIANT_SHIFT = 4
PATH_SPLITK_WS, PATH_POST_PASS, PATH_WINDOW, PATH_BNB = 0x100, 0x200, 0x400, 0x800


# The MetaDV entry points of include/autovc_hip_dv.h: a second header and a second table, added without
# an ABI bump (autovc_hip.h, ABI_VERSION and exported_symbols() are as they were); lib() binds both.
c_int_p = ctypes.POINTER(c_int)
_SIGS_DV = {
    "avc_crop_windows": (c_int, [c_void_p, c_int, c_int_p, c_void_p, c_int_p, c_int, c_int, c_int, c_int, c_int,
                                 c_void_p, c_int, c_void_p]),
    "avc_crop_windows_bwd": (c_int, [c_void_p, c_void_p, c_int_p, c_void_p, c_int_p, c_void_p, c_int, c_int, c_int,
                                     c_int, c_int, c_void_p, c_void_p]),
    "avc_chan_mean": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "avc_chan_mean_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "avc_metadv_head": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_int, c_void_p, c_void_p, c_void_p]),
}

# The waveform -> log-mel entry point of include/autovc_hip_audio.h: a third header and a third table,
# added the same way (no ABI bump; the first two tables are as they were); lib() binds all three.
MEL_FRAME_MAJOR, MEL_CHANNEL_MAJOR = 0, 1
MEL_MAX_WEIGHTS = 8192
_SIGS_AUDIO = {
    "avc_audio2mel": (c_int, [c_void_p, c_ll, c_int_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int_p, c_void_p,
                              c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_void_p]),
}

# The sample-rate converter of include/autovc_hip_resample.h: a fourth header and a fourth table, added the
# same way (no ABI bump; the first three tables are as they were); lib() binds all four.
RESAMPLE_MAX_WEIGHTS = 131072
_SIGS_RESAMPLE = {
    "avc_resample": (c_int, [c_void_p, c_ll, c_int_p, c_void_p, c_int, c_void_p, c_int, c_int_p, c_void_p, c_int, c_int,
                             c_int, c_void_p, c_ll, c_void_p]),
    "avc_resample_tile": (c_int, [c_int, c_int, c_int]),
}

# Per-utterance BatchNorm of include/autovc_hip_eval.h: a fifth header and a fifth table, added the same
# way (no ABI bump; the first four tables are as they were); lib() binds all five.
BN_SEG_LDS_ROWS = 240
_SIGS_EVAL = {
    "avc_bn_seg_apply": (c_int, [c_void_p, c_int, c_ll, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# Per-segment moments and AdaIN of include/autovc_hip_seg.h: a sixth header and a sixth table, added the same
# way (no ABI bump; the first five tables are as they were); lib() binds all six.
SEG_MOMENTS_LDS_FLOATS = 16368
_SIGS_SEG = {
    "avc_seg_moments": (c_int, [c_void_p, c_int, c_ll, c_void_p, c_void_p]),
    "avc_adain_seg": (c_int, [c_void_p, c_int, c_ll, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# The ragged-batch kernels of include/autovc_hip_ragged.h: a seventh header and a seventh table, added the
# same way (no ABI bump; the first six tables are as they were); lib() binds all seven.
_SIGS_RAGGED = {
    "avc_bn_seg_ragged": (c_int, [c_void_p, c_int, c_ll, c_int, c_int, c_int, c_int_p, c_void_p, c_void_p, c_void_p,
                                  c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "avc_row_mask": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int_p, c_void_p, c_void_p]),
    "avc_bilstm_ragged_fwd": (c_int, [c_void_p, c_void_p, c_int_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_int, c_void_p]),
}

# The ragged-batch MelGAN glue of include/autovc_hip_vocoder.h: an eighth header and an eighth table, added the
# same way (no ABI bump; the first seven tables are as they were); lib() binds all eight.
_SIGS_VOCODER = {
    "avc_mg_gather_ragged": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int_p,
                                     c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "avc_mg_act_ragged": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "avc_mg_conv_out_ragged": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int_p,
                                       c_void_p, c_int, c_void_p, c_void_p]),
}

# The GE2E loss of include/autovc_hip_ge2e.h: a ninth header and a ninth table, added the same way (no ABI
# bump; the first eight tables are as they were); lib() binds all nine.
GE2E_MAX_N, GE2E_MAX_M, GE2E_MAX_D, GE2E_MAX_ROWS = 1024, 1024, 2048, 8192
_SIGS_GE2E = {
    "avc_ge2e_ws": (c_size, [c_int, c_int, c_int]),
    "avc_ge2e": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# Softmax cross-entropy of include/autovc_hip_xent.h: a tenth header and a tenth table, added the same way (no
# ABI bump; the first nine tables are as they were); lib() binds all ten.
XENT_MAX_B, XENT_MAX_C = 65536, 16384
_SIGS_XENT = {
    "avc_xent_ws": (c_size, [c_int, c_int]),
    "avc_xent": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p,
                         c_void_p, c_void_p]),
}

# The critic step's loss tail of include/autovc_hip_critic.h: an eleventh header and an eleventh table, added the
# same way (no ABI bump; the first ten tables are as they were); lib() binds all eleven.
CRITIC_MAX_B, CRITIC_MAX_E, CRITIC_MAX_N = 4096, 4096, 65536
_SIGS_CRITIC = {
    "avc_critic_loss_ws": (c_size, [c_int]),
    "avc_critic_loss": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "avc_critic_loss_grad": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_void_p, c_void_p, c_void_p]),
}

# The cycle step's loss tail of include/autovc_hip_cycle.h: a twelfth header and a twelfth table, added the same
# way (no ABI bump; the first eleven tables are as they were); lib() binds all twelve.
CYCLE_MAX_NX, CYCLE_GRID = 2 ** 31 - 1, 256
_CYCLE_IN = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
             c_int, c_void_p, c_void_p, c_ll]
_SIGS_CYCLE = {
    "avc_cycle_loss_ws": (c_size, [c_int, c_ll]),
    "avc_cycle_loss": (c_int, _CYCLE_IN + [c_void_p, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "avc_cycle_loss_grad": (c_int, _CYCLE_IN + [c_float, c_float, c_float, c_void_p] + [c_void_p] * 6
                            + [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
}

_lib = None
_lock = threading.Lock()


def build(verbose: bool = False, force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libautovc_hip.so (in-tree)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    if not force and os.path.exists(LIB_PATH):
        import glob

        # every header a translation unit includes (csrc/*.h, the public ABI header)
        deps = srcs + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "..", "include", h)
                                                              for h in ("autovc_hip.h", "autovc_hip_dv.h",
                                                                        "autovc_hip_audio.h",
                                                                        "autovc_hip_resample.h",
                                                                        "autovc_hip_eval.h", "autovc_hip_seg.h",
                                                                        "autovc_hip_ragged.h",
                                                                        "autovc_hip_vocoder.h",
                                                                        "autovc_hip_ge2e.h", "autovc_hip_xent.h",
                                                                        "autovc_hip_critic.h",
                                                                        "autovc_hip_cycle.h")]
        newest = max(os.path.getmtime(p) for p in deps)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = LIB_PATH + ".tmp"
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed"]
    objdir = os.path.join(HERE, "_build")
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, os.path.basename(p) + ".o") for p in srcs]
    # one hipcc per translation unit, concurrently (the gfx950 device compile dominates)
    procs = []
    for src, obj in zip(srcs, objs):
        cmd = [hipcc] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    failed = [cmd for cmd, pr in procs if pr.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs, check=True, cwd=CSRC)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libautovc_hip.so not found at {LIB_PATH}; run autoformer_amd._lib.build() "
                               "(or __graft_entry__.build()). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in (list(_SIGS.items()) + list(_SIGS_DV.items()) + list(_SIGS_AUDIO.items())
                                  + list(_SIGS_RESAMPLE.items()) + list(_SIGS_EVAL.items()) + list(_SIGS_SEG.items())
                                  + list(_SIGS_RAGGED.items()) + list(_SIGS_VOCODER.items())
                                  + list(_SIGS_GE2E.items()) + list(_SIGS_XENT.items())
                                  + list(_SIGS_CRITIC.items()) + list(_SIGS_CYCLE.items())):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        v = L.avc_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libautovc_hip ABI {v} != expected {ABI_VERSION}; rebuild")
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().avc_last_error().decode(errors="replace")
        raise RuntimeError(f"libautovc_hip {what} failed ({rc}): {msg}")


_FNS = {}  # name -> bound ctypes function (one dict lookup per launch instead of lib() + getattr)


_REC = None  # a replay.StepRecord while a step is being recorded (replay.recording)


def call(name: str, *args) -> None:
    fn = _FNS.get(name)
    if fn is None:
        fn = _FNS[name] = getattr(lib(), name)
    rc = fn(*args)
    if rc != 0:
        check(rc, name)
    if _REC is not None:
        _REC.add_native(fn, name, args)


def exported_symbols():
    return list(_SIGS.keys())


def exported_symbols_dv():
    """The entry points of include/autovc_hip_dv.h (the MetaDV kernels)."""
    return list(_SIGS_DV.keys())


def exported_symbols_audio():
    """The entry points of include/autovc_hip_audio.h (waveform -> log-mel)."""
    return list(_SIGS_AUDIO.keys())


def exported_symbols_resample():
    """The entry points of include/autovc_hip_resample.h (band-limited sample-rate conversion)."""
    return list(_SIGS_RESAMPLE.keys())


def exported_symbols_eval():
    """The entry points of include/autovc_hip_eval.h (per-utterance BatchNorm)."""
    return list(_SIGS_EVAL.keys())


def exported_symbols_seg():
    """The entry points of include/autovc_hip_seg.h (per-segment moments and AdaIN)."""
    return list(_SIGS_SEG.keys())


def exported_symbols_ragged():
    """The entry points of include/autovc_hip_ragged.h (ragged batches of whole utterances)."""
    return list(_SIGS_RAGGED.keys())


def exported_symbols_vocoder():
    """The entry points of include/autovc_hip_vocoder.h (the MelGAN generator over ragged batches)."""
    return list(_SIGS_VOCODER.keys())


def exported_symbols_ge2e():
    """The entry points of include/autovc_hip_ge2e.h (the GE2E loss and its gradients)."""
    return list(_SIGS_GE2E.keys())


def exported_symbols_xent():
    """The entry points of include/autovc_hip_xent.h (softmax cross-entropy, its gradient, the top-1 count)."""
    return list(_SIGS_XENT.keys())


def exported_symbols_critic():
    """The entry points of include/autovc_hip_critic.h (the critic step's fused loss tail and its gradients)."""
    return list(_SIGS_CRITIC.keys())


def exported_symbols_cycle():
    """The entry points of include/autovc_hip_cycle.h (the cycle step's fused loss tail and its gradients)."""
    return list(_SIGS_CYCLE.keys())
