"""Whole-utterance conversion, the host side (no GPU): plan_whole, the wav-to-wav CLI's parser, the families
convert_whole refuses, and the ledger of the seventh ABI header (include/autovc_hip_ragged.h)."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

from .conftest import ROOT

HEADER_RAGGED = os.path.join(ROOT, "include", "autovc_hip_ragged.h")


# ----------------------------------------------------------------------- plan_whole
def _check_plan(lens, freq, max_batch, max_frames):
    from autoformer_amd.convert import padded_len, plan_whole

    plan = plan_whole(lens, freq, max_batch, max_frames)
    seen = [i for idx, _ in plan for i in idx]
    assert sorted(seen) == list(range(len(lens)))              # every index exactly once
    flat_p = [padded_len(lens[i], freq) for i in seen]
    assert flat_p == sorted(flat_p)                            # sorted by padded length
    for idx, Tmax in plan:
        P = [padded_len(lens[i], freq) for i in idx]
        assert Tmax == max(P) and Tmax % freq == 0 and all(p % freq == 0 and p >= lens[i] for p, i in zip(P, idx))
        assert 1 <= len(idx) <= max_batch
        assert len(idx) * Tmax <= max_frames or len(idx) == 1  # over budget only alone
    assert plan_whole(lens, freq, max_batch, max_frames) == plan   # deterministic
    return plan


def test_plan_whole_covers_caps_and_is_deterministic():
    rng = np.random.RandomState(0)
    for freq, max_batch, max_frames in ((8, 64, 16384), (22, 4, 1000), (16, 1, 50), (32, 7, 640)):
        _check_plan([int(v) for v in rng.randint(1, 700, size=41)], freq, max_batch, max_frames)
    assert _check_plan([], 8, 4, 100) == []


def test_plan_whole_single_over_budget_and_ties():
    from autoformer_amd.convert import MAX_FRAMES, plan_whole

    plan = _check_plan([40, 13, 24, 128, 5], 8, 2, 64)
    assert plan == [([4, 1], 16), ([2], 24), ([0], 40), ([3], 128)]            # 128 > 64 frames: alone
    assert plan_whole([40, 13, 24, 128, 5], 8) == [([4, 1, 2, 0, 3], 128)]
    assert plan_whole([9, 16, 10], 8) == [([0, 1, 2], 16)]                     # equal padded lengths: by index
    assert MAX_FRAMES == 16384
    with pytest.raises(ValueError):
        plan_whole([10], 8, max_batch=0)
    with pytest.raises(ValueError):
        plan_whole([0], 8)


# ----------------------------------------------------------------------- CLI parser
def test_cli_parser_required_and_exclusive_arguments(capsys):
    from autoformer_amd.convert import _parser, main

    p = _parser()
    a = p.parse_args(["--src", "a.wav", "b.wav", "--ref", "t.wav", "--out_dir", "o", "--det_init"])
    assert a.src == ["a.wav", "b.wav"] and a.src_dir is None and a.ref == ["t.wav"] and a.src_ref is None
    assert (a.model, a.dim_neck, a.dim_emb, a.dim_pre, a.freq) == ("AutoVC", 44, 256, 512, 22)
    assert (a.embedder, a.max_batch, a.dtype) == ("LstmDV", 64, "bf16")
    assert not a.resample and not a.save_mel
    for bad in (["--ref", "t.wav", "--out_dir", "o"],                                   # no source
                ["--src", "a.wav", "--src_dir", "d", "--ref", "t.wav", "--out_dir", "o"],  # both sources
                ["--src", "a.wav", "--out_dir", "o"],                                    # no target recordings
                ["--src", "a.wav", "--ref", "t.wav"],                                    # no out_dir
                ["--src", "a.wav", "--ref", "t.wav", "--out_dir", "o", "--embedder", "X"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    capsys.readouterr()
    base = ["--src", "a.wav", "--ref", "t.wav", "--out_dir", "o"]
    with pytest.raises(SystemExit, match="--ckpt"):
        main(base)
    with pytest.raises(SystemExit, match="--vocoder_ckpt"):
        main(base + ["--ckpt", "m", "--embedder_ckpt", "e"])
    with pytest.raises(SystemExit, match="GPU"):
        main(base + ["--det_init", "--device", "cpu"])
    assert "wav to wav" in p.format_help() and "--src_ref" in p.format_help()


# ----------------------------------------------------------------------- families
def test_convert_whole_refuses_other_families_by_message():
    """Before any kernel runs: the models stay on the CPU, no device is touched."""
    from autoformer_amd.convert import Converter, convert_whole
    from autoformer_amd.factory.AutoVC2 import AutoVC2
    from autoformer_amd.factory.AutoVC_Adjust import AutoVC_Adjust
    from autoformer_amd.factory.MetaConv import MetaConv

    mel, e = np.zeros((30, 80), np.float32), np.zeros(256, np.float32)
    for cls, needle in ((MetaConv, "Meta model"), (AutoVC2, "AdaIN variant"), (AutoVC_Adjust, "_Adjust variant")):
        m = cls(44, 256, 512, 22)
        with pytest.raises(NotImplementedError, match=needle) as ei:
            convert_whole(m, [mel], e, e)
        assert cls.__name__ in str(ei.value)
        with pytest.raises(NotImplementedError, match=needle):
            Converter(m, 176, "cpu").convert_whole(mel, e, e)


def test_per_utterance_bn_lens_argument():
    from autoformer_amd import layers as Lyr

    with pytest.raises(TypeError, match="kernels.Lens"):
        Lyr.per_utterance_bn(lens=[3, 4])
    assert Lyr.per_utterance_bn().lens is None and Lyr.ragged_lens() is None


# ----------------------------------------------------------------------- the seventh header's ledger
G_ = "test_gpu_ragged_kernels.py::"
LEDGER_RAGGED = {
    "avc_bn_seg_ragged": [G_ + "test_bn_against_fp64", G_ + "test_bn_output_forms",
                          G_ + "test_bn_full_lengths_match_bn_seg_apply_bit_for_bit",
                          G_ + "test_bn_segments_are_independent", G_ + "test_refusals_leave_the_outputs_alone",
                          "test_convert_whole.py::test_ragged_host_refusals_without_a_gpu"],
    "avc_row_mask": [G_ + "test_row_mask", G_ + "test_row_mask_full_lengths_write_nothing",
                     G_ + "test_refusals_leave_the_outputs_alone",
                     "test_convert_whole.py::test_ragged_host_refusals_without_a_gpu"],
    "avc_bilstm_ragged_fwd": [G_ + "test_bilstm_against_fp64", G_ + "test_bilstm_full_lengths_match_lstm_fwd",
                              G_ + "test_refusals_leave_the_outputs_alone",
                              "test_convert_whole.py::test_ragged_host_refusals_without_a_gpu"],
}


def declared_symbols_ragged():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_RAGGED).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_ragged_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    declared = declared_symbols_ragged()
    assert set(declared) == set(LEDGER_RAGGED) == set(_lib.exported_symbols_ragged())
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg())
    assert not set(declared) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "ragged.hip" in _lib.SOURCES
    cache = {}
    for sym, refs in LEDGER_RAGGED.items():
        for ref_ in refs:
            fname, func = ref_.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref_)


def test_ragged_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)
    ok, short, long_ = (ctypes.c_int * 2)(5, 8), (ctypes.c_int * 2)(5, 1), (ctypes.c_int * 2)(9, 8)

    def err():
        return Lb.avc_last_error().decode()

    def bn(y=p, lens=ok, ldev=p, C=80, ld=80, T=8, out=p, act=1, dtype=_lib.F32):
        return Lb.avc_bn_seg_ragged(y, dtype, ld, 2, T, C, lens, ldev, p, p, 1e-5, act, None, out, None, None, None, None)

    def mask(x=p, lens=ok, ldev=p, C=80, ld=80, T=8):
        return Lb.avc_row_mask(x, None, ld, 2, T, C, lens, ldev, None)

    def rnn(x=p, lens=ok, ldev=p, H=44, T=8, h=p, comp=_lib.F32):
        return Lb.avc_bilstm_ragged_fwd(x, p, lens, ldev, 2, T, H, h, None, comp, None)

    for fn, name in ((bn, "avc_bn_seg_ragged"), (mask, "avc_row_mask"), (rnn, "avc_bilstm_ragged_fwd")):
        assert fn(lens=short) != 0 and name + ": lens[1] = 1 outside 2..T = 8" in err()
        assert fn(lens=long_) != 0 and name + ": lens[0] = 9 outside 2..T = 8" in err()
        assert fn(lens=None) != 0 and "null pointer" in err()
        assert fn(ldev=None) != 0 and "null pointer" in err()
        assert fn(T=1) != 0
    assert bn(y=None) != 0 and "null pointer" in err()
    assert bn(out=None) != 0 and "neither out nor out_bf16" in err()
    assert bn(C=0) != 0 and "C = 0" in err()
    assert bn(ld=79) != 0 and "ld = 79" in err()
    assert bn(act=9) != 0 and "unknown act" in err()
    assert bn(dtype=_lib.BF16) != 0 and "fp32 values only" in err()
    assert mask(x=None) != 0 and "null pointer" in err()
    assert mask(C=0) != 0 and mask(ld=3) != 0
    assert rnn(x=None) != 0 and rnn(h=None) != 0 and "null pointer" in err()
    assert rnn(H=0) != 0 and rnn(H=65) != 0 and "H = 65" in err()
    assert rnn(comp=7) != 0 and "unknown compute" in err()
