"""The opt-in batched grid of the Meta and AdaIN families without a GPU (autoformer_amd/evaluate.py):
grid_family's table, batched_family as it was, the CLI flag, convert_grid's check of batch_families, and
the ledger and host refusals of the sixth ABI header (include/autovc_hip_seg.h)."""
import ast
import ctypes
import importlib
import os
import re

import pytest

from .conftest import ROOT

HEADER_SEG = os.path.join(ROOT, "include", "autovc_hip_seg.h")

PLAIN = ["AutoVC", "MetaConv", "MetaPool"]
ADAIN = ["AutoVC2", "MetaConv2", "MetaPool2"]
ADJUST = ["AutoVC_Adjust", "MetaConv_Adjust", "MetaPool_Adjust"]


def _bare(name):
    """An instance of the factory class without running its constructor: the family is decided by type."""
    cls = getattr(importlib.import_module(f"autoformer_amd.factory.{name}"), name)
    return cls.__new__(cls)


def _subclass():
    from autoformer_amd.factory.AutoVC import AutoVC

    class Mine(AutoVC):
        pass

    return Mine.__new__(Mine)


# (model, isAdjust, isAdain) -> grid_family
TABLE = ([(n, False, False, {"AutoVC": "autovc"}.get(n, "meta")) for n in PLAIN]
         + [(n, False, True, "adain") for n in ADAIN]
         + [(n, False, False, None) for n in ADAIN]           # an AdaIN model called without isAdain
         + [(n, True, False, None) for n in ADJUST]
         + [(n, False, False, None) for n in ADJUST]
         + [(n, True, False, None) for n in PLAIN]            # isAdjust on any model
         + [(n, False, True, None) for n in PLAIN]            # isAdain on a model without AdaIN
         + [(n, True, True, None) for n in ADAIN])


@pytest.mark.parametrize("name,isAdjust,isAdain,want", TABLE)
def test_grid_family_table(name, isAdjust, isAdain, want):
    from autoformer_amd.evaluate import grid_family

    assert grid_family(_bare(name), isAdjust, isAdain) == want


def test_grid_family_is_by_exact_type():
    import torch

    from autoformer_amd.evaluate import grid_family

    assert grid_family(_subclass()) is None                    # the tenth class: a subclass is not AutoVC
    assert grid_family(torch.nn.Linear(2, 2)) is None
    assert grid_family(_bare("AutoVC")) == "autovc"            # the defaults: no Adjust, no AdaIN


def test_batched_family_is_unchanged():
    from autoformer_amd.evaluate import batched_family

    assert batched_family(_bare("AutoVC"))
    assert not batched_family(_bare("AutoVC"), True, False) and not batched_family(_bare("AutoVC"), False, True)
    for name in PLAIN[1:] + ADAIN + ADJUST:
        for adj in (False, True):
            for ada in (False, True):
                assert not batched_family(_bare(name), adj, ada), (name, adj, ada)
    assert not batched_family(_subclass())


def test_cli_flag_parses():
    from autoformer_amd.evaluate import _parser

    p = _parser()
    assert p.parse_args(["--root", "r"]).batch_families is False
    assert p.parse_args(["--root", "r", "--batch_families"]).batch_families is True
    assert p.parse_args(["--root", "r", "--model", "MetaConv2", "--batch_families"]).model == "MetaConv2"


@pytest.mark.parametrize("bad", ["yes", 1, None, 0.0])
def test_convert_grid_checks_batch_families_first(bad):
    """Before the model, the embeddings or a device are looked at: every other argument here is unusable."""
    from autoformer_amd.evaluate import convert_grid

    with pytest.raises(TypeError, match="batch_families must be a bool"):
        convert_grid(object(), None, None, batch_families=bad)


def test_generate_result_takes_the_flag():
    import inspect

    from autoformer_amd.evaluate import Evaluator, convert_grid

    for fn in (Evaluator.generate_result, convert_grid):
        assert inspect.signature(fn).parameters["batch_families"].default is False


# ----------------------------------------------------------------------- the sixth header's ledger
G_ = "test_gpu_seg_moments.py::"
LEDGER_SEG = {
    "avc_seg_moments": [G_ + "test_against_fp64_per_segment", G_ + "test_one_segment_matches_the_whole_tensor_kernels",
                        G_ + "test_segments_are_independent", G_ + "test_nothing_outside_the_outputs_is_written",
                        "test_evaluate_families.py::test_seg_host_refusals_without_a_gpu"],
    "avc_adain_seg": [G_ + "test_against_fp64_per_segment", G_ + "test_misaligned_base_takes_the_scalar_path",
                      G_ + "test_large_mean_small_spread", G_ + "test_segments_are_independent",
                      G_ + "test_nothing_outside_the_outputs_is_written",
                      "test_evaluate_families.py::test_seg_host_refusals_without_a_gpu"],
}


def declared_symbols_seg():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_SEG).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_seg_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols
    from .test_evaluate import declared_symbols_eval

    declared = declared_symbols_seg()
    assert set(declared) == set(LEDGER_SEG) == set(_lib.exported_symbols_seg())
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval())
    assert not set(declared) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    assert set(_lib.exported_symbols_eval()) == set(declared_symbols_eval())   # and the fifth
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "seg_moments.hip" in _lib.SOURCES
    hdr = open(HEADER_SEG).read()
    cap = int(re.search(r"#define AVC_SEG_MOMENTS_LDS_FLOATS (\d+)", hdr).group(1))
    assert cap == _lib.SEG_MOMENTS_LDS_FLOATS and cap % 4 == 0
    assert cap * 4 + 64 <= 65536 and cap >= 176 * 80       # with the reduction slots within 64 KiB; the conversion shape fits
    cache = {}
    for sym, refs in LEDGER_SEG.items():
        for ref_ in refs:
            fname, func = ref_.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref_)


def test_seg_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)
    for args, msg in (((None, 2, 80, p, None), b"null"), ((p, 2, 80, None, None), b"null"),
                      ((p, 0, 80, p, None), b"bad shape B = 0"), ((p, -1, 80, p, None), b"bad shape"),
                      ((p, 2, 0, p, None), b"n = 0"), ((p, 2, -5, p, None), b"n = -5")):
        assert Lb.avc_seg_moments(*args) == -1, args
        assert msg in Lb.avc_last_error(), (args, Lb.avc_last_error())
    for args, msg in (((None, 2, 80, p, p, p, None), b"null"), ((p, 2, 80, None, p, p, None), b"null"),
                      ((p, 2, 80, p, None, p, None), b"null"), ((p, 2, 80, p, p, None, None), b"null"),
                      ((p, 0, 80, p, p, p, None), b"bad shape B = 0"), ((p, 2, 0, p, p, p, None), b"n = 0")):
        assert Lb.avc_adain_seg(*args) == -1, args
        assert msg in Lb.avc_last_error(), (args, Lb.avc_last_error())
