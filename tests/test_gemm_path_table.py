"""CPU checks of the avc_gemm_last_path encoding and of the table tests/test_gpu_gemm_paths.py runs:
the Python constants mirror the header's enum, and every kernel family and variant the witness can
name is the expected value of at least one row -- a new variant fails here until it has a case."""
import os
import re

from .conftest import ROOT
from .gemm_path_cases import CASES, DTYPES, LAYOUTS, PATH_FAMILY_VARIANTS, gemm_path


def test_python_constants_mirror_the_header_enum():
    from autoformer_amd import _lib as L

    src = open(os.path.join(ROOT, "include", "autovc_hip.h")).read()
    enum = {k: int(v, 0) for k, v in re.findall(r"\bAVC_(PATH_[A-Z_0-9]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", src)}
    mine = {k: v for k, v in vars(L).items() if k.startswith("PATH_") and isinstance(v, int)}
    assert enum == mine and len(enum) == 11, (enum, mine)
    assert set(PATH_FAMILY_VARIANTS) == {v for k, v in mine.items()
                                           if k not in ("PATH_VARIANT_SHIFT", "PATH_SPLITK_WS", "PATH_POST_PASS",
                                                        "PATH_WINDOW", "PATH_BNB")}


def test_every_family_and_variant_is_some_rows_expected_value():
    from autoformer_amd import _lib as L

    fam_var = {(c.expect & 0xF, (c.expect >> L.PATH_VARIANT_SHIFT) & 0xF) for c in CASES}
    want = {(f, v) for f, vs in PATH_FAMILY_VARIANTS.items() for v in vs}
    assert fam_var == want, (sorted(want - fam_var), sorted(fam_var - want))
    exp = {c.expect for c in CASES}
    # the flag bits on the families that can set them
    for f, v in ((L.PATH_NT, 1), (L.PATH_NT, 2), (L.PATH_CONV, 0), (L.PATH_FAST, 1)):
        assert gemm_path(f, v, L.PATH_BNB) in exp, (f, v, "BNB instance")
    assert gemm_path(L.PATH_RING, 2, L.PATH_BNB) in exp  # the halo conv ring's own BN-backward epilogue
    # the GELU / col_sum pass after a kernel without that epilogue -- and the ring without it
    for f, v in ((L.PATH_GENERIC, 0), (L.PATH_FAST, 1), (L.PATH_NT, 1)):
        assert gemm_path(f, v, L.PATH_POST_PASS) in exp, (f, v, "pass after")
    assert any(c.col_sum and c.expect == gemm_path(L.PATH_RING, 1) for c in CASES)
    # guard columns on every row whose descriptor allows ldc != N
    assert all(c.ldc_pad > 0 or c.bnb is not None for c in CASES)
    assert gemm_path(L.PATH_NT, 1, L.PATH_WINDOW) in exp and gemm_path(L.PATH_NT, 1, L.PATH_WINDOW | L.PATH_BNB) in exp
    # each tt form under each split-K mode: single pass, workspace reduction, atomics
    tags = {t for c in CASES for t in c.tags}
    for v in PATH_FAMILY_VARIANTS[L.PATH_TT]:
        for mode in ("single", "ws", "atomics"):
            assert f"tt{v}-{mode}" in tags, (v, mode)
    for c in CASES:
        for t in c.tags:
            if t.startswith("tt"):
                v, mode = int(t[2]), t[4:]
                assert c.expect == gemm_path(L.PATH_TT, v, L.PATH_SPLITK_WS if mode == "ws" else 0), c.name
                assert (c.split > 1) == (mode != "single"), c.name
    # the fast kernel: 2 widths x 4 layouts x 4 operand-dtype pairs
    for w, var in ((64, 1), (128, 2)):
        inst = {(c.a["ks"], c.b["ks"], c.a["dt"], c.b["dt"]) for c in CASES
                if f"fast{w}-instance" in c.tags and c.expect == gemm_path(L.PATH_FAST, var)}
        assert inst == {(a, b, x, y) for _, a, b in LAYOUTS for x, y in DTYPES}, w
