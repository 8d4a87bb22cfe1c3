"""The MetaDV speaker classifier (factory/MetaDV.py) without a GPU: state_dict layout, the seeded
window draw, the refusals made before any launch, the golden fixture's self-consistency against the
plain-torch restatement of tests/metadv_torch.py (which also provides the bf16 emulation of the GPU
tests), the tuple-returning embedder in embed_utterances, and the ledger of the second ABI header
(include/autovc_hip_dv.h): every entry point bound, exported and named in direct tests."""
import ast
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

from . import metadv_torch as MT
from .conftest import GOLDEN, ROOT
from .helpers import rel_inf

HEADER_DV = os.path.join(ROOT, "include", "autovc_hip_dv.h")
FP32_BAR = 1e-3  # the project's fp32 parity bar (tests/test_gpu_metadv.py)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "metadv.npz"))


@functools.lru_cache(maxsize=None)
def ref_state():
    """The closed-form weights under the fixture's state_dict layout."""
    from autoformer_amd.detinit import det_state_dict

    g = golden()

    class _Shape:
        def __init__(self, s):
            self.shape = tuple(int(d) for d in s.split(",") if d)

    tmpl = {str(k): _Shape(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    return {k: torch.from_numpy(v) for k, v in det_state_dict(tmpl).items()}


def x200():
    from autoformer_amd.detinit import det_inputs

    return det_inputs(3, 200)[0]


def test_state_dict_layout_matches_reference():
    import factory.MetaDV as M

    g = golden()
    m = M.MetaDV(256)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert len(sd) == 26 and sum(p.numel() for p in m.parameters()) == 11688088
    blk = M.MetaBlock(10, dim_emb=16, emb=64, crop_len=32, patch_size=8, sample_count=2)
    assert blk.output.weight.shape == (10, 16) and blk.conv_1.conv.weight.shape == (64, 32, 3)
    assert blk.mlp[3].weight.shape == (88, 64, 3) and blk.dv.weight.shape == (16, 128)


def test_seeded_draw_reproduces_the_reference_crops():
    import factory.MetaDV as M

    g = golden()
    m = M.MetaDV(256)
    random.seed(7)
    assert m.draw_lefts(176) == [20, 9, 25, 41] == [int(v) for v in g["lefts176"]]
    assert m.draw_lefts(128) == [0, 0, 0, 0]
    # with lens: row by row, each row's four draws inside its own length, as it would be embedded alone
    random.seed(9)
    lens = [int(v) for v in g["lens200"]]
    assert m.draw_lefts(200, lens) == g["lefts200"].tolist()


def test_short_input_and_bad_windows_are_refused_before_any_launch():
    import factory.MetaDV as M

    m = M.MetaDV(256)
    with pytest.raises(ValueError):
        m.draw_lefts(127)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 127, 80))  # a host tensor: the length is refused first
    with torch.no_grad():
        with pytest.raises(ValueError):
            m(torch.zeros(2, 176, 80), [176, 127])
        with pytest.raises(ValueError):
            m(torch.zeros(2, 176, 80), lefts=[0, 0, 0, 49])
        with pytest.raises(ValueError):
            m(torch.zeros(2, 176, 80), [176, 150], lefts=[[0, 0], [0, 0], [0, 23], [0, 0]])
        with pytest.raises(ValueError):
            m(torch.zeros(2, 176, 80), lefts=[0, 0, 0])
    with pytest.raises(ValueError):
        m(torch.zeros(2, 176, 80), [176, 150])  # lens is an inference argument
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 176, 80))  # no CPU fallback


def test_fixture_is_self_consistent():
    """The restatement reproduces the fixture's outputs to 1e-5 and the step's gradient norms
    to 1e-4; windows shifted by one frame land more than 10x the fp32 bar away."""
    g = golden()
    sd = ref_state()
    x176 = torch.from_numpy(g["x176"])
    lefts = [int(v) for v in g["lefts176"]]
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = x176.clone().requires_grad_(True)
    pred, dvec = MT.forward(leaves, x, lefts)
    assert rel_inf(pred.detach().numpy(), g["pred176"]) < 1e-5
    assert rel_inf(dvec.detach().numpy(), g["dvec176"]) < 1e-5
    loss = MT.step_loss(pred, dvec, torch.from_numpy(g["e176"]), torch.from_numpy(g["step_labels"]))
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g["step_loss"]), rtol=1e-5)
    grads = {k: v.grad for k, v in leaves.items()}
    grads["dx"] = x.grad
    for n, gr in grads.items():
        ref_n = float(g["step_gnorm/" + n])
        assert abs(gr.norm().item() - ref_n) <= 1e-4 * ref_n + 1e-9, n
        head = g["step_ghead/" + n]
        assert np.abs(gr.reshape(-1)[:64].numpy() - head).max() <= 1e-4 * max(np.abs(head).max(), 1e-9) + 1e-9, n
    assert float(grads["metablock.mlp.3.weight"][:87].abs().max()) == 0.0  # one output channel is consumed
    with torch.no_grad():
        p128, d128 = MT.forward(sd, x176[:, :128], [0, 0, 0, 0])
        assert rel_inf(p128.numpy(), g["pred128"]) < 1e-5 and rel_inf(d128.numpy(), g["dvec128"]) < 1e-5
        lens = [int(v) for v in g["lens200"]]
        p200, d200 = MT.forward(sd, torch.from_numpy(x200()), g["lefts200"].tolist(), lens)
        assert rel_inf(p200.numpy(), g["pred200"]) < 1e-5 and rel_inf(d200.numpy(), g["dvec200"]) < 1e-5
        _, shifted = MT.forward(sd, x176, [v + 1 for v in lefts])
        assert rel_inf(shifted.numpy(), g["dvec176"]) > 10 * FP32_BAR


def test_bf16_emulation_drift_is_small_next_to_a_wrong_window():
    g = golden()
    sd = ref_state()
    x176 = torch.from_numpy(g["x176"])
    lefts = [int(v) for v in g["lefts176"]]
    d_emu = rel_inf(MT.emulate_bf16(sd, x176, lefts)[1].numpy(), g["dvec176"])
    print(f"bf16 emulation drift of d_vec from the fixture: {d_emu:.3e}")
    assert d_emu < 5e-2, d_emu  # the project's bf16 bar: the emulation itself sits inside it


class _TupleStub:
    """(x, lens[, lefts]) -> (predictions (B, 3), d_vec (B, 2)): d_vec = [first bin, first window start or -1]."""
    crop_len = 128

    def __init__(self):
        self.calls = []

    def __call__(self, x, lens, lefts=None):
        self.calls.append((tuple(x.shape), list(lens), lefts))
        d = [[float(x[b, 0, 0]), float(lefts[0][b]) if lefts is not None else -1.0] for b in range(x.shape[0])]
        return torch.zeros(x.shape[0], 3), torch.tensor(d)


def test_embed_utterances_takes_the_dvec_of_a_tuple_embedder():
    from autoformer_amd.embed import embed_utterances, speaker_dvector

    rng = np.random.RandomState(0)
    lengths = [200, 130, 230, 150]
    mels = [rng.rand(n, 80).astype(np.float32) + 0.5 for n in lengths]
    stub = _TupleStub()
    out = embed_utterances(stub, mels, len_crop=176, max_batch=3)
    assert out.shape == (4, 2) and [c[0][0] for c in stub.calls] == [3, 1]
    assert [out[i, 0] for i in range(4)] == [m[0, 0] for m in mels] and set(out[:, 1]) == {-1.0}
    # per-utterance window starts travel to the utterance's own row of its batch, crops-major
    lefts = [[i, 0, 0, 0] for i in range(4)]
    stub = _TupleStub()
    out = embed_utterances(stub, mels, len_crop=176, max_batch=3, lefts=lefts)
    assert list(out[:, 1]) == [0.0, 1.0, 2.0, 3.0]
    assert stub.calls[0][2] == [[1, 3, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]  # sorted by length: 130, 150/176, 200
    np.testing.assert_allclose(speaker_dvector(stub, mels, 176, 3, lefts), out.mean(axis=0))
    with pytest.raises(ValueError, match="crop_len"):
        embed_utterances(stub, mels, len_crop=64)
    with pytest.raises(ValueError):
        embed_utterances(stub, mels, len_crop=176, lefts=lefts[:2])


def test_embed_cli_knows_the_embedders():
    from autoformer_amd import embed

    args = embed._parser().parse_args(["--spmel", "x", "--embedder", "MetaDV", "--num_classes", "40", "--det_init"])
    assert args.embedder == "MetaDV" and args.num_classes == 40
    assert embed._parser().parse_args(["--spmel", "x"]).embedder == "LstmDV"
    with pytest.raises(SystemExit):
        embed.main(["--spmel", "x", "--embedder", "MetaDV", "--det_init", "--device", "cpu"])


# ----------------------------------------------------------------------- the second header's ledger
D_ = "test_gpu_metadv_kernels.py::"
LEDGER_DV = {
    "avc_crop_windows": [D_ + "test_crop_windows_equals_the_gather", D_ + "test_host_refusals_launch_nothing"],
    "avc_crop_windows_bwd": [D_ + "test_crop_windows_bwd_equals_the_scatter_sum",
                             D_ + "test_host_refusals_launch_nothing"],
    "avc_chan_mean": [D_ + "test_chan_mean_forward_and_backward"],
    "avc_chan_mean_bwd": [D_ + "test_chan_mean_forward_and_backward"],
    "avc_metadv_head": [D_ + "test_metadv_head_against_fp64", D_ + "test_host_refusals_launch_nothing"],
}


def declared_symbols_dv():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_DV).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_dv_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    declared = declared_symbols_dv()
    assert len(declared) == 5 and set(declared) == set(LEDGER_DV)
    assert set(declared) == set(_lib.exported_symbols_dv())
    assert not set(declared) & set(declared_symbols())          # no name shared with autovc_hip.h ...
    assert not set(declared) & set(_lib.exported_symbols())     # ... and the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31                   # added without an ABI bump
    cache = {}
    for sym, refs in LEDGER_DV.items():
        assert refs, sym
        for ref in refs:
            fname, func = ref.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref)


def test_dv_host_refusals_without_a_gpu():
    """Every argument check precedes the launch: bad arguments come back as errors on a box with no device."""
    from autoformer_amd import _lib

    L = _lib.lib()
    arr = (_lib.c_int * 2)(0, 5)
    p = ctypes.c_void_p(256)  # never dereferenced: each call below is refused first
    assert L.avc_crop_windows(None, 0, arr, p, None, 1, 20, 8, 16, 2, p, 0, None) == -1
    assert b"null" in L.avc_last_error()
    assert L.avc_crop_windows(p, 0, arr, p, None, 1, 20, 8, 16, 2, p, 0, None) == -1  # left 5 > 20 - 16
    assert b"left[1][0] = 5" in L.avc_last_error()
    assert L.avc_crop_windows(p, 0, arr, p, None, 1, 12, 8, 16, 2, p, 0, None) == -1  # W > T
    assert b"longer than T" in L.avc_last_error()
    assert L.avc_crop_windows(p, 1, arr, p, None, 1, 32, 8, 16, 2, p, 0, None) == -1  # bf16 -> fp32
    assert L.avc_crop_windows_bwd(p, None, arr, p, None, None, 1, 20, 8, 16, 2, p, None) == -1
    assert L.avc_crop_windows_bwd(p, None, arr, p, arr, None, 1, 32, 8, 16, 2, p, None) == -1  # last without last_dev
    assert L.avc_chan_mean(None, 2, 1, 8, 4, p, None) == -1
    assert L.avc_chan_mean_bwd(p, 0, 1, 8, 4, p, None) == -1
    assert L.avc_metadv_head(p, p, 2, 4, p, None, p, None, 1, 6, 4, 3, p, p, None) == -1  # E % 4
    assert L.avc_metadv_head(p, None, 2, 4, p, None, p, None, 1, 8, 4, 3, p, p, None) == -1
