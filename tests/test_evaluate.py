"""The Evaluator and the conversion grid without a GPU (autoformer_amd/evaluate.py, reference
util/evaluate.py second half): the ledger of the fifth ABI header (include/autovc_hip_eval.h), the host
refusals of avc_bn_seg_apply on a machine with no device, the cosine summaries on a hand-made array,
build_metadata's filter and order, and the grid's planning step -- the crop draws in the reference's
order and the encoder rows it deduplicates."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

from .conftest import ROOT

HEADER_EVAL = os.path.join(ROOT, "include", "autovc_hip_eval.h")

# ----------------------------------------------------------------------- the fifth header's ledger
G_ = "test_gpu_bn_seg.py::"
LEDGER_EVAL = {
    "avc_bn_seg_apply": [G_ + "test_against_fp64_batch_norm_per_segment", G_ + "test_outputs_and_residual",
                         G_ + "test_large_mean_small_spread", G_ + "test_segments_are_independent",
                         G_ + "test_nothing_outside_the_tile_is_written",
                         "test_evaluate.py::test_bn_seg_host_refusals_without_a_gpu"],
}


def declared_symbols_eval():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_EVAL).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_eval_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols
    from .test_audio import declared_symbols_audio
    from .test_metadv import declared_symbols_dv
    from .test_resample import declared_symbols_resample

    declared = declared_symbols_eval()
    assert set(declared) == set(LEDGER_EVAL) == set(_lib.exported_symbols_eval())
    others = [(_lib.exported_symbols(), declared_symbols()), (_lib.exported_symbols_dv(), declared_symbols_dv()),
              (_lib.exported_symbols_audio(), declared_symbols_audio()),
              (_lib.exported_symbols_resample(), declared_symbols_resample())]
    for table, header in others:
        assert not set(declared) & set(table) and not set(declared) & set(header)
        assert set(table) == set(header)                              # the four earlier tables are as they were
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31   # added without an ABI bump
    assert "bn_seg.hip" in _lib.SOURCES
    hdr = open(HEADER_EVAL).read()
    assert int(re.search(r"#define AVC_BN_SEG_LDS_ROWS (\d+)", hdr).group(1)) == _lib.BN_SEG_LDS_ROWS
    # the resident tile + the reduction scratch fit the 64 KiB a workgroup may take
    assert (_lib.BN_SEG_LDS_ROWS * 64 + 4 * 64) * 4 <= 65536
    cache = {}
    for sym, refs in LEDGER_EVAL.items():
        assert refs, sym
        for ref_ in refs:
            fname, func = ref_.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref_)


# ----------------------------------------------------------------------- host refusals, no device
def refusal_cases():
    """(what is wrong, keyword overrides of a valid call, a piece of the message)."""
    return [
        ("T = 1", {"T": 1}, b"T = 1"),
        ("T = 0", {"T": 0}, b"T = 0"),
        ("T < 0", {"T": -4}, b"T = -4"),
        ("C = 0", {"C": 0}, b"bad shape"),
        ("B = 0", {"B": 0}, b"bad shape"),
        ("B < 0", {"B": -1}, b"bad shape"),
        ("ld < C", {"ld": 79}, b"ld = 79 is below C = 80"),
        ("null y", {"y": None}, b"null"),
        ("null gamma", {"gamma": None}, b"null"),
        ("null beta", {"beta": None}, b"null"),
        ("no output", {"out": None, "out_bf16": None}, b"neither out nor out_bf16"),
        ("unknown act", {"act": 6}, b"unknown act 6"),
        ("negative act", {"act": -1}, b"unknown act -1"),
        ("bf16 y", {"y_dtype": 1}, b"y_dtype = 1"),
        ("unknown dtype", {"y_dtype": 7}, b"y_dtype = 7"),
        ("negative eps", {"eps": -1e-5}, b"eps"),
        ("nan eps", {"eps": float("nan")}, b"eps"),
    ]


def call_bn_seg(Lb, **over):
    p = ctypes.c_void_p(256)  # never dereferenced: every check precedes the launch
    a = dict(y=p, y_dtype=0, ld=80, B=3, T=7, C=80, gamma=p, beta=p, eps=1e-5, act=1, residual=None, out=p,
             out_bf16=None, mean=None, rstd=None)
    a.update(over)
    return Lb.avc_bn_seg_apply(a["y"], a["y_dtype"], a["ld"], a["B"], a["T"], a["C"], a["gamma"], a["beta"], a["eps"],
                               a["act"], a["residual"], a["out"], a["out_bf16"], a["mean"], a["rstd"], None)


def test_bn_seg_host_refusals_without_a_gpu():
    from autoformer_amd import _lib

    Lb = _lib.lib()
    for what, over, msg in refusal_cases():
        assert call_bn_seg(Lb, **over) == -1, what
        assert msg in Lb.avc_last_error(), (what, Lb.avc_last_error())


def test_per_utterance_bn_refuses_gradients():
    import torch

    from autoformer_amd import layers as Lyr

    with pytest.raises(RuntimeError, match="forward-only"):
        with Lyr.per_utterance_bn():
            pass
    assert not Lyr._PER_UTT["on"]
    with torch.no_grad():
        with Lyr.per_utterance_bn():
            assert Lyr._PER_UTT["on"]
            with Lyr.per_utterance_bn():
                pass
            assert Lyr._PER_UTT["on"]
    assert not Lyr._PER_UTT["on"]


# ----------------------------------------------------------------------- the cosine summaries
def test_cos_summaries_by_hand():
    """cos[source][target][judged speaker], N = 3, values chosen so every sum is exact in binary."""
    from autoformer_amd.evaluate import Evaluator, get_cos_rc, get_cos_trans

    c = np.array([[[1.0, 0.5, 0.25], [0.0, 0.75, 0.5], [0.25, 0.0, 0.5]],
                  [[0.5, 0.25, 0.0], [0.125, 0.875, 0.25], [0.5, 0.25, 1.0]],
                  [[0.75, 0.0, 0.125], [0.25, 0.5, 0.0], [0.0, 0.375, 0.625]]])
    # reconstruction i -> i against i: 1.0, 0.875, 0.625; against the others: (0.5 + 0.25)/2,
    # (0.125 + 0.25)/2, (0.0 + 0.375)/2
    rc, rc_other = get_cos_rc(c)
    assert rc == (1.0 + 0.875 + 0.625) / 3
    assert rc_other == (0.375 + 0.1875 + 0.1875) / 3
    # source 0: targets 1, 2 against themselves 0.75, 0.5 -> 0.625; everything off the diagonal of c[0]:
    # 0.5 + 0.25 + 0.0 + 0.5 + 0.25 + 0.0 = 1.5 -> / 6 = 0.25
    # source 1: targets 0, 2: 0.5, 1.0 -> 0.75; off-diagonal 0.25 + 0 + 0.125 + 0.25 + 0.5 + 0.25 = 1.375 -> / 6
    # source 2: targets 0, 1: 0.75, 0.5 -> 0.625; off-diagonal 0 + 0.125 + 0.25 + 0 + 0 + 0.375 = 0.75 -> 0.125
    tr, tr_other = get_cos_trans(c)
    assert tr == pytest.approx((0.625 + 0.75 + 0.625) / 3, abs=1e-15)
    assert tr_other == pytest.approx((0.25 + 1.375 / 6 + 0.125) / 3, abs=1e-15)
    E = Evaluator.__new__(Evaluator)  # the methods are the same functions
    assert E.get_cos_rc(c) == (rc, rc_other) and E.get_cos_trans(c) == (tr, tr_other)


# ----------------------------------------------------------------------- build_metadata
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(root=".", num_speaker=2, batch_size=2, max_uttr_idx=6, erroment_num=2, len_crop=8,
                             device="cpu", all_speaker=[], embedder=None, metadata=[])
        self.__dict__.update(kw)


def test_build_metadata_filters_and_sorts():
    from autoformer_amd.evaluate import Evaluator

    dv = np.zeros(4, np.float32)
    meta = [["p300", dv, "p300/a.npy"], ["p225", dv, "p225/a.npy"], ["p999", dv, "p999/a.npy"],
            [226, dv, "226/a.npy"], ["p250", dv, "p250/a.npy"]]
    E = Evaluator(_Cfg(all_speaker=["p300", "p225", "226", "p001"], metadata=meta))
    assert [d[0] for d in E.metadata] == [226, "p225", "p300"]        # str(name) in all_speaker; sorted by name
    assert E.metadata[1][2] == "p225/a.npy"
    assert list(E.remain_idx) == [2, 3, 4, 5] and E.enrroment_idx == [] and E.vocoder is None
    assert not hasattr(E, "all_dv")                                    # no judge: no enrolment draws
    for f in ("root", "num_speaker", "batch_size", "max_uttr_idx", "erroment_num", "len_crop", "device", "all_speaker",
              "embedder", "metadata"):
        assert hasattr(E, f)
    for m in ("build_metadata", "crop_mel", "get_mel", "get_trans_mel", "get_wavs", "get_dv", "generate_real_dv",
              "get_real_data_cos", "get_cos_rc", "get_cos_trans", "generate_result"):
        assert callable(getattr(E, m))
    with pytest.raises(RuntimeError, match="vocoder"):
        E.get_wavs(None)
    with pytest.raises(RuntimeError, match="judge"):
        E.generate_result([None])


def test_enrolment_draws_follow_python_random(tmp_path):
    """generate_real_dv: erroment_num random.choice draws from remain_idx, each removed once drawn; the
    judge then embeds every speaker's enrolment utterances (a stub judge: the mean frame)."""
    import random

    import torch

    from autoformer_amd.evaluate import Evaluator

    rng = np.random.RandomState(0)
    meta = []
    for spk in ("a", "b"):
        os.makedirs(tmp_path / spk)
        row = [spk, np.zeros(3, np.float32)]
        for u in range(5):
            np.save(tmp_path / spk / f"{u}.npy", rng.rand(6 + u, 3).astype(np.float32))
            row.append(f"{spk}/{u}.npy")
        meta.append(row)

    def judge(x, lens):
        return torch.stack([x[b, :n].mean(dim=0) for b, n in enumerate(lens)])

    random.seed(11)
    np.random.seed(4)
    E = Evaluator(_Cfg(root=str(tmp_path), all_speaker=["a", "b"], metadata=meta, max_uttr_idx=7, erroment_num=3,
                       len_crop=8, embedder=judge))
    random.seed(11)
    remain = list(range(2, 7))
    picks = []
    for _ in range(3):
        picks.append(random.choice(remain))
        remain.remove(picks[-1])
    assert [int(i) for i in E.enrroment_idx] == picks and [int(i) for i in E.remain_idx] == remain
    # speaker a's d-vector by hand: enrolment mels, cropped / padded to 8 frames under the same numpy seed
    from autoformer_amd.convert import crop_mel

    np.random.seed(4)
    want = np.zeros(3, np.float32)
    for i in picks:
        want += crop_mel(np.load(tmp_path / meta[0][i]), 8)[0].mean(axis=0)
    got = E.all_dv[0].numpy()
    assert got.shape == (1, 3)
    np.testing.assert_allclose(got[0], want / 3, rtol=1e-6)
    cos, std = E.get_real_data_cos()
    assert cos.shape == (2, 2) and std.shape == (2, 2)
    assert (cos >= 0).all() and (cos <= 1 + 1e-6).all() and (std >= 0).all()


# ----------------------------------------------------------------------- the plan
def test_plan_draw_order_replays_crop_mel():
    """Per pair: the source crop, then the target crop -- the draws get_trans_mel makes (evaluate.py:66-67),
    replayed here with crop_mel itself under the same numpy seed; with two models, model after model
    within each pair (evaluate.py:196-199)."""
    from autoformer_amd.convert import crop_mel
    from autoformer_amd.evaluate import _cut, all_pairs, plan_grid

    rng = np.random.RandomState(1)
    mels = [rng.rand(T, 4).astype(np.float32) for T in (30, 16, 11, 45)]   # longer, exact, shorter, longer
    lens = [m.shape[0] for m in mels]
    for copies in (1, 2):
        np.random.seed(77)
        plans = plan_grid(lens, None, 16, np.random, tgt_lens=lens, copies=copies)
        assert len(plans) == copies
        np.random.seed(77)
        for i, (s, t) in enumerate(all_pairs(4)):
            for p in plans:
                assert p.pairs[i] == (s, t)
                src, pad_s = crop_mel(mels[s], 16)
                tgt, pad_t = crop_mel(mels[t], 16)
                np.testing.assert_array_equal(_cut(mels[s], p.src_crop[i][0], 16), src)
                np.testing.assert_array_equal(_cut(mels[t], p.tgt_crop[i][0], 16), tgt)
                assert (p.src_crop[i][1], p.tgt_crop[i][1], p.pads[i]) == (pad_s, pad_t, pad_s)
    # without target mels only the sources draw; a seeded generator of the caller's is used as given
    a = plan_grid(lens, [(0, 1), (3, 0), (0, 2)], 16, np.random.RandomState(5))[0]
    r = np.random.RandomState(5)
    assert [c[0] for c in a.src_crop] == [r.randint(0, 14), r.randint(0, 29), r.randint(0, 14)]
    assert a.tgt_crop is None and a.pairs == [(0, 1), (3, 0), (0, 2)]


def test_plan_deduplicates_encoder_rows():
    from autoformer_amd.evaluate import plan_grid

    p = plan_grid([10, 12, 16], None, 16, np.random.RandomState(0))[0]     # three sources, none longer
    assert len(p.enc_rows) == 3 and len(p.pairs) == 9
    assert p.enc_rows == [(0, 0), (1, 0), (2, 0)]
    assert p.pair_enc == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert p.pads == [6, 6, 6, 4, 4, 4, 0, 0, 0]
    # a longer source draws an offset per pair: pairs share an encoder row only where the offsets agree
    q = plan_grid([10, 400, 16], None, 16, np.random.RandomState(0))[0]
    lefts = [q.src_crop[i][0] for i in (3, 4, 5)]
    assert len(set(lefts)) == 3                                             # (this seed: three distinct offsets)
    assert q.enc_rows == [(0, 0)] + [(1, l) for l in lefts] + [(2, 0)]
    assert q.pair_enc == [0, 0, 0, 1, 2, 3, 4, 4, 4]
    # ... and do share it where they agree (T - len_crop = 1: randint(0, 1) is always 0)
    s = plan_grid([17, 17], None, 16, np.random.RandomState(0))[0]
    assert s.enc_rows == [(0, 0), (1, 0)] and s.pair_enc == [0, 0, 1, 1]


def test_convert_grid_argument_checks():
    from autoformer_amd.evaluate import batched_family, convert_grid

    mels = [np.zeros((8, 80), np.float32)] * 2
    with pytest.raises(ValueError, match="max_batch"):
        convert_grid(None, mels, np.zeros((2, 4), np.float32), max_batch=0)
    with pytest.raises(ValueError, match="emb must be"):
        convert_grid(None, mels, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="target mels"):
        convert_grid(None, mels, np.zeros((2, 4), np.float32), isAdjust=True)
    from autoformer_amd.factory.AutoVC import AutoVC
    from autoformer_amd.factory.MetaConv import MetaConv

    m = AutoVC(4, 8, 16, 4)
    assert batched_family(m) and not batched_family(m, isAdain=True) and not batched_family(m, isAdjust=True)
    assert not batched_family(MetaConv(44, 256, 512, 16))
