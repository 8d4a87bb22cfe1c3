"""Training the classifier, the host side (no GPU): the ledger of the tenth ABI header
(include/autovc_hip_xent.h) and its refusals (every check precedes the launch), kernels.Labels, the utterance
sampler on a generated mel tree, and the trainer's command line and resume checks."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .test_ge2e import _tree

HEADER_XENT = os.path.join(ROOT, "include", "autovc_hip_xent.h")


def declared_symbols_xent():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_XENT).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


# ----------------------------------------------------------------------- the tenth header
def test_xent_header_symbols():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    declared = declared_symbols_xent()
    assert declared == ["avc_xent", "avc_xent_ws"]
    assert set(declared) == set(_lib.exported_symbols_xent())
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg()
               + _lib.exported_symbols_ragged() + _lib.exported_symbols_vocoder() + _lib.exported_symbols_ge2e())
    assert not set(declared) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]                     # every declared symbol is built
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "xent.hip" in _lib.SOURCES
    src = open(HEADER_XENT).read()
    lim = {k: int(v) for k, v in re.findall(r"#define AVC_XENT_MAX_(\w+) (\d+)", src)}
    assert lim == {"B": _lib.XENT_MAX_B, "C": _lib.XENT_MAX_C}
    assert lim["C"] >= 16384 and lim["B"] >= 64


def test_xent_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)

    def err():
        return Lb.avc_last_error().decode()

    def call(logits=p, ld=8, B=4, C=8, labels=p, smooth=0.0, L=p, d=q, ldd=8, correct=p, ws=p):
        return Lb.avc_xent(logits, ld, B, C, labels, smooth, L, d, ldd, correct, ws, None)

    for name in ("logits", "labels", "L", "ws"):
        assert call(**{name: None}) == -1 and "avc_xent: null pointer" in err() and name in err(), name
    assert call(B=0) == -1 and "avc_xent: bad shape B = 0" in err()
    assert call(C=0, ld=0, ldd=0) == -1 and "C = 0" in err()
    assert call(ld=7) == -1 and "ld = 7 is below C = 8" in err()
    assert call(ldd=7) == -1 and "ldd = 7 is below C = 8" in err()
    assert call(smooth=-0.01) == -1 and "smooth" in err()
    assert call(smooth=1.0) == -1 and "smooth" in err()
    assert call(smooth=float("nan")) == -1 and "smooth" in err()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and "ws must be 16-byte aligned" in err()
    assert call(B=_lib.XENT_MAX_B + 1) == -1 and "past the limits" in err() and "B" in err()
    big = _lib.XENT_MAX_C + 1
    assert call(C=big, ld=big, ldd=big) == -1 and "past the limits" in err() and "C" in err()
    assert call(d=p) == -1 and "dlogits must not alias logits" in err()
    assert call(d=ctypes.c_void_p(4096 + 64)) == -1 and "must not alias" in err()     # overlapping, not equal
    # the size query: 0 for what the call refuses, positive otherwise
    for B, C in ((0, 8), (8, 0), (-1, 8), (_lib.XENT_MAX_B + 1, 8), (8, big)):
        assert Lb.avc_xent_ws(B, C) == 0, (B, C)
    for B, C in ((1, 1), (3, 5), (64, 256), (2, 16384), (_lib.XENT_MAX_B, _lib.XENT_MAX_C)):
        n = Lb.avc_xent_ws(B, C)
        assert n >= 8 * B and n % 16 == 0, (B, C, n)


def test_labels_are_checked_on_the_host():
    """Labels refuses before it touches the device: `device` here names one that need not exist."""
    import torch

    from autoformer_amd import kernels as K

    for bad in ([0, -1, 2], [0, 5, 2], np.array([5]), torch.tensor([1, -1])):
        with pytest.raises(ValueError, match="every label must lie in 0..C - 1 = 4"):
            K.Labels(bad, 5, "cuda:0")
    for bad in ([0.0, 1.0], np.array([0.0, 1.0]), torch.tensor([0.0, 1.0]), np.array([True, False]),
                torch.tensor([True]), [True, 1], ["1"]):
        with pytest.raises(TypeError, match="integer labels"):
            K.Labels(bad, 5, "cuda:0")
    with pytest.raises(ValueError):
        K.Labels([], 5, "cuda:0")
    for good in ([0, 4, 2], np.array([0, 4, 2], dtype=np.int64), torch.tensor([0, 4, 2]), np.array([0, 4, 2], np.uint8)):
        lab = K.Labels(good, 5, "cpu")
        assert lab.B == 3 and lab.C == 5 and lab.vals == (0, 4, 2)
        assert lab.dev.dtype == torch.int32 and lab.dev.tolist() == [0, 4, 2]


def test_wrappers_need_a_device():
    import torch

    from autoformer_amd import kernels as K
    from autoformer_amd.xent import SoftmaxXent, softmax_xent

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        softmax_xent(torch.randn(3, 5), K.Labels([0, 1, 2], 5, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.xent(torch.randn(3, 5), K.Labels([0, 1, 2], 5, "cpu"))
    with pytest.raises(ValueError):
        SoftmaxXent(1.0)
    assert SoftmaxXent(0.1).smooth == 0.1 and SoftmaxXent().correct is None and not list(SoftmaxXent().parameters())


# ----------------------------------------------------------------------- UtteranceBatches
@pytest.fixture(scope="module")
def mel_tree(tmp_path_factory):
    spk = {f"s{k}": [40 + 3 * k + u for u in range(7)] for k in range(5)}
    spk["mixed"] = [50, 20, 50, 31, 50, 50]       # two utterances below T = 32; index 2 and 5 are validation
    return _tree(str(tmp_path_factory.mktemp("spmel")), spk)


def _ub(root, B=6, T=32, val_every=3, seed=0):
    from autoformer_amd.train_classifier import UtteranceBatches

    return UtteranceBatches(root, B, T, val_every=val_every, seed=seed, crop_len=24, sample_count=4)


def test_utterance_batches(mel_tree, capsys):
    ub = _ub(mel_tree, seed=5)
    out = capsys.readouterr().out
    assert "6 speakers, 27 training and 12 validation utterances, 2 left out (shorter than 32 frames)" in out
    assert ub.speakers == sorted(os.listdir(mel_tree)) == ["mixed"] + [f"s{k}" for k in range(5)]   # the class order
    train, val = {f for _, f in ub.train}, {f for _, f in ub.val}
    assert not train & val                                                       # disjoint
    usable = {os.path.join(mel_tree, s, f) for s in os.listdir(mel_tree) for f in os.listdir(os.path.join(mel_tree, s))
              if np.load(os.path.join(mel_tree, s, f)).shape[0] >= 32}
    assert train | val == usable and len(usable) == 39                           # together: the usable utterances
    for label, f in ub.train + ub.val:
        assert ub.speakers[label] == os.path.basename(os.path.dirname(f))
    for spk in ub.speakers:                                                      # by position in the sorted list
        files = sorted(os.listdir(os.path.join(mel_tree, spk)))
        for i, f in enumerate(files):
            if os.path.join(mel_tree, spk, f) in usable:
                assert (os.path.join(mel_tree, spk, f) in val) == (i % 3 == 2), (spk, f)
    seen = set()
    for _ in range(8):
        x, labels, lefts = next(ub)
        assert x.dtype == np.float32 and x.shape == (6, 32, 80)
        assert labels.dtype == np.int64 and labels.shape == (6,) and 0 <= labels.min() and labels.max() < 6
        assert len(lefts) == 4 and all(isinstance(v, int) and 0 <= v <= 32 - 24 for v in lefts)
        assert len(ub.last) == 6
        for r, (s, path, off) in enumerate(ub.last):
            src = np.load(path)
            assert ub.speakers[labels[r]] == s == os.path.basename(os.path.dirname(path))
            assert path in train                                                  # never a validation utterance
            assert 0 <= off and off + 32 <= src.shape[0]
            np.testing.assert_array_equal(x[r], src[off:off + 32])
        seen |= set(labels.tolist())
    assert len(seen) > 3                                                         # the speakers are drawn


def test_utterance_batches_reproducible_and_resumable(mel_tree):
    a, b, c = _ub(mel_tree, seed=1), _ub(mel_tree, seed=1), _ub(mel_tree, seed=2)

    def same(p, q):
        return np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2]

    ba = [next(a) for _ in range(3)]
    assert all(same(p, q) for p, q in zip(ba, [next(b) for _ in range(3)]))      # same seed, same sequence
    assert not all(same(p, q) for p, q in zip(ba, [next(c) for _ in range(3)]))
    st = a.state()
    nxt = [next(a) for _ in range(3)]
    c.set_state(st)
    assert all(same(p, q) for p, q in zip(nxt, [next(c) for _ in range(3)]))     # set_state(state()) continues exactly
    a.set_state(st)
    assert same(next(a), nxt[0])


def test_utterance_batches_leave_the_global_states_alone(mel_tree):
    np.random.seed(123)
    random.seed(123)
    before, before_py = np.random.get_state(), random.getstate()
    ub = _ub(mel_tree)
    next(ub), next(ub)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert random.getstate() == before_py


def test_utterance_batches_errors(mel_tree, tmp_path):
    from autoformer_amd.train_classifier import UtteranceBatches

    with pytest.raises(ValueError, match="speaker mixed has no training utterance of at least 51 frames"):
        UtteranceBatches(mel_tree, 4, 51, val_every=3, crop_len=24)
    with pytest.raises(ValueError, match="shorter than crop_len"):
        UtteranceBatches(mel_tree, 4, 23, val_every=3, crop_len=24)
    with pytest.raises(ValueError, match="val_every"):
        UtteranceBatches(mel_tree, 4, 32, val_every=1, crop_len=24)
    with pytest.raises(ValueError):
        UtteranceBatches(mel_tree, 0, 32, val_every=3, crop_len=24)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError, match="no speaker folders"):
        UtteranceBatches(str(tmp_path / "empty"), 4, 32, crop_len=24)


def test_read_ahead_hands_tuples_through(mel_tree):
    from autoformer_amd.train_embedder import ReadAhead

    direct, ahead = _ub(mel_tree, seed=9), _ub(mel_tree, seed=9)
    feed = ReadAhead(ahead, count=3, depth=2, pin=False)
    for _ in range(3):
        x, labels, lefts = next(feed)
        want = next(direct)
        np.testing.assert_array_equal(x.numpy(), want[0])
        assert np.array_equal(labels, want[1]) and lefts == want[2] and feed.state == direct.state()
    feed.close()


def test_validation_crops():
    from autoformer_amd.train_classifier import centre_crop, even_lefts

    mel = np.arange(10)[:, None] * np.ones((1, 3))
    assert centre_crop(mel, 4)[:, 0].tolist() == [3, 4, 5, 6] and centre_crop(mel, 10).shape == (10, 3)
    assert even_lefts(176, 128, 4) == [0, 16, 32, 48] and even_lefts(128, 128, 4) == [0, 0, 0, 0]
    assert even_lefts(200, 128, 1) == [36] and even_lefts(130, 128, 3) == [0, 1, 2]


# ----------------------------------------------------------------------- CLI
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "autoformer_amd.train_classifier", *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_cli_parser_defaults():
    from autoformer_amd.train_classifier import _parser

    a = _parser().parse_args(["--spmel", "d", "--out", "f"])
    assert (a.batch, a.len_crop, a.lr, a.smooth, a.val_every) == (64, 176, 1e-4, 0.0, 10)
    assert (a.dtype, a.device, a.seed, a.det_init, a.deterministic, a.resume, a.eval_spmel) == \
        ("bf16", "cuda:0", 0, False, False, None, None)
    assert a.num_iters > 0 and a.eval_every > 0 and a.save_every > 0 and a.log_every > 0
    with pytest.raises(SystemExit):
        _parser().parse_args(["--spmel", "d"])                                   # --out is required


def test_cli_refuses_without_a_device(mel_tree, tmp_path):
    import torch

    out = str(tmp_path / "c.ckpt")
    r = _cli("--spmel", mel_tree, "--out", out, "--device", "cpu")
    assert r.returncode != 0 and "the HIP kernels need a GPU" in r.stderr and not os.path.exists(out)
    if not torch.cuda.is_available():
        r = _cli("--spmel", mel_tree, "--out", out)
        assert r.returncode != 0 and "no GPU is available" in r.stderr and not os.path.exists(out)


def test_resume_refuses_a_torn_checkpoint_or_other_speakers(tmp_path):
    import torch

    from autoformer_amd.train_classifier import _load_resume_classifier
    from autoformer_amd.train_embedder import _weights_digest

    path = str(tmp_path / "c.ckpt")
    sd = {"a": torch.arange(6.0).reshape(2, 3), "b": torch.ones(4)}
    torch.save(sd, path)
    torch.save({"iteration": 2, "weights_sha256": _weights_digest(sd)}, path + ".state")
    json.dump(["p225", "p226"], open(path + ".speakers.json", "w"))
    got, state = _load_resume_classifier(path, ["p225", "p226"])
    assert state["iteration"] == 2 and all(torch.equal(got[k], sd[k]) for k in sd)
    for other in (["p226", "p225"], ["p225"], ["p225", "p226", "p227"]):
        with pytest.raises(SystemExit, match="speakers.json lists 2 speakers that are not"):
            _load_resume_classifier(path, other)
    sd["b"][1] = 1.5                                                             # weights of another iteration
    torch.save(sd, path)
    with pytest.raises(SystemExit, match="was not written with these weights"):
        _load_resume_classifier(path, ["p225", "p226"])
