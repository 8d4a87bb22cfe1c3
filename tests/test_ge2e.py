"""Training the embedder, the host side (no GPU): the ledger of the ninth ABI header
(include/autovc_hip_ge2e.h) and its refusals (every check precedes the launch), the equal-error rate, the
speaker-batch sampler on a generated mel tree, and the trainer's command line."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT

HEADER_GE2E = os.path.join(ROOT, "include", "autovc_hip_ge2e.h")


def declared_symbols_ge2e():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_GE2E).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


# ----------------------------------------------------------------------- the ninth header
def test_ge2e_header_symbols():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    declared = declared_symbols_ge2e()
    assert declared == ["avc_ge2e", "avc_ge2e_ws"]
    assert set(declared) == set(_lib.exported_symbols_ge2e())
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg()
               + _lib.exported_symbols_ragged() + _lib.exported_symbols_vocoder())
    assert not set(declared) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]                     # every declared symbol is built
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "ge2e.hip" in _lib.SOURCES
    # the limits the binding quotes are the header's, and admit what the issue asks for
    src = open(HEADER_GE2E).read()
    lim = {k: int(v) for k, v in re.findall(r"#define AVC_GE2E_MAX_(\w+) (\d+)", src)}
    assert lim == {"N": _lib.GE2E_MAX_N, "M": _lib.GE2E_MAX_M, "D": _lib.GE2E_MAX_D, "ROWS": _lib.GE2E_MAX_ROWS}
    assert lim["N"] >= 128 and lim["M"] >= 64 and lim["D"] >= 1024 and lim["ROWS"] >= 128 * 64


def test_ge2e_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)

    def err():
        return Lb.avc_last_error().decode()

    def call(e=p, N=4, M=3, D=8, w=p, L=p, de=ctypes.c_void_p(512), dw=p, ws=p):
        return Lb.avc_ge2e(e, N, M, D, w, L, de, dw, ws, None)

    assert call(N=1) != 0 and "avc_ge2e: bad shape N = 1" in err()
    assert call(M=1) != 0 and "bad shape N = 4, M = 1" in err()
    assert call(D=0) != 0 and "D = 0" in err()
    for name in ("e", "w", "L", "ws"):
        assert call(**{name: None}) != 0 and "avc_ge2e: null pointer" in err(), name
    assert call(de=None) != 0 and "de and dw go together" in err()
    assert call(dw=None) != 0 and "de and dw go together" in err()
    assert call(ws=ctypes.c_void_p(260)) != 0 and "16-byte aligned" in err()
    assert call(de=p, e=p) != 0 and "must not alias" in err()
    assert call(N=_lib.GE2E_MAX_N + 1, M=2) != 0 and "past the LDS layout" in err()
    assert call(M=_lib.GE2E_MAX_M + 1, N=2) != 0 and "past the LDS layout" in err()
    assert call(D=_lib.GE2E_MAX_D + 1) != 0 and "past the LDS layout" in err()
    assert call(N=128, M=65) != 0 and "N * M <= 8192" in err()
    # the size query: 0 for what the call refuses, and what the header's layout says otherwise
    assert Lb.avc_ge2e_ws(1, 2, 8) == 0 and Lb.avc_ge2e_ws(2, 1, 8) == 0 and Lb.avc_ge2e_ws(2, 2, 0) == 0
    assert Lb.avc_ge2e_ws(128, 65, 8) == 0

    def r4(v):
        return (v + 3) & ~3
    for N, M, D in ((2, 2, 256), (3, 2, 8), (5, 3, 100), (4, 5, 257), (128, 64, 1024)):
        R = N * M
        floats = r4(N * D) + r4(N) + 2 * r4(R * N) + r4(R * D) + 2 * r4(R)
        assert Lb.avc_ge2e_ws(N, M, D) == 4 * floats, (N, M, D)


def test_ge2e_wrapper_needs_a_device():
    import torch

    from autoformer_amd.ge2e import GE2ELoss, ge2e_loss

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ge2e_loss(torch.randn(6, 8), 3, 2, torch.tensor(10.0))
    assert GE2ELoss().w.item() == 10.0 and [n for n, _ in GE2ELoss().named_parameters()] == ["w"]


# ----------------------------------------------------------------------- eer
def test_eer():
    from autoformer_amd.train_embedder import eer

    assert eer([0.9, 0.8], [0.1, 0.2, 0.3]) == 0.0                            # separable
    assert eer([0.1, 0.2, 0.3], [0.1, 0.2, 0.3]) == pytest.approx(0.5, abs=1e-12)   # targets equal to non-targets
    assert eer([0.5], [0.5]) == pytest.approx(0.5, abs=1e-12)
    # the curve crosses on the vertical segment at FAR = 1/4
    assert eer([0.9, 0.8, 0.4], [0.7, 0.3, 0.2, 0.1]) == pytest.approx(0.25, abs=1e-12)
    assert eer([0.1, 0.2], [0.8, 0.9]) == pytest.approx(1.0, abs=1e-12)      # inverted scores
    with pytest.raises(ValueError):
        eer([], [0.1])


# ----------------------------------------------------------------------- SpeakerBatches
def _tree(root, speakers, seed=0):
    """speakers: {name: [frame counts]}; every mel is (T, 80) with its own values."""
    rng = np.random.default_rng(seed)
    for spk, lens in speakers.items():
        os.makedirs(os.path.join(root, spk))
        for u, T in enumerate(lens):
            np.save(os.path.join(root, spk, f"u{u:02d}.npy"), rng.standard_normal((T, 80)).astype(np.float32))
    return root


@pytest.fixture(scope="module")
def mel_tree(tmp_path_factory):
    spk = {f"s{k}": [40 + 3 * k + u for u in range(5)] for k in range(6)}
    spk["short"] = [20, 25, 31, 31, 31]          # every utterance below partial[1] = 32
    spk["thin"] = [50, 50, 31, 20, 10]           # two usable utterances only
    return _tree(str(tmp_path_factory.mktemp("spmel")), spk)


def test_speaker_batches(mel_tree, capsys):
    from autoformer_amd.train_embedder import SpeakerBatches

    sb = SpeakerBatches(mel_tree, 4, 3, partial=(24, 32), seed=5)
    out = capsys.readouterr().out
    assert "6 speakers, 2 left out" in out                                      # short and thin, with the count
    assert [s for s, _ in sb.speakers] == [f"s{k}" for k in range(6)]
    seen_T = set()
    for _ in range(12):
        x = next(sb)
        assert x.dtype == np.float32 and x.shape[0] == 12 and x.shape[2] == 80
        T = x.shape[1]
        assert 24 <= T <= 32                                                    # one T in range per batch
        seen_T.add(T)
        rows = sb.last
        assert len(rows) == 12
        spk = [rows[n * 3][0] for n in range(4)]
        assert len(set(spk)) == 4                                               # N distinct speakers
        for n in range(4):
            assert {r[0] for r in rows[n * 3:n * 3 + 3]} == {spk[n]}            # speaker-major rows
            assert len({r[1] for r in rows[n * 3:n * 3 + 3]}) == 3              # M distinct utterances
        for r, (s, path, off) in enumerate(rows):
            src = np.load(path)
            assert os.path.basename(os.path.dirname(path)) == s
            assert 0 <= off and off + T <= src.shape[0]                         # the crop lies inside its utterance
            np.testing.assert_array_equal(x[r], src[off:off + T])
    assert len(seen_T) > 1                                                      # the length is drawn, not fixed


def test_speaker_batches_reproducible_and_resumable(mel_tree):
    from autoformer_amd.train_embedder import SpeakerBatches

    a, b = SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=1), SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=1)
    c = SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=2)
    xa = [next(a) for _ in range(3)]
    for x, y in zip(xa, [next(b) for _ in range(3)]):
        np.testing.assert_array_equal(x, y)                                    # same seed, same sequence
    assert any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(xa, [next(c) for _ in range(3)]))
    st = a.state()
    nxt = [next(a) for _ in range(3)]
    c.set_state(st)
    for x, y in zip(nxt, [next(c) for _ in range(3)]):
        np.testing.assert_array_equal(x, y)                                    # set_state(state()) continues exactly
    a.set_state(st)
    np.testing.assert_array_equal(next(a), nxt[0])


def test_speaker_batches_leaves_the_global_states_alone(mel_tree):
    from autoformer_amd.train_embedder import SpeakerBatches

    np.random.seed(123)
    random.seed(123)
    before, before_py = np.random.get_state(), random.getstate()
    sb = SpeakerBatches(mel_tree, 3, 2, (24, 32), seed=0)
    next(sb), next(sb)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert random.getstate() == before_py


def test_speaker_batches_refuses_too_few_speakers(mel_tree):
    from autoformer_amd.train_embedder import SpeakerBatches

    with pytest.raises(ValueError, match="6 usable speakers, a batch needs N = 7"):
        SpeakerBatches(mel_tree, 7, 3, (24, 32))
    with pytest.raises(ValueError, match="usable speakers"):
        SpeakerBatches(mel_tree, 4, 3, (24, 60))                              # no utterance is 60 frames long
    with pytest.raises(ValueError):
        SpeakerBatches(mel_tree, 1, 3, (24, 32))
    with pytest.raises(ValueError):
        SpeakerBatches(mel_tree, 4, 3, (33, 32))


def test_read_ahead_keeps_the_consumers_state(mel_tree):
    """The background reader hands out the sampler's own sequence, and its `state` is the sampler state after
    the batch handed out last, however far ahead the thread has drawn."""
    import time

    from autoformer_amd.train_embedder import ReadAhead, SpeakerBatches

    direct = SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=9)
    ahead = SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=9)
    feed = ReadAhead(ahead, count=5, depth=2, pin=False)
    assert feed.state == direct.state()                                          # nothing handed out yet
    deadline = time.time() + 30
    while feed._q.qsize() < 2 and time.time() < deadline:                         # the thread runs ahead
        time.sleep(0.01)
    assert feed._q.qsize() == 2 and ahead.state() != direct.state()
    for _ in range(3):
        np.testing.assert_array_equal(next(feed).numpy(), next(direct))
        assert feed.state == direct.state()
    resumed = SpeakerBatches(mel_tree, 4, 3, (24, 32), seed=0)
    resumed.set_state(feed.state)
    np.testing.assert_array_equal(next(resumed), next(direct))                    # a checkpoint taken here continues exactly
    feed.close()
    assert not feed._thread.is_alive()

    class Broken:
        def state(self):
            return "s"

        def __next__(self):
            raise OSError("unreadable mel")
    with pytest.raises(OSError, match="unreadable mel"):
        next(ReadAhead(Broken(), count=1, pin=False))                           # loader errors reach the consumer


def test_resume_refuses_a_torn_checkpoint(tmp_path):
    """FILE.state carries a digest of the weights it was written with; another FILE beside it is refused."""
    import torch

    from autoformer_amd.train_embedder import _load_resume, _weights_digest

    path = str(tmp_path / "dv.ckpt")
    sd = {"a": torch.arange(6.0).reshape(2, 3), "b": torch.ones(4)}
    torch.save(sd, path)
    torch.save({"iteration": 2, "weights_sha256": _weights_digest(sd)}, path + ".state")
    got, state = _load_resume(path)
    assert state["iteration"] == 2 and all(torch.equal(got[k], sd[k]) for k in sd)
    sd["b"][1] = 1.5                                                             # weights of another iteration
    torch.save(sd, path)
    with pytest.raises(SystemExit, match="was not written with these weights"):
        _load_resume(path)


# ----------------------------------------------------------------------- CLI
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "autoformer_amd.train_embedder", *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_cli_help():
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for opt in ("--spmel", "--out", "--speakers", "--utterances", "--partial", "--num_iters", "--lr", "--eval_spmel",
                "--eval_every", "--save_every", "--resume", "--dtype", "--device", "--seed", "--det_init",
                "--deterministic", "--log_every"):
        assert opt in r.stdout, opt


def test_cli_refuses_without_a_device(mel_tree, tmp_path):
    import torch

    out = str(tmp_path / "dv.ckpt")
    r = _cli("--spmel", mel_tree, "--out", out, "--device", "cpu")
    assert r.returncode != 0 and "the HIP kernels need a GPU" in r.stderr and not os.path.exists(out)
    if not torch.cuda.is_available():
        r = _cli("--spmel", mel_tree, "--out", out)
        assert r.returncode != 0 and "no GPU is available" in r.stderr and not os.path.exists(out)
