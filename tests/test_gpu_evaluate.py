"""The conversion grid and the Evaluator on the GPU (autoformer_amd/evaluate.py): a batched grid under
per-utterance BatchNorm against the CPU oracle run at B = 1 per pair, the bf16 mode, the untouched
BatchNorm buffers, eval mode, ragged chunking, the fall-back family, generate_result against a B = 1
loop, the CLI's wav export, and the gradient guard.

Setup of the grid tests: AutoVC(44, 256, 512, 16) on closed-form weights, T = 64, three speakers, one
source shorter than T (padded)."""
import functools
import os
import pickle
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from .conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, FREQ, N = 64, 16, 3
SHORT = T - 10   # source 1's frames


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def rel_inf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def _sources():
    from autoformer_amd.detinit import det_inputs

    x, e = det_inputs(N, T, seed=31)
    return [x[0], x[1][:SHORT], x[2]], e


def _autovc(comp, train=True):
    import autoformer_amd as A
    from autoformer_amd.detinit import det_init_
    from autoformer_amd.factory.AutoVC import AutoVC

    A.set_compute(comp)
    m = AutoVC(44, 256, 512, FREQ)
    det_init_(m)
    m = m.to(DEV)
    return m.train() if train else m.eval()


@functools.lru_cache(maxsize=None)
def oracle_grid():
    """mel_postnet (T, 80) of every pair from oracle.autovc_cpu.autovc_forward at B = 1, train mode (the
    reference's conversion); computed once, never modified."""
    from oracle import autovc_cpu as O

    srcs, e = _sources()
    sd = O.make_state(O.autovc_spec())
    out = []
    with torch.no_grad():
        for s in range(N):
            xp = np.zeros((1, T, 80), np.float32)
            xp[0, :srcs[s].shape[0]] = srcs[s]
            for t in range(N):
                o = O.autovc_forward(sd, torch.from_numpy(xp), torch.from_numpy(e[s][None]),
                                     torch.from_numpy(e[t][None]), freq=FREQ)
                a = o[1].squeeze(1)[0].numpy().copy()
                a.setflags(write=False)
                out.append(a)
    return tuple(out)


def _grid(m, **kw):
    from autoformer_amd.evaluate import convert_grid

    srcs, e = _sources()
    mels, pads = convert_grid(m, srcs, e, len_crop=T, **kw)
    assert len(mels) == N * N and pads == [0] * N + [T - SHORT] * N + [0] * N
    assert all(a.shape == (T, 80) and a.dtype == np.float32 for a in mels)
    return mels


def test_grid_matches_oracle_fp32_and_leaves_the_bn_buffers():
    """(a) every pair of the batched train-mode grid equals the oracle's B = 1 train-mode forward:
    rel-inf < 1e-3 per pair, the bar tests/test_convert.py holds the one-utterance conversion to.  Batch-wide
    statistics (a plain B = 9 forward, or this tree without per_utterance_bn) miss it.
    (c) every BatchNorm buffer is bit-identical before and after."""
    m = _autovc("fp32")
    before = {k: v.clone() for k, v in m.state_dict().items()
              if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    assert len(before) == 3 * 11                       # 3 encoder + 3 decoder + 5 postnet BatchNorms
    mels = _grid(m)
    ref = oracle_grid()
    rels = [rel_inf(mels[i], ref[i]) for i in range(N * N)]
    print("fp32 grid vs oracle, rel-inf per pair:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < 1e-3, rels
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert m.training
    # what the bar excludes: the same rows through a plain batched forward (statistics over all rows)
    srcs, e = _sources()
    x = np.zeros((N, T, 80), np.float32)
    for s in range(N):
        x[s, :srcs[s].shape[0]] = srcs[s]
    with torch.no_grad():
        xd, ed = torch.from_numpy(x).to(DEV), torch.from_numpy(e).to(DEV)
        _, plain, _ = m(xd, ed, ed)
    plain = plain.squeeze(1).cpu().numpy()
    assert max(rel_inf(plain[s], ref[s * N + s]) for s in range(N)) > 1e-3


def test_grid_matches_oracle_bf16():
    """(b) bf16 compute against the fp32 oracle, per pair, at the bf16 forward bars
    tests/test_gpu_model.py::test_autovc_bf16_loose applies to AutoVC's mel_postnet (its lines 117-118):
    relative Frobenius < 5e-2 and rel-inf < 1e-1.  Measured (profiles/eval_grid_bench.txt): Frobenius
    3.7e-2 .. 4.8e-2, rel-inf 4.0e-2 .. 9.5e-2 over the nine pairs, bit-identical from run to run; the
    B = 1 Converter loop in bf16 sits at 4.2e-2 .. 5.8e-2 / 5.1e-2 .. 8.6e-2 on the same inputs."""
    mels = _grid(_autovc("bf16"))
    ref = oracle_grid()
    frob = [float(np.linalg.norm(mels[i].astype(np.float64) - ref[i]) / np.linalg.norm(ref[i])) for i in range(N * N)]
    rels = [rel_inf(mels[i], ref[i]) for i in range(N * N)]
    print("bf16 grid vs oracle: frob", " ".join(f"{r:.2e}" for r in frob), "| rel-inf", " ".join(f"{r:.2e}" for r in rels))
    assert max(frob) < 5e-2 and max(rels) < 1e-1, (frob, rels)


def test_eval_mode_grid_equals_one_at_a_time():
    """(d) an eval-mode model (running statistics: every row independent already): the grid equals
    Converter.convert at B = 1, at the 1e-5 tolerances of tests/test_convert.py."""
    from autoformer_amd.convert import Converter

    m = _autovc("fp32", train=False)
    with torch.no_grad():   # running statistics that are not the identity
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.linspace(-0.5, 0.5, v.numel()))
            elif k.endswith("running_var"):
                v.copy_(torch.linspace(0.5, 2.0, v.numel()))
    mels = _grid(m)
    srcs, e = _sources()
    conv = Converter(m, T, DEV)
    for i, (s, t) in enumerate((s, t) for s in range(N) for t in range(N)):
        one = conv.convert(srcs[s], e[s], e[t])
        assert one.shape == (srcs[s].shape[0], 80)
        torch.testing.assert_close(torch.from_numpy(mels[i][:one.shape[0]]), torch.from_numpy(one), rtol=1e-5, atol=1e-5)
    assert not m.training


def test_ragged_chunking():
    """(e) max_batch = 4 -- chunks of 4, 4 and a ragged 1 (and the three encoder rows in one chunk) --
    meets the same bar against the oracle as max_batch = 64, and the two agree within it."""
    m = _autovc("fp32")
    small, big = _grid(m, max_batch=4), _grid(m, max_batch=64)
    ref = oracle_grid()
    assert max(rel_inf(small[i], ref[i]) for i in range(N * N)) < 1e-3
    assert max(rel_inf(small[i], big[i]) for i in range(N * N)) < 1e-3
    one = _grid(m, max_batch=1)   # every chunk a single row, the encoder's too
    assert max(rel_inf(one[i], ref[i]) for i in range(N * N)) < 1e-3


def test_fallback_family_equals_the_converter_loop():
    """(f) MetaConv is not batched: the grid takes Converter.get_trans_mel pair by pair on the crops it
    drew -- the same draws, bit-identical results (one source shorter than len_crop, one longer)."""
    import autoformer_amd as A
    from autoformer_amd.convert import Converter
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.evaluate import batched_family, convert_grid
    from autoformer_amd.factory.MetaConv import MetaConv

    A.set_compute("fp32")
    Tm = 176
    x, e = det_inputs(2, Tm + 40, seed=33)
    srcs = [x[0][:Tm - 16], x[1]]
    m = MetaConv(44, 256, 512, 22)
    det_init_(m)
    m = m.to(DEV).train()
    assert not batched_family(m)
    np.random.seed(9)
    mels, pads = convert_grid(m, srcs, e, len_crop=Tm)
    assert pads == [16, 16, 0, 0]
    np.random.seed(9)
    conv = Converter(m, Tm, DEV)
    for i, (s, t) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        one = conv.convert(srcs[s], e[s], e[t], trim=False)
        assert np.array_equal(mels[i], one), (s, t)


# ----------------------------------------------------------------------- Evaluator
def _tree(root, n_spk=3, n_utt=6, seed=41):
    """<root>/<speaker>/<k>.npy mels (lengths around T, one shorter, some longer) and the test.pkl list."""
    from autoformer_amd.detinit import det_inputs

    lens = [T, T + 9, T - 7, T + 30, T, T + 3]
    meta = []
    for s in range(n_spk):
        spk = f"p{230 - s}"      # listed in descending order: build_metadata sorts
        os.makedirs(os.path.join(root, spk))
        x, e = det_inputs(n_utt, T + 40, seed=seed + s)
        row = [spk, e[0]]
        for u in range(n_utt):
            np.save(os.path.join(root, spk, f"{u}.npy"), x[u][:lens[(u + s) % len(lens)]])
            row.append(f"{spk}/{u}.npy")
        meta.append(row)
    with open(os.path.join(root, "test.pkl"), "wb") as f:
        pickle.dump(meta, f)
    return meta


class _Cfg:
    pass


def _config(root, meta, judge):
    c = _Cfg()
    c.root, c.num_speaker, c.batch_size, c.max_uttr_idx, c.erroment_num = str(root), 3, 2, 8, 2
    c.len_crop, c.device, c.embedder, c.metadata = T, DEV, judge, meta
    c.all_speaker = sorted(d[0] for d in meta)
    return c


def test_generate_result_equals_a_one_at_a_time_loop(tmp_path):
    """(g) generate_result on a generated tree (3 speakers x 6 utterances) with an LstmDV judge on
    closed-form weights: (3, 3, 3), equal to 1e-4 absolute to Converter.get_trans_mel + the judge at
    B = 1 + cos_scores, looped here under the same seeds; get_real_data_cos shapes and ranges."""
    import random

    from autoformer_amd.convert import Converter
    from autoformer_amd.detinit import det_init_
    from autoformer_amd.embed import cos_scores, embed_utterances
    from autoformer_amd.evaluate import Evaluator
    from autoformer_amd.factory.LstmDV import LstmDV

    m = _autovc("fp32")
    judge = LstmDV()
    det_init_(judge)
    judge = judge.to(DEV).eval()
    meta = _tree(str(tmp_path))
    random.seed(3)
    np.random.seed(3)
    E = Evaluator(_config(tmp_path, meta, judge))
    assert [d[0] for d in E.metadata] == ["p228", "p229", "p230"]
    assert len(E.enrroment_idx) == 2 and len(E.remain_idx) == 4 and len(E.all_dv) == 3
    assert tuple(E.all_dv[0].shape) == (1, 256)
    np.random.seed(17)
    res = E.generate_result([m], sound_id=2)
    assert len(res) == 1 and res[0].shape == (3, 3, 3)
    # the loop: pair after pair, source crop then target crop from numpy's global state
    np.random.seed(17)
    conv = Converter(m, T, DEV)
    dvs = np.concatenate([d.cpu().numpy() for d in E.all_dv])
    want = np.zeros((3, 3, 3))
    for s in range(3):
        for t in range(3):
            ms, mt = (np.load(os.path.join(str(tmp_path), E.metadata[i][2])) for i in (s, t))
            _, _, trans = conv.get_trans_mel(ms, mt, E.metadata[s][1], E.metadata[t][1])
            emb = embed_utterances(judge, [trans[0].cpu().numpy()], T)
            want[s, t] = cos_scores(emb, dvs)[0]
    print("generate_result vs the B = 1 loop: max abs", float(np.abs(res[0] - want).max()))
    assert np.abs(res[0] - want).max() < 1e-4
    assert (res[0] >= 0).all() and (res[0] <= 1 + 1e-6).all()
    rc, rc_other = E.get_cos_rc(res[0])
    tr, tr_other = E.get_cos_trans(res[0])
    assert all(0 <= v <= 1 + 1e-6 for v in (rc, rc_other, tr, tr_other))
    cos, std = E.get_real_data_cos()
    assert cos.shape == (3, 3) and std.shape == (3, 3)
    assert (cos >= 0).all() and (cos <= 1 + 1e-6).all() and (std >= 0).all() and (std <= 0.5 + 1e-6).all()


def test_cli_writes_the_grid_as_wavs(tmp_path):
    """(h) python -m autoformer_amd.evaluate --det_init --wav_dir (and an LstmDV judge, for the two summary
    lines), the MelGAN generator from a checkpoint file written here:
    <wav_dir>/<source speaker>/<source_id>_<target_id>.wav for the 9 pairs, 22,050 Hz 16-bit mono,
    (T - pad) * 256 samples.  A fresh child process under its own time limit."""
    from autoformer_amd.detinit import det_melgan_state
    from autoformer_amd.melgan import Generator

    root, out = tmp_path / "mels", tmp_path / "wavs"
    meta = _tree(str(root))
    g = Generator(80, 32, 3)
    sd = {k: torch.from_numpy(v) for k, v in
          det_melgan_state([(k, tuple(v.shape)) for k, v in g.state_dict().items()]).items()}
    torch.save(sd, str(tmp_path / "melgan_state.bin"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "autoformer_amd.evaluate", "--root", str(root), "--meta", "test.pkl",
                        "--model", "AutoVC", "--det_init", "--wav_dir", str(out), "--vocoder_ckpt",
                        str(tmp_path / "melgan_state.bin"), "--dtype", "bf16", "--len_crop", str(T), "--freq", str(FREQ),
                        "--seed", "5", "--embedder", "LstmDV", "--erroment_num", "2", "--max_uttr_idx", "8"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "9 wavs" in r.stdout
    assert "reconstruction: cos to own speaker" in r.stdout and "conversion: cos to the target speaker" in r.stdout
    names = sorted(d[0] for d in meta)
    by_name = {d[0]: d for d in meta}
    for s in range(3):
        frames = min(T, np.load(os.path.join(str(root), by_name[names[s]][2])).shape[0])   # sound_id 2
        for t in range(3):
            with wave.open(str(out / names[s] / f"{s}_{t}.wav"), "rb") as w:
                assert (w.getframerate(), w.getsampwidth(), w.getnchannels()) == (22050, 2, 1)
                assert w.getnframes() == frames * 256, (s, t)
                pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
            assert np.abs(pcm).max() > 0
    assert sum(len(f) for _, _, f in os.walk(str(out))) == 9
    assert any(min(T, np.load(os.path.join(str(root), d[2])).shape[0]) < T for d in meta)   # one padded source


def test_per_utterance_bn_needs_no_grad():
    """(i) entering per_utterance_bn with gradients enabled raises, and so does a train-mode conv + BN
    layer reached with them enabled inside it; eval-mode BatchNorm keeps its path."""
    from autoformer_amd import layers as Lyr

    m = _autovc("fp32")
    srcs, e = _sources()
    x = torch.from_numpy(np.stack([srcs[0], srcs[2]])).to(DEV)
    ed = torch.from_numpy(e[:2]).to(DEV)
    with pytest.raises(RuntimeError, match="forward-only"):
        with Lyr.per_utterance_bn():
            m(x, ed, ed)
    with torch.no_grad():
        with Lyr.per_utterance_bn():
            with torch.enable_grad():
                with pytest.raises(RuntimeError, match="forward-only"):
                    m(x, ed, ed)
            a = m(x, ed, ed)[1]
        b = m(x, ed, ed)[1]
    assert not Lyr._PER_UTT["on"]
    assert not torch.equal(a, b)        # per-utterance against batch statistics: different functions
    m.eval()
    with torch.no_grad():
        with Lyr.per_utterance_bn():
            c = m(x, ed, ed)[1]
        d = m(x, ed, ed)[1]
    assert torch.equal(c, d)
