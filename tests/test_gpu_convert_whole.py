"""Whole-utterance conversion on the GPU (autoformer_amd.convert.convert_whole, layers.per_utterance_bn(lens=...)):
ragged batches against the CPU oracle run at B = 1 on each utterance padded to its own P_b, the bf16 mode
against the existing one-utterance path, eval mode, batch independence, the wav-to-wav CLI and
`evaluate --whole`.

Setup: AutoVC(44, 256, 512, freq 8) on closed-form weights, inputs from det_inputs sliced to the lengths of
three batches, one per conv row-tile family of conv_ring.hip:
  (40, 13, 24, 128, 5)  Tmax = 128, the aligned family; 13 needs padding to freq, 5 is shorter than freq
  (176, 150, 64)        Tmax = 176, the one-utterance tiles (128 < Tmax <= 192)
  (40, 24)              Tmax = 40, the general family
Utterance i is converted from speaker i to speaker i + 1 (mod n)."""
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from .conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FREQ = 8
CASES = [(40, 13, 24, 128, 5), (176, 150, 64), (40, 24)]
FP32_BAR = 1e-3      # rel-inf: what test_gpu_evaluate.py and test_convert.py hold one-utterance conversion to


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def rel_inf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def rel_frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def padded(T):
    return -(-T // FREQ) * FREQ


@functools.lru_cache(maxsize=None)
def inputs(lengths):
    """(mels, emb_org, emb_trg) of a case; read-only."""
    from autoformer_amd.detinit import det_inputs

    n = len(lengths)
    x, e = det_inputs(n, max(lengths), seed=51 + n)
    mels = tuple(np.ascontiguousarray(x[i][:lengths[i]]) for i in range(n))
    for a in mels + (e,):
        a.setflags(write=False)
    return mels, e, np.roll(e, -1, axis=0)


@functools.lru_cache(maxsize=None)
def oracle(lengths):
    """mel_postnet (T_b, 80) of each utterance: oracle.autovc_cpu.autovc_forward at B = 1, train mode, on the
    utterance zero-padded to P_b, cut to T_b.  Computed once per case, never modified."""
    from oracle import autovc_cpu as O

    mels, eo, et = inputs(lengths)
    sd = O.make_state(O.autovc_spec())
    out = []
    with torch.no_grad():
        for i, m in enumerate(mels):
            xp = np.zeros((1, padded(m.shape[0]), 80), np.float32)
            xp[0, :m.shape[0]] = m
            o = O.autovc_forward(sd, torch.from_numpy(xp), torch.tensor(eo[i][None]), torch.tensor(et[i][None]), freq=FREQ)
            a = o[1].squeeze(1)[0][:m.shape[0]].numpy().copy()
            a.setflags(write=False)
            out.append(a)
    return tuple(out)


def _autovc(comp, train=True):
    import autoformer_amd as A
    from autoformer_amd.detinit import det_init_
    from autoformer_amd.factory.AutoVC import AutoVC

    A.set_compute(comp)
    m = AutoVC(44, 256, 512, FREQ)
    det_init_(m)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _whole(m, lengths, **kw):
    from autoformer_amd.convert import convert_whole

    mels, eo, et = inputs(lengths)
    out = convert_whole(m, list(mels), eo, et, **kw)
    assert [a.shape for a in out] == [(T, 80) for T in lengths] and all(a.dtype == np.float32 for a in out)
    return out


@pytest.mark.parametrize("lengths", CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp32_matches_the_oracle_and_leaves_the_bn_buffers(lengths):
    """Each utterance of one ragged batch equals the oracle's B = 1 train-mode forward at its own P_b
    (rel-inf < 1e-3); the BatchNorm buffers are bit-identical before and after.  The same rows through the
    existing equal-length per_utterance_bn() on the Tmax-padded batch MISS the bar for every row shorter
    than Tmax: statistics over Tmax rows, conv padding at Tmax -- the function the bar excludes."""
    from autoformer_amd import layers as Lyr
    from autoformer_amd.convert import plan_whole

    m = _autovc("fp32")
    before = {k: v.clone() for k, v in m.state_dict().items()
              if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    assert len(before) == 3 * 11
    assert len(plan_whole(lengths, FREQ)) == 1          # one call, one batch
    got = _whole(m, lengths)
    ref = oracle(lengths)
    rels = [rel_inf(got[i], ref[i]) for i in range(len(lengths))]
    print(f"fp32 ragged {lengths} vs oracle, rel-inf:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < FP32_BAR, rels
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert m.training
    # what the bar excludes
    mels, eo, et = inputs(lengths)
    Tmax = max(padded(T) for T in lengths)
    x = np.zeros((len(lengths), Tmax, 80), np.float32)
    for i, a in enumerate(mels):
        x[i, :a.shape[0]] = a
    with torch.no_grad(), Lyr.per_utterance_bn():
        _, eq, _ = m(torch.from_numpy(x).to(DEV), torch.tensor(eo).to(DEV), torch.tensor(et).to(DEV))
    eq = eq.squeeze(1).cpu().numpy()
    short = [i for i, T in enumerate(lengths) if padded(T) < Tmax]
    wrong = [rel_inf(eq[i][:lengths[i]], ref[i]) for i in short]
    print("  the equal-length path on the short rows:", " ".join(f"{r:.2e}" for r in wrong))
    assert short and min(wrong) > FP32_BAR, wrong


@pytest.mark.parametrize("lengths", CASES, ids=lambda c: "-".join(map(str, c)))
def test_bf16_against_the_one_utterance_path(lengths):
    """bf16 compute against the fp32 oracle, per utterance: relative Frobenius and rel-inf of the ragged batch
    next to those of the EXISTING B = 1 path on the same utterance, Converter(model, len_crop = P_b).convert
    (no crop draw at T <= len_crop).  The ragged path may exceed that baseline by at most 1.5x:
    profiles/eval_grid_bench.txt records batched and one-at-a-time bf16 errors within 1.1x of each other on
    the fixed-length grid; 1.5x leaves room for the different summation order over other lengths.  Both
    columns are printed; profiles/convert_whole_bench.txt records a run.  Measured over the ten utterances:
    ragged Frobenius 2.8e-2 .. 4.0e-2, rel-inf 3.6e-2 .. 7.1e-2 (inside the project's bf16 bars, 5e-2 / 1e-1);
    one at a time 3.6e-2 .. 5.5e-2 and 4.4e-2 .. 1.13e-1 -- the existing path itself is past those bars at
    P = 16 and 24 (its conv output is stored in bf16 before the statistics; the ragged path keeps it fp32)."""
    from autoformer_amd.convert import Converter

    m = _autovc("bf16")
    got = _whole(m, lengths)
    ref = oracle(lengths)
    mels, eo, et = inputs(lengths)
    rows = []
    for i, T in enumerate(lengths):
        one = Converter(m, padded(T), DEV).convert(mels[i], eo[i], et[i])
        assert one.shape == (T, 80)
        rows.append((rel_frob(got[i], ref[i]), rel_frob(one, ref[i]), rel_inf(got[i], ref[i]), rel_inf(one, ref[i])))
        print(f"bf16 T={T:4d} P={padded(T):4d}: frob ragged {rows[-1][0]:.3e} one-at-a-time {rows[-1][1]:.3e} | "
              f"rel-inf ragged {rows[-1][2]:.3e} one-at-a-time {rows[-1][3]:.3e}")
    for T, (fr, fo, ir, io) in zip(lengths, rows):
        assert fr <= 1.5 * fo and ir <= 1.5 * io, (T, fr, fo, ir, io)


def test_eval_mode_equals_one_at_a_time():
    """An eval-mode model (running statistics that are not the identity): each utterance of the ragged batch
    equals Converter(model, P_b).convert at rtol = atol = 1e-5."""
    from autoformer_amd.convert import Converter

    m = _autovc("fp32", train=False)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.linspace(-0.5, 0.5, v.numel()))
            elif k.endswith("running_var"):
                v.copy_(torch.linspace(0.5, 2.0, v.numel()))
    for lengths in CASES:
        got = _whole(m, lengths)
        mels, eo, et = inputs(lengths)
        for i, T in enumerate(lengths):
            one = Converter(m, padded(T), DEV).convert(mels[i], eo[i], et[i])
            torch.testing.assert_close(torch.from_numpy(got[i]), torch.from_numpy(one), rtol=1e-5, atol=1e-5)
    assert not m.training


def test_batches_are_independent():
    """max_batch = 2 with a max_frames that cuts further gives, per utterance, what one batch gives: within
    the fp32 bar, both meet the oracle, and in fp32 bit for bit -- the BatchNorm sums have a fixed order per
    utterance, the recurrences are per utterance, and the fp32 products accumulate each output element over
    K in one order whatever the batch's shape (measured: identical at Tmax = 16, 24, 40 and 128 against one
    batch at 128).  A permuted input permutes the output, bit for bit."""
    from autoformer_amd.convert import plan_whole

    lengths = CASES[0]
    m = _autovc("fp32")
    one = _whole(m, lengths)
    plan = plan_whole(lengths, FREQ, max_batch=2, max_frames=64)
    assert [sorted(idx) for idx, _ in plan] == [[1, 4], [2], [0], [3]]     # 8+16 | 24 | 40 | 128 (over budget alone)
    many = _whole(m, lengths, max_batch=2, max_frames=64)
    ref = oracle(lengths)
    d = [rel_inf(many[i], one[i]) for i in range(len(lengths))]
    print("several batches vs one, rel-inf:", " ".join(f"{r:.2e}" for r in d),
          "| bit-identical:", [bool(np.array_equal(a, b)) for a, b in zip(many, one)])
    assert max(d) < FP32_BAR and max(rel_inf(many[i], ref[i]) for i in range(len(lengths))) < FP32_BAR
    assert all(np.array_equal(a, b) for a, b in zip(many, one))
    # the same batch again: fixed-order sums, no atomics -- bit-identical from run to run
    again = _whole(m, lengths)
    assert all(np.array_equal(a, b) for a, b in zip(again, one))
    from autoformer_amd.convert import convert_whole

    mels, eo, et = inputs(lengths)
    perm = [3, 0, 4, 2, 1]
    out = convert_whole(m, [mels[i] for i in perm], eo[perm], et[perm])
    assert all(np.array_equal(out[k], one[i]) for k, i in enumerate(perm))


# ----------------------------------------------------------------------- CLIs
def _write_wav(path, samples, f0, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(samples) / 22050.0
    x = 0.3 * np.sin(2 * np.pi * f0 * t) + 0.15 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.02 * rng.randn(samples)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(22050)
        w.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _read_pcm(path):
    with wave.open(str(path), "rb") as w:
        assert (w.getframerate(), w.getsampwidth(), w.getnchannels()) == (22050, 2, 1)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def test_cli_wav_to_wav(tmp_path):
    """python -m autoformer_amd.convert --det_init on synthetic wavs of three lengths: one wav per source with
    n_frames(L) * 256 samples, non-silent; another target speaker gives other audio (second run in process)."""
    from autoformer_amd.convert import main
    from autoformer_amd.melgan import n_frames

    sizes = {"a": 11025, "b": 19845, "c": 30000}
    for k, (name, L) in enumerate(sizes.items()):
        _write_wav(tmp_path / f"{name}.wav", L, 110.0 * (k + 1), k)
    for k in range(2):
        _write_wav(tmp_path / f"ref{k}.wav", 26000, 95.0 + 20 * k, 10 + k)
        _write_wav(tmp_path / f"other{k}.wav", 26000, 310.0 + 45 * k, 20 + k)
    common = ["--det_init", "--freq", str(FREQ), "--dtype", "bf16", "--save_mel"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "autoformer_amd.convert", "--src_dir", str(tmp_path), "--ref",
                        str(tmp_path / "ref0.wav"), str(tmp_path / "ref1.wav"), "--out_dir", str(tmp_path / "o1")]
                       + common, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "7 wavs" in r.stdout            # --src_dir takes every wav of the folder, the references too
    assert main(["--src"] + [str(tmp_path / f"{n}.wav") for n in sizes] + ["--ref", str(tmp_path / "other0.wav"),
                str(tmp_path / "other1.wav"), "--out_dir", str(tmp_path / "o2")] + common) == 0
    for name, L in sizes.items():
        a, b = _read_pcm(tmp_path / "o1" / f"{name}.wav"), _read_pcm(tmp_path / "o2" / f"{name}.wav")
        assert a.shape == b.shape == (n_frames(L) * 256,), name
        assert np.abs(a).max() > 0 and np.abs(b).max() > 0
        assert not np.array_equal(a, b)
        assert np.load(tmp_path / "o2" / f"{name}.npy").shape == (n_frames(L), 80)
    assert sorted(os.listdir(tmp_path / "o2")) == sorted([f"{n}.wav" for n in sizes] + [f"{n}.npy" for n in sizes])


def test_evaluate_whole_exports_full_length_wavs(tmp_path):
    """evaluate --wav_dir --whole: every pair's wav has the source's full length (frames * 256), also where
    that is longer than len_crop; in process."""
    import pickle

    from autoformer_amd.detinit import det_inputs, det_melgan_state
    from autoformer_amd.evaluate import main
    from autoformer_amd.melgan import Generator

    root, out = tmp_path / "mels", tmp_path / "wavs"
    frames = {"p1": 70, "p2": 203}
    meta = []
    for k, (spk, T) in enumerate(frames.items()):
        os.makedirs(root / spk)
        x, e = det_inputs(1, T, seed=61 + k)
        np.save(root / spk / "0.npy", x[0])
        meta.append([spk, e[0], f"{spk}/0.npy"])
    with open(root / "test.pkl", "wb") as f:
        pickle.dump(meta, f)
    g = Generator(80, 32, 3)
    sd = {k: torch.from_numpy(v) for k, v in
          det_melgan_state([(k, tuple(v.shape)) for k, v in g.state_dict().items()]).items()}
    torch.save(sd, str(tmp_path / "melgan_state.bin"))
    assert main(["--root", str(root), "--model", "AutoVC", "--det_init", "--wav_dir", str(out), "--whole",
                 "--vocoder_ckpt", str(tmp_path / "melgan_state.bin"), "--dtype", "bf16", "--len_crop", "64",
                 "--freq", "16", "--sound_id", "2", "--max_uttr_idx", "3"]) == 0
    for s, (spk, T) in enumerate(frames.items()):
        for t in range(2):
            pcm = _read_pcm(out / spk / f"{s}_{t}.wav")
            assert pcm.shape == (T * 256,) and np.abs(pcm).max() > 0
