"""The polyphase resampling kernel (resample.hip, include/autovc_hip_resample.h) and what is built on it:
Resample.frames, make_spec.wav_to_mel / convert_tree with resampling switched on.

Reference r: the fp64 restatement of tests/resample_ref.py (a per-output walk over resampy's half table,
no polyphase table).  Metric, per utterance:
    e = max_t |out - r| / max(max_t |r|, tiny)
Bar: max(4 x d32, 4 x 2^-24), d32 the largest e of a CPU fp32 evaluation of the same fp32 table in tap
order (tests/test_resample.py apply_table) over the same inputs, computed here at run time; the factor 4
covers the FMA against the separately rounded product, the floor is fp32 unit round-off.  A tap, phase
or sample off by one puts e above 0.5 (tests/test_resample.py test_impulses_reproduce_the_filter_columns).
"""
import functools
import os

import numpy as np
import pytest
import torch

from . import audio_ref as A
from . import resample_ref as R
from .test_audio import write_wav
from .test_resample import apply_table, call_resample, ref, refusal_cases, rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATES = (48000, 16000, 44100)
NAMES = ("zeros", "const", "imp_first", "imp_last", "imp_mid", "sine1k", "noise")
FLOOR = 4.0 * 2.0 ** -24


def dev(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def table(fs):
    from autoformer_amd.resample import resample_table

    return resample_table(fs, device=DEV)


@functools.lru_cache(maxsize=None)
def resampler(fs):
    from autoformer_amd.resample import Resample

    return Resample(fs)


# input lengths: the base ones, then those whose output count is one below, at and one above a multiple of
# L (3 periods) and of the kernel's output tile (one tile: a second workgroup starts), and a period past it
LENGTHS = {"1": lambda tb, tile: 1, "100": lambda tb, tile: 100, "320": lambda tb, tile: 320,
           "321": lambda tb, tile: 321, "5000": lambda tb, tile: 5000,
           "3M-1": lambda tb, tile: 3 * tb.M - 1, "3M": lambda tb, tile: 3 * tb.M, "3M+1": lambda tb, tile: 3 * tb.M + 1,
           "tile-1": lambda tb, tile: tile - 1, "tile": lambda tb, tile: tile, "tile+1": lambda tb, tile: tile + 1,
           "tile+M": lambda tb, tile: tile + tb.M}


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("length", list(LENGTHS))
def test_kernel_within_the_bar(fs, length):
    """Seven inputs of one length in one launch, each against the fp64 restatement."""
    tb = table(fs)
    per_tile = tb.tile() // tb.L * tb.M           # inputs that give exactly one tile of outputs
    N = LENGTHS[length](tb, per_tile)
    if length.startswith("tile"):
        assert (per_tile * tb.L) % tb.M == 0 and per_tile * tb.L // tb.M == tb.tile()
    sig = R.signals(N, fs)
    x = np.stack([sig[n] for n in NAMES])
    out, out_lens = resampler(fs).frames(dev(x))
    torch.cuda.synchronize()
    n_out = R.out_len(N, fs, 22050)
    assert out_lens == [n_out] * len(NAMES) and out.shape == (len(NAMES), n_out) and out.dtype == torch.float32
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    d32 = max(rel(apply_table(tb, sig[n], np.float32), ref(n, N, fs)) for n in NAMES)
    bar = max(4.0 * d32, FLOOR)
    worst = 0.0
    for i, n in enumerate(NAMES):
        e = rel(got[i], ref(n, N, fs))
        worst = max(worst, e)
        assert e <= bar, (n, e, bar)
        if (N * tb.L) % tb.M:
            assert got[i, -1] == 0.0            # librosa's pad sample
    assert not got[0].any()                     # zeros in, exact zeros out
    print(f"{fs} N={N} ({n_out} out, tile {tb.tile()}): e = {worst:.2e}, d32 = {d32:.2e}, bar {bar:.2e}")


@pytest.mark.parametrize("fs", RATES)
def test_ragged_batch_in_one_launch(fs):
    """lens = [5000, 100, 321], stride 5000, one launch through the C entry.  The input rows are NaN past
    lens[b] (a read past an utterance's end would show), the output is prefilled with NaN between two
    guard rows (every element must be written, zeros included; nothing outside), and each row equals its
    single-utterance result bit for bit."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    tb = table(fs)
    lens = [5000, 100, 321]
    x = np.full((3, 5000), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = R.signals(n, fs)["noise"]
    xd = dev(x)
    out_lens = [R.out_len(n, fs, 22050) for n in lens]
    stride = max(out_lens)
    host, tab, wts = tb.on(DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    buf = torch.full((5, stride), float("nan"), device=DEV)
    L.call("avc_resample", xd.data_ptr(), 5000, (L.c_int * 3)(*lens), lens_dev.data_ptr(), 3, wts.data_ptr(),
           tb.n_weights, host, tab.data_ptr(), tb.L, tb.M, tb.taps, buf[1:4].data_ptr(), stride, K.stream())
    torch.cuda.synchronize()
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[4]).all()
    got = buf[1:4].cpu().numpy()
    assert np.isfinite(got).all()
    for b, n in enumerate(lens):
        nv = n * tb.L // tb.M
        assert not got[b, nv:].any() and got[b, :nv].any()
        single, sl = resampler(fs).frames(xd[b:b + 1, :n])
        assert sl == [out_lens[b]] and np.array_equal(single[0].cpu().numpy(), got[b, :out_lens[b]])
        e = rel(got[b, :out_lens[b]], ref("noise", n, fs))
        d32 = rel(apply_table(tb, x[b, :n], np.float32), ref("noise", n, fs))
        print(f"{fs} row {b} (N = {n}): e = {e:.2e}, d32 = {d32:.2e}")
        assert e <= max(4.0 * d32, FLOOR)
    # the module on the same batch (the NaN padding is never read), and on a list of utterances
    f1, l1 = resampler(fs).frames(xd, lens=lens)
    f2, l2 = resampler(fs).frames([xd[b, :n] for b, n in enumerate(lens)])
    assert l1 == l2 == out_lens and torch.equal(f1, buf[1:4]) and torch.equal(f2, f1)


def test_same_rate_bypass_and_host_tensors():
    from autoformer_amd.resample import Resample

    x = dev(R.signals(500, 22050)["noise"])[None]
    out, lens = Resample(22050).frames(x, lens=[400])
    assert out is x and lens == [400]
    with pytest.raises(RuntimeError):
        resampler(48000).frames(x.cpu())


def test_host_refusals_launch_nothing():
    """The refusals of tests/test_resample.py with real device pointers: -1, the message, an untouched output."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    host, tab, wts = table(48000).on(DEV)
    x = torch.zeros(2, 5000, device=DEV)
    out = torch.full((2, 2297), 3.5, device=DEV)
    lens_dev = torch.tensor([5000, 100], dtype=torch.int32, device=DEV)   # alive until the valid call has run
    ptrs = {"x": x.data_ptr(), "lens_dev": lens_dev.data_ptr(), "weights": wts.data_ptr(), "tab_dev": tab.data_ptr(),
            "out": out.data_ptr()}
    for what, over, msg in refusal_cases():
        assert call_resample(Lb, ptrs, **over) == -1, what
        assert msg in Lb.avc_last_error(), (what, Lb.avc_last_error())
    torch.cuda.synchronize()
    assert (out == 3.5).all()
    assert call_resample(Lb, ptrs) == 0         # the valid call the cases are overrides of
    torch.cuda.synchronize()
    assert not out.any()


# ----------------------------------------------------------------------- make_spec with resampling
@functools.lru_cache(maxsize=None)
def a2m():
    from autoformer_amd.melgan import Audio2Mel

    m = Audio2Mel().to(DEV)
    m.load_state_dict({"mel_basis": torch.from_numpy(A.mel_basis()), "window": torch.hann_window(1024)})
    return m


def test_wav_to_mel_from_48k_is_the_fp64_chain():
    """wav_to_mel(x, 48000, resample=True) against restated resample -> peak normalise -> fp64 mel, with
    test_gpu_audio2mel.py's per-frame metric.  Bar: 4 x the figure of the fp32 CPU composition (fp32 table
    in tap order -> x / max|x| in fp32 -> F.pad + torch.stft + matmul + log10) over the same inputs.  A
    1 kHz sine synthesised at 48 kHz peaks in the same mel bin as one synthesised at 22050 Hz."""
    from autoformer_amd import make_spec as MS

    from .test_gpu_audio2mel import composition

    basis = A.mel_basis().astype(np.float64)
    tb = table(48000)
    N = 12000
    sig = R.signals(N, 48000)
    inputs = {"noise": sig["noise"], "sine1k": 0.3 * sig["sine1k"], "imp_mid": sig["imp_mid"]}
    refs, comp = {}, {}
    for n, x in inputs.items():
        refs[n] = A.linear_mel(A.peak_normalise(R.resample(x, 48000, 22050)), basis)
        y32 = apply_table(tb, x, np.float32)
        comp[n] = float(A.frame_error(composition(y32 / np.abs(y32).max()), refs[n]).max())
    bar = 4.0 * max(comp.values())
    assert 1e-8 < bar < 1e-5, comp
    mels = {}
    for n, x in inputs.items():
        mels[n] = MS.wav_to_mel(x, 48000, a2m=a2m(), resample=True)
        T = A.n_frames(R.out_len(N, 48000, 22050))
        assert mels[n].shape == (T, 80) == refs[n].shape and mels[n].dtype == np.float32
        e = float(A.frame_error(mels[n], refs[n]).max())
        print(f"{n}: e = {e:.2e}, composition {comp[n]:.2e}, bar {bar:.2e}")
        assert e <= bar
    native = MS.wav_to_mel(0.3 * R.signals(5513, 22050)["sine1k"], 22050, a2m=a2m())
    assert mels["sine1k"][4:-4].mean(axis=0).argmax() == native[4:-4].mean(axis=0).argmax()
    with pytest.raises(ValueError, match="48000 Hz"):
        MS.wav_to_mel(inputs["noise"], 48000, a2m=a2m())        # the default still refuses


def test_convert_tree_with_resample(tmp_path):
    """python -m autoformer_amd.make_spec --resample on a two-speaker tree of 48 kHz and 22.05 kHz PCM16 wavs."""
    from autoformer_amd import make_spec as MS
    from autoformer_amd.resample import out_len

    rng = np.random.RandomState(12)
    wavs = {("s1", "a.wav"): (48000, 9000), ("s1", "b.wav"): (22050, 3000), ("s2", "c.wav"): (48000, 7001),
            ("s2", "d.wav"): (22050, 5000), ("s2", "e.wav"): (48000, 12000)}
    for (spk, fn), (fs, n) in wavs.items():
        os.makedirs(tmp_path / "wav" / spk, exist_ok=True)
        write_wav(tmp_path / "wav" / spk / fn, 0.2 * rng.randn(n).clip(-3, 3), fs=fs)
    with pytest.raises(ValueError, match=r"s1/a\.wav.*48000 Hz"):
        MS.main(["--wav_dir", str(tmp_path / "wav"), "--out_dir", str(tmp_path / "no")])
    assert not os.path.exists(tmp_path / "no")
    MS.main(["--wav_dir", str(tmp_path / "wav"), "--out_dir", str(tmp_path / "spmel"), "--max_batch", "2",
             "--resample"])
    assert sorted(os.listdir(tmp_path / "spmel" / "s1")) == ["a..npy", "b..npy"]
    assert sorted(os.listdir(tmp_path / "spmel" / "s2")) == ["c..npy", "d..npy", "e..npy"]
    for (spk, fn), (fs, n) in wavs.items():
        mel = np.load(tmp_path / "spmel" / spk / MS.out_name(fn))
        assert mel.dtype == np.float32 and mel.shape == (A.n_frames(out_len(n, fs)), 80)
        assert np.isfinite(mel).all() and mel.max() > -5.0
