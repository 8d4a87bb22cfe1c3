"""The waveform -> log-mel path without a GPU: the fp64 restatement of tests/audio_ref.py against the
reference's own operator (torch.stft in fp64 + matmul), the closed-form invariants of the Slaney
filterbank for both the product's function and the restatement's, the frame-count formula, the ledger
of the third ABI header (include/autovc_hip_audio.h), the host refusals of avc_audio2mel on a machine
with no device, the compact filter table, and the bookkeeping of autoformer_amd.make_spec on wavs
written with the standard library.

The filterbank invariants pin the FORMULA (Slaney scale, triangles, 2 / (f[m+2] - f[m])), not
librosa's bits: neither librosa nor the reference's Audio2Mel runs where this suite does."""
import ast
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import audio_ref as R
from .conftest import ROOT

HEADER_AUDIO = os.path.join(ROOT, "include", "autovc_hip_audio.h")


# ----------------------------------------------------------------------- the restatement itself
def test_restatement_equals_the_reference_operator_in_fp64():
    """np.pad reflect + np.fft.rfft + matmul against F.pad reflect + torch.stft(center=False) + matmul,
    both fp64: largest difference over the frame's peak <= 1e-12 (3.6e-16 when this was written)."""
    basis = R.mel_basis(dtype=np.float64)
    win = torch.hann_window(1024, dtype=torch.float64)
    np.testing.assert_allclose(win.numpy(), R.hann_periodic(), rtol=0, atol=1e-15)
    worst = 0.0
    for name, x in R.signals().items():
        xt = torch.from_numpy(x.astype(np.float64))[None, None]
        padded = F.pad(xt, (R.PAD, R.PAD), "reflect").squeeze(1)
        spec = torch.stft(padded, n_fft=1024, hop_length=256, win_length=1024, window=win, center=False,
                          return_complex=True)
        mel_t = torch.matmul(torch.from_numpy(basis), spec.abs())[0].numpy().T  # (T, 80)
        mel_n = R.linear_mel(x, basis)
        assert mel_t.shape == mel_n.shape == (R.n_frames(x.shape[0]), 80), name
        peak = np.maximum(mel_t.max(axis=1), 1e-300)
        worst = max(worst, float((np.abs(mel_t - mel_n).max(axis=1) / peak).max()))
    print(f"restatement vs torch.stft fp64: {worst:.2e}")
    assert worst <= 1e-12


# ----------------------------------------------------------------------- the filterbank
def _bases():
    from autoformer_amd.melgan import slaney_mel_basis

    return {"product": slaney_mel_basis(22050, 1024, 80, 0.0, None), "restatement": R.mel_basis()}


@pytest.mark.parametrize("which", ["product", "restatement"])
def test_filterbank_closed_form_invariants(which):
    """Row sums: a unit-area triangle sampled every 22050/1024 Hz sums to 1 exactly only when its
    corners fall on bins.  The closed form that gives every other number below to 1e-7 has row sums
    times 22050/1024 between 0.9738 and 1.0369 (the narrow filters around the 1 kHz knee, 4 to 6
    bins wide), a mean of 1.00015 and a median deviation of 0.23 %; what is held here is the mean
    within 0.5 % and every row within 4 %."""
    W = _bases()[which]
    assert W.shape == (80, 513) and W.dtype == np.float32
    nz = W != 0
    assert nz.any(axis=1).all()                       # no empty filter
    assert nz.sum(axis=0).max() <= 2                  # a bin feeds at most two filters
    widths = [int(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1) for r in W]
    assert min(widths) == 3 and max(widths) == 41
    assert all(nz[m, np.flatnonzero(nz[m])[0]:np.flatnonzero(nz[m])[-1] + 1].all() for m in range(80))  # contiguous
    rel = 1e-7
    np.testing.assert_allclose(W[0, 1:4], [0.01276074, 0.02316559, 0.01040485], rtol=4 * rel)  # 8 printed digits
    assert W[0, 0] == 0
    np.testing.assert_allclose(W.max(), 0.024146901, rtol=rel)
    np.testing.assert_allclose(W[79].max(), 0.0022081186, rtol=rel)
    area = W.astype(np.float64).sum(axis=1) * 22050 / 1024
    assert abs(area.mean() - 1) < 5e-3 and np.abs(area - 1).max() < 4e-2


def test_mel_scale_and_the_two_filterbanks_agree():
    from autoformer_amd.melgan import hz_to_mel, mel_to_hz

    assert float(hz_to_mel(1000.0)) == 15.0 and R.hz_to_mel(1000.0) == 15.0
    assert abs(float(hz_to_mel(11025.0)) - 49.910594) < 1e-6 and abs(R.hz_to_mel(11025.0) - 49.910594) < 1e-6
    for hz in (0.0, 440.0, 999.0, 1000.0, 5000.0, 11025.0):
        assert abs(float(mel_to_hz(hz_to_mel(hz))) - hz) < 1e-9 and abs(R.mel_to_hz(R.hz_to_mel(hz)) - hz) < 1e-9
    b = _bases()
    np.testing.assert_allclose(b["product"], b["restatement"], rtol=1e-6, atol=1e-12)
    # free parameters only change the host table
    from autoformer_amd.melgan import slaney_mel_basis

    np.testing.assert_allclose(slaney_mel_basis(16000, 1024, 40, 90.0, 7600.0),
                               R.mel_basis(16000, 1024, 40, 90.0, 7600.0), rtol=1e-6, atol=1e-12)


def test_module_buffers_and_constructor():
    from autoformer_amd.melgan import Audio2Mel
    from melgan.modules import Audio2Mel as Shim

    assert Shim is Audio2Mel
    m = Audio2Mel()
    sd = m.state_dict()
    assert list(sd) == ["mel_basis", "window"]
    assert sd["mel_basis"].shape == (80, 513) and sd["mel_basis"].dtype == torch.float32
    assert sd["window"].shape == (1024,) and torch.equal(sd["window"], torch.hann_window(1024))
    assert (m.n_fft, m.hop_length, m.win_length, m.sampling_rate, m.n_mel_channels) == (1024, 256, 1024, 22050, 80)
    for kw in ({"n_fft": 2048}, {"hop_length": 128}, {"win_length": 512}, {"n_mel_channels": 129}):
        with pytest.raises(ValueError):
            Audio2Mel(**kw)
    other = Audio2Mel(sampling_rate=16000, n_mel_channels=40, mel_fmin=90.0, mel_fmax=7600.0)
    assert other.mel_basis.shape == (40, 513)


def test_frame_count_and_short_utterances():
    from autoformer_amd.melgan import Audio2Mel, n_frames

    for L, T in ((385, 1), (511, 1), (512, 2), (3 * 256 + 17, 3), (1000, 3), (4096, 16), (88200, 344), (8 * 256, 8)):
        assert n_frames(L) == T == R.n_frames(L) == (L + 2 * 384 - 1024) // 256 + 1
        assert R.magnitudes(np.zeros(L)).shape == (T, 513)
    assert Audio2Mel.n_frames(4096) == 16
    for L in (384, 100, 0):
        with pytest.raises(ValueError, match="too short"):
            n_frames(L)
    with pytest.raises(RuntimeError):   # the reference's own pad refuses the same lengths
        F.pad(torch.zeros(1, 1, 384), (384, 384), "reflect")


def test_compact_table_restores_the_basis_and_a_dense_basis_is_refused():
    from autoformer_amd import _lib
    from autoformer_amd.melgan import Audio2Mel, compact_basis

    m = Audio2Mel()
    W = m.mel_basis.numpy()
    table, weights = compact_basis(W)
    assert table.shape == (80, 3) and table.dtype == np.int32 and weights.dtype == np.float32
    assert 900 <= weights.size <= 1200 and weights.size == table[:, 1].sum()
    back = np.zeros_like(W)
    for mm, (st, cnt, off) in enumerate(table):
        back[mm, st:st + cnt] = weights[off:off + cnt]
    assert np.array_equal(back, W)
    # a filter with a hole keeps its interior zeros; an empty filter has count 0
    H = np.zeros((3, 513), dtype=np.float32)
    H[0, 5], H[0, 9] = 1.0, 2.0
    H[2, 512] = 3.0
    t2, w2 = compact_basis(H)
    assert t2.tolist() == [[5, 5, 0], [0, 0, 5], [512, 1, 5]] and w2.tolist() == [1, 0, 0, 0, 2, 3]
    # tables() is host work: cached per buffer version, rebuilt after a load_state_dict
    t_a = m.tables()
    assert m.tables() is t_a
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["mel_basis"][3] *= 2
    m.load_state_dict(sd)
    t_b = m.tables()
    assert t_b is not t_a and not torch.equal(t_a[2], t_b[2])
    dense = {"mel_basis": torch.ones(80, 513), "window": sd["window"]}
    m.load_state_dict(dense)
    with pytest.raises(ValueError, match="LDS budget"):
        m.tables()
    assert 80 * 513 > _lib.MEL_MAX_WEIGHTS


# ----------------------------------------------------------------------- the third header's ledger
A_ = "test_gpu_audio2mel.py::"
LEDGER_AUDIO = {
    "avc_audio2mel": [A_ + "test_signals_within_the_bar", A_ + "test_ragged_batch_in_one_launch",
                      A_ + "test_host_refusals_launch_nothing"],
}


def declared_symbols_audio():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_AUDIO).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_audio_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols
    from .test_metadv import declared_symbols_dv

    declared = declared_symbols_audio()
    assert len(declared) == 1 and set(declared) == set(LEDGER_AUDIO)
    assert set(declared) == set(_lib.exported_symbols_audio())
    assert not set(declared) & set(declared_symbols()) and not set(declared) & set(declared_symbols_dv())
    assert not set(declared) & set(_lib.exported_symbols()) and not set(declared) & set(_lib.exported_symbols_dv())
    assert len(_lib.exported_symbols_dv()) == 5      # the two earlier tables are as they were
    assert set(_lib.exported_symbols()) == set(declared_symbols())
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31   # added without an ABI bump
    assert "audio.hip" in _lib.SOURCES
    hdr = open(HEADER_AUDIO).read()
    assert int(re.search(r"#define AVC_MEL_MAX_WEIGHTS (\d+)", hdr).group(1)) == _lib.MEL_MAX_WEIGHTS
    assert int(re.search(r"#define AVC_MEL_FRAME_MAJOR (\d+)", hdr).group(1)) == _lib.MEL_FRAME_MAJOR
    assert int(re.search(r"#define AVC_MEL_CHANNEL_MAJOR (\d+)", hdr).group(1)) == _lib.MEL_CHANNEL_MAJOR
    cache = {}
    for sym, refs in LEDGER_AUDIO.items():
        assert refs, sym
        for ref in refs:
            fname, func = ref.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref)


def refusal_cases():
    """(what is wrong, keyword overrides of a valid call, a piece of the message).  Shared with the GPU
    file, which sends the same calls with real device pointers and checks that nothing is written."""
    return [
        ("null audio", {"audio": None}, b"null"),
        ("null lens", {"lens": None}, b"null"),
        ("null lens_dev", {"lens_dev": None}, b"null"),
        ("null window", {"window": None}, b"null"),
        ("null twiddle", {"twiddle": None}, b"null"),
        ("null filt", {"filt": None}, b"null"),
        ("null filt_dev", {"filt_dev": None}, b"null"),
        ("null weights", {"weights": None}, b"null"),
        ("null out", {"out": None}, b"null"),
        ("L = 384", {"lens_v": [4096, 384]}, b"lens[1] = 384"),
        ("L > stride", {"lens_v": [4097, 1000]}, b"exceeds the row stride"),
        ("Tmax too small", {"Tmax": 15}, b"16 frames, Tmax = 15"),
        ("n_mel 129", {"n_mel": 129}, b"n_mel = 129"),
        ("n_mel 0", {"n_mel": 0}, b"n_mel = 0"),
        ("layout 2", {"layout": 2}, b"unknown layout 2"),
        ("n_fft 2048", {"n_fft": 2048}, b"n_fft=2048"),
        ("win 512", {"win": 512}, b"win=512"),
        ("hop 128", {"hop": 128}, b"hop=128"),
        ("too many weights", {"n_weights": 8193}, b"LDS budget"),
        ("filter past the bins", {"filt_v": [510, 4, 0]}, b"filter 0"),
        ("filter past the weights", {"filt_v": [0, 4, 7]}, b"filter 0"),
        ("B = 0", {"B": 0}, b"bad shape"),
    ]


def call_audio2mel(Lb, ptrs, **over):
    """avc_audio2mel for two utterances of stride 4096 and two filters, with overrides; ptrs: name -> pointer."""
    from autoformer_amd import _lib

    a = dict(ptrs)
    lens_v = over.pop("lens_v", [4096, 1000])
    filt_v = over.pop("filt_v", [0, 4, 0]) + [4, 6, 4]
    a.update(lens=(_lib.c_int * 2)(*lens_v), filt=(_lib.c_int * 6)(*filt_v), B=2, n_weights=10, n_mel=2, n_fft=1024,
             win=1024, hop=256, Tmax=16, layout=0)
    a.update(over)
    return Lb.avc_audio2mel(a["audio"], 4096, a["lens"], a["lens_dev"], a.get("scale"), a["B"], a["window"],
                            a["twiddle"], a["filt"], a["filt_dev"], a["weights"], a["n_weights"], a["n_mel"],
                            a["n_fft"], a["win"], a["hop"], 1e-5, a["out"], a["Tmax"], a["layout"], None)


def test_audio_host_refusals_without_a_gpu():
    """Every argument check precedes the launch: each bad call comes back as an error, with its message,
    on a machine with no device.  The pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)
    ptrs = {k: p for k in ("audio", "lens_dev", "window", "twiddle", "filt_dev", "weights", "out")}
    for what, over, msg in refusal_cases():
        assert call_audio2mel(Lb, ptrs, **over) == -1, what
        assert msg in Lb.avc_last_error(), (what, Lb.avc_last_error())


# ----------------------------------------------------------------------- make_spec bookkeeping
def write_wav(path, x, fs=22050, width=2):
    """x float (N,) or (N, C) in [-1, 1) -> PCM wav; returns the quantised samples as read back by soundfile's rule."""
    x = np.asarray(x, dtype=np.float64)
    full = 32768.0 if width == 2 else 2147483648.0
    q = np.clip(np.round(x * full), -full, full - 1).astype("<i2" if width == 2 else "<i4")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if q.ndim == 1 else q.shape[1])
        w.setsampwidth(width)
        w.setframerate(fs)
        w.writeframes(q.tobytes())
    return (q.astype(np.float64) / full).astype(np.float32)


def test_make_spec_reads_wavs():
    from autoformer_amd import make_spec as MS

    rng = np.random.RandomState(3)
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        mono = write_wav(os.path.join(d, "m.wav"), 0.3 * rng.randn(700).clip(-3, 3))
        x, fs = MS.read_wav(os.path.join(d, "m.wav"))
        assert fs == 22050 and x.dtype == np.float32 and np.array_equal(x, mono)
        assert MS.wav_info(os.path.join(d, "m.wav")) == (700, 22050)
        st = write_wav(os.path.join(d, "s.wav"), 0.3 * rng.randn(500, 2).clip(-3, 3))
        x, fs = MS.read_wav(os.path.join(d, "s.wav"))
        assert x.shape == (500, 2) and np.array_equal(MS.first_channel(x), st[:, 0])
        w32 = write_wav(os.path.join(d, "w.wav"), 0.3 * rng.randn(400).clip(-3, 3), width=4)
        x, _ = MS.read_wav(os.path.join(d, "w.wav"))
        assert np.array_equal(x, w32)
        with wave.open(os.path.join(d, "b.wav"), "wb") as w:
            w.setnchannels(1), w.setsampwidth(1), w.setframerate(22050), w.writeframes(bytes(500))
        with pytest.raises(ValueError, match="16- or 32-bit"):
            MS.read_wav(os.path.join(d, "b.wav"))
    with pytest.raises(ValueError, match="16000 Hz"):
        MS.wav_to_mel(np.zeros(1000, dtype=np.float32), 16000, a2m=object())
    assert MS.out_name("p225_001.wav") == "p225_001..npy"   # np.save("p225_001.") of the notebook


def test_make_spec_tree_names_and_length_batching(tmp_path):
    """The walk, the refusal by name, the output names and the batching, with the kernel call replaced
    by a recorder (the mels themselves are the GPU file's business)."""
    from autoformer_amd import make_spec as MS

    assert MS.plan_batches([500, 400, 900, 400, 700], 2) == [[1, 3], [0, 4], [2]]
    assert MS.plan_batches([], 4) == [] and MS.plan_batches([5], 1) == [[0]]
    with pytest.raises(ValueError):
        MS.plan_batches([5], 0)
    rng = np.random.RandomState(5)
    wavs = {("spkB", "u2.wav"): 900, ("spkB", "u1.wav"): 500, ("spkA", "x.wav"): 700, ("spkA", "a.wav"): 400,
            ("spkA", "st.wav"): 600}
    data = {}
    for (spk, fn), n in wavs.items():
        os.makedirs(tmp_path / "wav" / spk, exist_ok=True)
        x = 0.2 * rng.randn(n, 2 if fn == "st.wav" else 1).clip(-3, 3)
        q = write_wav(tmp_path / "wav" / spk / fn, x if fn == "st.wav" else x[:, 0])
        data[(spk, fn)] = q[:, 0] if q.ndim > 1 else q
    (tmp_path / "wav" / "spkA" / "notes.txt").write_text("not a wav")
    (tmp_path / "wav" / "stray.wav").write_bytes(b"")       # not under a speaker: not walked
    assert MS.list_wavs(str(tmp_path / "wav")) == [("spkA", "a.wav"), ("spkA", "st.wav"), ("spkA", "x.wav"),
                                                   ("spkB", "u1.wav"), ("spkB", "u2.wav")]
    calls = []

    def recorder(a2m, waves):
        calls.append([w.copy() for w in waves])
        return [np.full((MS.n_frames(len(w)), 80), float(len(w)), dtype=np.float32) for w in waves]

    out = tmp_path / "spmel"
    written = MS.convert_tree(str(tmp_path / "wav"), str(out), max_batch=2, a2m=object(), mels_fn=recorder)
    assert [os.path.relpath(p, out) for p in written] == ["spkA/a..npy", "spkA/st..npy", "spkA/x..npy",
                                                          "spkB/u1..npy", "spkB/u2..npy"]
    assert [[len(w) for w in c] for c in calls] == [[400, 500], [600, 700], [900]]   # sorted by length, two to a launch
    assert np.array_equal(calls[1][0], data[("spkA", "st.wav")])                     # first channel of the stereo file
    assert np.array_equal(calls[0][1], data[("spkB", "u1.wav")])
    for p, n in zip(written, (400, 600, 700, 500, 900)):
        m = np.load(p)
        assert m.dtype == np.float32 and m.shape == (MS.n_frames(n), 80) and (m == n).all()
    # what embed.build_metadata and data.py list: <speaker>/*.npy
    assert sorted(f for f in os.listdir(out / "spkA") if f.endswith(".npy")) == ["a..npy", "st..npy", "x..npy"]
    # a wrong rate or a too-short file is refused by name before anything is written
    write_wav(tmp_path / "wav" / "spkB" / "u0.wav", np.zeros(600), fs=16000)
    with pytest.raises(ValueError, match=r"spkB/u0\.wav.*16000 Hz"):
        MS.convert_tree(str(tmp_path / "wav"), str(tmp_path / "o2"), a2m=object(), mels_fn=recorder)
    assert not os.path.exists(tmp_path / "o2")
    write_wav(tmp_path / "wav" / "spkB" / "u0.wav", np.zeros(300))
    with pytest.raises(ValueError, match=r"spkB/u0\.wav.*too short"):
        MS.convert_tree(str(tmp_path / "wav"), str(tmp_path / "o2"), a2m=object(), mels_fn=recorder)


def test_peak_normalisation_rule():
    x = np.array([0.1, -0.4, 0.2])
    np.testing.assert_allclose(R.peak_normalise(x), x / 0.4)
    assert np.array_equal(R.peak_normalise(np.zeros(4)), np.zeros(4))
