"""The vocoder over ragged batches, the host side (no GPU): the ledger of the eighth ABI header
(include/autovc_hip_vocoder.h), its refusals (every check precedes the launch), the planning with freq = 1,
the refusals of short utterances, and the wiring of the wav-to-wav CLI and of evaluate.export_grid_wavs with a
stub vocoder that records the batches it is given."""
import ast
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch

from .conftest import ROOT

HEADER_VOCODER = os.path.join(ROOT, "include", "autovc_hip_vocoder.h")
G_ = "test_gpu_vocoder_ragged.py::"
C_ = "test_vocoder_ragged.py::test_vocoder_host_refusals_without_a_gpu"
LEDGER_VOCODER = {
    "avc_mg_gather_ragged": [G_ + "test_gather_against_fp64", G_ + "test_gather_full_lengths_match_the_rectangular_form",
                             G_ + "test_refusals_launch_nothing", C_],
    "avc_mg_act_ragged": [G_ + "test_act_against_fp64", G_ + "test_refusals_launch_nothing", C_],
    "avc_mg_conv_out_ragged": [G_ + "test_conv_out_against_fp64", G_ + "test_refusals_launch_nothing", C_],
}


def declared_symbols_vocoder():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_VOCODER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


# ----------------------------------------------------------------------- the eighth header's ledger
def test_vocoder_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    declared = declared_symbols_vocoder()
    assert set(declared) == set(LEDGER_VOCODER) == set(_lib.exported_symbols_vocoder())
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg()
               + _lib.exported_symbols_ragged())
    assert not set(declared) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]                     # every declared symbol is built
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "melgan_ragged.hip" in _lib.SOURCES
    cache = {}
    for sym, refs in LEDGER_VOCODER.items():
        for ref_ in refs:
            fname, func = ref_.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref_)


def test_vocoder_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)
    ok, long_, zero = (ctypes.c_int * 2)(5, 8), (ctypes.c_int * 2)(9, 8), (ctypes.c_int * 2)(5, 0)
    small = (ctypes.c_int * 2)(8, 1)

    def err():
        return Lb.avc_last_error().decode()

    def gather(x=p, lens=ok, ldev=p, B=2, T=8, C=80, taps=7, dil=1, pad=3, scale=1, out=p, xdt=_lib.F32, odt=_lib.BF16):
        return Lb.avc_mg_gather_ragged(x, xdt, B, T, C, taps, dil, pad, 1, 0.2, lens, ldev, scale, out, odt, None)

    def act(x=p, lens=ok, ldev=p, B=2, T=8, C=80, scale=1, out=p, out16=None):
        return Lb.avc_mg_act_ragged(x, B, T, C, 0.2, lens, ldev, scale, out, out16, None)

    def conv(x=p, lens=ok, ldev=p, B=2, T=8, C=32, scale=1, out=p, taps=7, w=p, bias=p):
        return Lb.avc_mg_conv_out_ragged(x, B, T, C, taps, w, bias, 0.2, lens, ldev, scale, out, None)

    for fn, name in ((gather, "avc_mg_gather_ragged"), (act, "avc_mg_act_ragged"), (conv, "avc_mg_conv_out_ragged")):
        assert fn(lens=long_) != 0 and name + ": lens[0] = 9 outside 1..Tmax = 8" in err()     # a length above Tmax
        assert fn(lens=zero) != 0 and name + ": lens[1] = 0 outside 1..Tmax = 8" in err()
        assert fn(C=82) != 0 and name + ": C = 82 must be a positive multiple of 4" in err()   # C % 4 != 0
        assert fn(C=0) != 0 and "multiple of 4" in err()
        assert fn(x=None) != 0 and name + ": null pointer" in err()                            # a null pointer
        assert fn(out=None) != 0 and "null pointer" in err()
        assert fn(lens=None) != 0 and "null pointer" in err()
        assert fn(ldev=None) != 0 and "null pointer" in err()
        assert fn(B=0) != 0 and fn(B=65536) != 0 and "B = 65536" in err()
        assert fn(T=0) != 0 and fn(scale=0) != 0 and "scale = 0" in err()
        assert fn(T=1 << 20, scale=1 << 11) != 0 and "exceed 2^30" in err()
        assert fn(x=ctypes.c_void_p(260)) != 0 and "aligned to 4 elements" in err()
    # pad >= lens[b]*scale
    assert gather(lens=small, taps=3, dil=9, pad=9, scale=8) != 0
    assert "avc_mg_gather_ragged: reflection pad 9 needs more than pad rows, lens[1]*scale = 8" in err()
    assert gather(lens=(ctypes.c_int * 2)(3, 8)) != 0 and "reflection pad 3" in err() and "lens[0]*scale = 3" in err()
    assert gather(taps=3, dil=2, pad=1) != 0 and "keeps the length" in err()
    assert gather(taps=0, pad=0) != 0 and gather(dil=0, pad=0) != 0
    assert gather(xdt=5) != 0 and "unknown dtype" in err()
    assert gather(out=ctypes.c_void_p(260), odt=_lib.BF16) != 0 and "aligned" in err()         # bf16: 8 bytes
    assert act(out=None, out16=None) != 0 and "neither out nor out_bf16" in err()
    assert conv(lens=(ctypes.c_int * 2)(3, 8)) != 0 and "reflection pad 3" in err()
    assert conv(lens=small, scale=3) != 0 and "lens[1]*scale = 3" in err()
    assert conv(taps=5) != 0 and "taps = 5" in err()
    assert conv(w=None) != 0 and conv(bias=None) != 0 and "null pointer" in err()


# ----------------------------------------------------------------------- planning with freq = 1
def test_plan_with_freq_one_keeps_lengths_and_cuts():
    from autoformer_amd.convert import padded_len, plan_whole
    from autoformer_amd.melgan import VOCODER_MAX_BATCH, VOCODER_MAX_FRAMES

    assert [padded_len(T, 1) for T in (4, 21, 37, 633)] == [4, 21, 37, 633]                    # no rounding
    lens = [21, 4, 37, 9, 21]
    assert plan_whole(lens, 1, 2, 8192) == [([1, 3], 9), ([0, 4], 21), ([2], 37)]              # B <= max_batch
    assert plan_whole(lens, 1, 64, 8192) == [([1, 3, 0, 4, 2], 37)]
    assert plan_whole(lens, 1, 64, 63) == [([1, 3, 0], 21), ([4], 21), ([2], 37)]              # B * Tmax <= max_frames
    assert plan_whole(lens, 1, 64, 20) == [([1, 3], 9), ([0], 21), ([4], 21), ([2], 37)]       # over budget: alone
    rng = np.random.RandomState(3)
    many = [int(v) for v in rng.randint(4, 700, size=64)]
    plan = plan_whole(many, 1, VOCODER_MAX_BATCH, VOCODER_MAX_FRAMES)
    assert sorted(i for idx, _ in plan for i in idx) == list(range(64))
    for idx, Tmax in plan:
        assert Tmax == max(many[i] for i in idx) and len(idx) <= VOCODER_MAX_BATCH
        assert len(idx) * Tmax <= VOCODER_MAX_FRAMES
    # the default budget: the live set of the generator, 224 KiB per mel frame (melgan.py), stays at a few GB
    assert (VOCODER_MAX_BATCH, VOCODER_MAX_FRAMES) == (32, 8192) and VOCODER_MAX_FRAMES * 224 * 1024 <= 2 << 30


def test_short_utterances_are_refused_before_any_launch():
    """On the CPU: the refusal comes before a device is touched."""
    from autoformer_amd.convert import convert_whole
    from autoformer_amd.factory.AutoVC import AutoVC
    from autoformer_amd.melgan import Generator, MelVocoder

    voc = MelVocoder(device="cpu", generator=Generator(80, 32, 3))
    good, bad = np.zeros((9, 80), np.float32), np.zeros((3, 80), np.float32)
    with pytest.raises(ValueError, match=r"mels\[1\] has 3 frames"):
        voc.inverse_ragged([good, bad])
    with pytest.raises(ValueError, match="must be"):
        voc.inverse_ragged([np.zeros((9, 81), np.float32)])
    assert voc.inverse_ragged([]) == []
    e = np.zeros(256, np.float32)
    with pytest.raises(ValueError, match="fewer than 4 frames"):
        convert_whole(AutoVC(44, 256, 512, 22), [good, bad], e, e, vocoder=voc)


# ----------------------------------------------------------------------- export_grid_wavs
class StubVocoder:
    """Records what it is given; a wav is its mel's first column repeated 256 times, scaled into [-1, 1]."""
    device = "cpu"

    def __init__(self):
        self.ragged, self.rect = [], []

    @staticmethod
    def _wav(mel):
        return torch.as_tensor(np.asarray(mel)[:, 0]).float().repeat_interleave(256) / 100.0

    def inverse_ragged(self, mels, max_batch=None, max_frames=None):
        self.ragged.append(([tuple(m.shape) for m in mels], max_batch))
        return [self._wav(m) for m in mels]

    def inverse_frames(self, x):
        self.rect.append(tuple(x.shape))
        return torch.stack([self._wav(m) for m in x])


def _read(path):
    with wave.open(path, "rb") as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (22050, 1, 2)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def test_export_grid_wavs_whole_goes_through_inverse_ragged(tmp_path):
    from autoformer_amd.evaluate import export_grid_wavs

    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    lens = [12, 12, 7, 7]
    mels = [np.full((T, 80), 10.0 * (i + 1), np.float32) for i, T in enumerate(lens)]
    voc = StubVocoder()
    written = export_grid_wavs(voc, mels, [0] * 4, pairs, ["spkA", "spkB"], str(tmp_path), None, max_batch=3)
    assert voc.rect == [] and voc.ragged == [([(12, 80), (12, 80), (7, 80), (7, 80)], 3)]      # all pairs, input order
    assert [os.path.relpath(p, tmp_path) for p in written] == ["spkA/0_0.wav", "spkA/0_1.wav", "spkB/1_0.wav",
                                                               "spkB/1_1.wav"]
    for i, p in enumerate(written):
        pcm = _read(p)
        assert pcm.shape == (lens[i] * 256,) and abs(int(pcm[0]) - round(0.1 * (i + 1) * 32767)) <= 1   # pair i's own wav


def test_export_grid_wavs_len_crop_still_groups_by_equal_length(tmp_path):
    from autoformer_amd.evaluate import export_grid_wavs

    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    pads = [0, 4, 0, 4, 0]
    mels = [np.full((16, 80), 10.0 * (i + 1), np.float32) for i in range(5)]
    voc = StubVocoder()
    written = export_grid_wavs(voc, mels, pads, pairs, ["a", "b", "c"], str(tmp_path), 16, max_batch=2)
    assert voc.ragged == [] and voc.rect == [(2, 12, 80), (2, 16, 80), (1, 16, 80)]
    assert sorted(os.path.relpath(p, tmp_path) for p in written) == ["a/0_0.wav", "a/0_1.wav", "b/1_0.wav", "b/1_1.wav",
                                                                     "c/2_0.wav"]
    for i, (s, t) in enumerate(pairs):
        pcm = _read(os.path.join(tmp_path, "abc"[s], f"{s}_{t}.wav"))
        assert pcm.shape == ((16 - pads[i]) * 256,) and abs(int(pcm[0]) - round(0.1 * (i + 1) * 32767)) <= 1


# ----------------------------------------------------------------------- the wav-to-wav CLI
def test_cli_hands_the_vocoder_to_convert_whole(tmp_path, monkeypatch):
    """main() with everything that needs a device replaced: convert_whole receives the vocoder, and the wavs it
    returns are written under the sources' names, in input order."""
    import autoformer_amd as A
    from autoformer_amd import convert as Cv
    from autoformer_amd import embed, evaluate, melgan

    seen = {}

    class Model:
        def train(self):
            return self

        def eval(self):
            return self

    class Voc:
        def __init__(self, device=None, generator=None):
            seen["voc_device"] = device

    class A2M:
        def to(self, device):
            return self

    def fake_convert_whole(model, mels, e_org, e_trg, max_batch=64, max_frames=None, device=None, vocoder=None):
        seen["call"] = (len(mels), max_batch, device, type(vocoder).__name__)
        return ([np.full((T, 80), i, np.float32) for i, T in enumerate((5, 9))],
                [np.full(T * 256, 0.1 * (i + 1), np.float32) for i, T in enumerate((5, 9))])

    monkeypatch.setattr(evaluate, "_load_module", lambda *a: Model())
    monkeypatch.setattr(Cv, "whole_family", lambda m: None)
    monkeypatch.setattr(melgan, "MelVocoder", Voc)
    monkeypatch.setattr(melgan, "Audio2Mel", A2M)
    monkeypatch.setattr(Cv, "_wav_mels", lambda paths, a2m, device, resample: [np.zeros((6, 80), np.float32)] * len(paths))
    monkeypatch.setattr(embed, "speaker_dvector", lambda emb, mels: np.zeros(256, np.float32))
    monkeypatch.setattr(Cv, "convert_whole", fake_convert_whole)
    out = tmp_path / "out"
    try:
        rc = Cv.main(["--src", "x/b.wav", "y/a.wav", "--ref", "t.wav", "--out_dir", str(out), "--det_init",
                      "--max_batch", "7", "--save_mel"])
    finally:
        A.set_compute("bf16")
    assert rc == 0 and seen["call"] == (2, 7, "cuda:0", "Voc") and seen["voc_device"] == "cuda:0"
    assert sorted(os.listdir(out)) == ["a.npy", "a.wav", "b.npy", "b.wav"]
    for name, i, T in (("b", 0, 5), ("a", 1, 9)):                         # input order, not sorted names
        pcm = _read(str(out / (name + ".wav")))
        assert pcm.shape == (T * 256,) and abs(int(pcm[0]) - round(0.1 * (i + 1) * 32767)) <= 1
        assert np.load(str(out / (name + ".npy"))).shape == (T, 80)
