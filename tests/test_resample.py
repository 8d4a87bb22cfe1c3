"""The sample-rate converter without a GPU: the fp64 restatement of tests/resample_ref.py against the
continuous Kaiser-windowed sinc, the quirk kept at 48000 -> 22050, the product's polyphase table against
the restatement, impulses, output lengths, the ledger of the fourth ABI header
(include/autovc_hip_resample.h), the host refusals of avc_resample on a machine with no device, and the
bookkeeping of autoformer_amd.make_spec with resampling switched on.

Neither librosa nor resampy runs where this suite does: what is pinned is the FORMULA of resampy's
kaiser_best interpolator as tests/resample_ref.py states it, not a library's bits."""
import ast
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from . import resample_ref as R
from .conftest import ROOT
from .test_audio import write_wav

HEADER_RESAMPLE = os.path.join(ROOT, "include", "autovc_hip_resample.h")
RATES = (48000, 16000, 44100, 96000)
LENGTHS = (1, 100, 320, 321, 5000)
# rate -> (L, M, step, taps, weights): the table of DESIGN §7, re-derived by test_table_shapes below
SHAPES = {48000: (147, 320, 235, 277, 40719), 16000: (441, 320, 512, 127, 56007), 44100: (1, 2, 256, 255, 255),
          96000: (147, 640, 117, 559, 82173)}


def apply_table(tb, x, dtype=np.float64):
    """The product's polyphase table applied on the CPU in `dtype`, taps ascending (the kernel's order;
    a product rounded to dtype, then the add).  Vectorised over the outputs, sequential over the taps."""
    x = np.asarray(x, dtype=dtype)
    N = x.shape[0]
    W = tb.weights64 if dtype == np.float64 else tb.weights
    assert W.dtype == dtype
    nv = N * tb.L // tb.M
    y = np.zeros(-((-N * tb.L) // tb.M), dtype=dtype)
    j, r = np.divmod(np.arange(nv), tb.L)
    off, first, cnt = (tb.table[r, c].astype(np.int64) for c in range(3))
    acc = np.zeros(nv, dtype=dtype)
    for k in range(tb.taps):
        g = j * tb.M + off + k
        ok = (k >= first) & (k < first + cnt) & (g >= 0) & (g < N)
        acc = acc + W[k, r] * np.where(ok, x[np.clip(g, 0, N - 1)], dtype(0))
    y[:nv] = acc
    assert y.dtype == dtype
    return y


@functools.lru_cache(maxsize=None)
def ref(name, N, fs):
    """fp64 restatement of signal `name` of N samples at fs -> 22050 Hz; computed once, never modified."""
    y = R.resample(R.signals(N, fs)[name], fs, 22050)
    y.setflags(write=False)
    return y


def rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ----------------------------------------------------------------------- the restatement itself
def interpolation_bound(fs):
    """Linear interpolation between table entries d = 1/512 apart errs by at most max|h''| d^2 / 8 per tap;
    |h''| d^2 on a cell is read off the table as the larger second difference at its two ends.  Summed
    over the taps of the worst phase (every offset 0..step-1 of both wings), per unit of max|x|."""
    win, _ = R.half_table()
    L, M, scale, step = R.setup(fs, 22050)
    d2 = np.zeros(R.NWIN + 1)
    d2[1:R.NWIN - 1] = np.abs(win[2:] - 2.0 * win[1:-1] + win[:-2])
    d2[0] = np.abs(2.0 * win[1] - 2.0 * win[0])          # h is even
    cell = np.maximum(d2[:-1], d2[1:]) / 8.0
    wing = max(cell[off::step].sum() for off in range(step))
    return 2.0 * wing * scale


@pytest.mark.parametrize("fs", [16000, 44100, 8000])
def test_restatement_against_the_closed_form(fs):
    """Where scale * 512 is an integer the table form is the continuous Kaiser-windowed sinc (np.i0) sampled
    with linear interpolation, and nothing else.  Bar: the interpolation bound above times max|x|, times a
    margin of 1.5 for |h''| between the two ends of a cell and the wing's dropped last tap (|h| < 3e-8).
    Derived bound / measured, both as a fraction of the output's peak, on 600 samples of noise:
        16000: 1.08e-05 / 1.64e-06     44100: 1.16e-05 / 1.6e-08     8000: 1.03e-05 / 1.85e-06
    (the bound adds absolute values tap by tap; the errors of neighbouring taps alternate in sign)."""
    x = R.signals(600, fs)["noise"].astype(np.float64)
    table, closed = R.resample(x, fs, 22050), R.closed_form(x, fs, 22050)
    peak = np.abs(closed).max()
    bound = 1.5 * interpolation_bound(fs) * np.abs(x).max() / peak
    e = float(np.abs(table - closed).max() / peak)
    print(f"{fs}: table form vs closed form {e:.3e} of peak, bound {bound:.3e}")
    assert 0 < bound < 1e-4 and e <= bound


def test_kept_quirk_at_48000():
    """step = int(0.459375 * 512) = 235, not 235.2: the filter is stretched by 235.2 / 235 and the interior
    DC gain is 1.0004706 .. 1.0005004 over the 147 phases (measured on the restatement) instead of 1.
    Band: that interval widened by 1e-5 on each side; it must not contain 1.0, and 16000 -> 22050, whose
    step is exact, must be within 1e-5 of 1."""
    L, M, scale, step = R.setup(48000, 22050)
    assert (L, M, step) == (147, 320, 235) and scale * 512 == 235.2
    y = R.resample(np.ones(2000), 48000, 22050)
    mid = y[294:294 + 2 * 147]               # wings of 139 inputs = 64 outputs are inside [0, N)
    print(f"48000 -> 22050 DC gain {mid.min():.7f} .. {mid.max():.7f}")
    lo, hi = 1.0004706 - 1e-5, 1.0005004 + 1e-5
    assert lo > 1.0 and lo <= mid.min() and mid.max() <= hi
    assert len(np.unique(np.round(mid[:147], 12))) > 50          # it varies with the phase
    y16 = R.resample(np.ones(600), 16000, 22050)
    assert np.abs(y16[300:500] - 1.0).max() < 1e-5
    # the continuous filter at the un-truncated step differs visibly: 2.4e-3 of peak on noise
    from autoformer_amd.resample import resample_table

    assert resample_table(48000).step == 235


# ----------------------------------------------------------------------- the product's table
@pytest.mark.parametrize("fs", RATES)
def test_table_shapes(fs):
    from autoformer_amd import _lib
    from autoformer_amd.resample import rate_pair, resample_table

    tb = resample_table(fs)
    L, M, step, taps, nw = SHAPES[fs]
    assert (tb.L, tb.M, tb.step, tb.taps, tb.n_weights) == (L, M, step, taps, nw) and rate_pair(fs) == (L, M)
    assert R.setup(fs, 22050)[:2] == (L, M) and R.setup(fs, 22050)[3] == step
    assert tb.weights.shape == (taps, L) and tb.weights.dtype == np.float32 and tb.weights64.dtype == np.float64
    assert np.array_equal(tb.weights, tb.weights64.astype(np.float32))     # rounded once
    assert tb.table.shape == (L, 3) and tb.table.dtype == np.int32
    assert (tb.table[:, 1] == 0).all() and tb.table[:, 2].max() == taps and tb.table[:, 2].min() >= taps - 1
    for r in range(L):                                                     # zero padded past a residue's count
        assert not tb.weights64[tb.table[r, 2]:, r].any()
    assert nw <= _lib.RESAMPLE_MAX_WEIGHTS
    assert resample_table(fs) is tb                                        # built once per pair
    # the wings: (32769 - off) // step taps each
    assert taps == R.NWIN // step + (R.NWIN - step) // step


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("N", LENGTHS)
def test_product_table_equals_the_restatement(fs, N):
    """The polyphase table applied in fp64 == the per-output walk over the half table, <= 1e-12 of peak
    (1.9e-15 at most when this was written): N = 100 is shorter than one wing (139 inputs at 48000),
    N = 320 is the case N L / M = 147 exactly (no pad sample), N = 1 gives one output from one tap."""
    from autoformer_amd.resample import out_len, resample_table

    tb = resample_table(fs)
    want = ref("noise", N, fs)
    got = apply_table(tb, R.signals(N, fs)["noise"], np.float64)
    assert got.shape == want.shape == (out_len(N, fs),) == (R.out_len(N, fs, 22050),)
    e = rel(got, want)
    print(f"{fs} N={N}: table vs restatement {e:.2e}")
    assert e <= 1e-12
    padded = (N * tb.L) % tb.M != 0
    assert (want[-1] == 0.0 and got[-1] == 0.0) if padded else (want[-1] != 0.0 and got[-1] != 0.0)
    if padded and len(want) > 1:
        assert want[-2] != 0.0 and got[-2] != 0.0


def test_out_len_and_the_pad_sample():
    from autoformer_amd.resample import Resample, out_len

    assert [out_len(n, 48000) for n in LENGTHS] == [1, 46, 147, 148, 2297]
    assert [out_len(n, 16000) for n in LENGTHS] == [2, 138, 441, 443, 6891]
    assert [out_len(n, 44100) for n in LENGTHS] == [1, 50, 160, 161, 2500]
    assert out_len(192000, 48000) == 88200 and out_len(777, 22050) == 777
    assert Resample(48000).out_len(321) == 148
    for fs in RATES:
        for n in LENGTHS:
            assert out_len(n, fs) == R.out_len(n, fs, 22050) == int(np.ceil(n * 22050 / fs))
    y = ref("noise", 320, 48000)               # 320 * 147 / 320 = 147 exactly: nothing is padded
    assert len(y) == 147 and y[-1] != 0.0
    y = ref("noise", 321, 48000)               # floor = 147, ceil = 148: the last sample is the pad
    assert len(y) == 148 and y[-1] == 0.0 and y[-2] != 0.0


@pytest.mark.parametrize("fs", [48000, 16000, 44100])
def test_impulses_reproduce_the_filter_columns(fs):
    """x = unit impulse at m: y[j L + r] is exactly the one weight W[k, r] with j M + offset_r + k = m, or 0
    outside the residue's taps -- at sample 0, N - 1 and the middle, from the restatement (which has no
    such table).  What an off-by-one costs, measured on the restatement with 1000 samples of noise, as a
    fraction of the output's peak: the input moved by one sample 0.70 (48000), 1.68 (16000), 0.81 (44100);
    the output moved by one sample 1.31, 1.41, 1.31.  The GPU bar (about 1e-6) sits six orders under."""
    from autoformer_amd.resample import resample_table

    tb = resample_table(fs)
    N = 700
    for name, m in (("imp_first", 0), ("imp_last", N - 1), ("imp_mid", N // 2)):
        y = ref(name, N, fs)
        nv = N * tb.L // tb.M
        j, r = np.divmod(np.arange(nv), tb.L)
        k = m - j * tb.M - tb.table[r, 0]
        inside = (k >= 0) & (k < tb.table[r, 2])
        want = np.where(inside, tb.weights64[np.clip(k, 0, tb.taps - 1), r], 0.0)
        assert np.abs(y[:nv] - want).max() <= 1e-15 and not y[nv:].any(), name
    x = R.signals(1000, fs)["noise"].astype(np.float64)
    y = R.resample(x, fs, 22050)
    moved = R.resample(np.concatenate(([0.0], x[:-1])), fs, 22050)
    shift_in, shift_out = rel(moved, y), rel(y[:-2], y[1:-1])
    print(f"{fs}: input off by one {shift_in:.2f} of peak, output off by one {shift_out:.2f}")
    assert shift_in > 0.5 and shift_out > 0.5


# ----------------------------------------------------------------------- the fourth header's ledger
G_ = "test_gpu_resample.py::"
LEDGER_RESAMPLE = {
    "avc_resample": [G_ + "test_kernel_within_the_bar", G_ + "test_ragged_batch_in_one_launch",
                     "test_resample.py::test_resample_host_refusals_without_a_gpu"],
    "avc_resample_tile": [G_ + "test_kernel_within_the_bar", "test_resample.py::test_tile_is_host_arithmetic"],
}


def declared_symbols_resample():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_RESAMPLE).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avc_[a-z0-9_]+)\s*\(", src)))


def test_resample_header_ledger():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols
    from .test_audio import declared_symbols_audio
    from .test_metadv import declared_symbols_dv

    declared = declared_symbols_resample()
    assert set(declared) == set(LEDGER_RESAMPLE) == set(_lib.exported_symbols_resample())
    others = [(_lib.exported_symbols(), declared_symbols()), (_lib.exported_symbols_dv(), declared_symbols_dv()),
              (_lib.exported_symbols_audio(), declared_symbols_audio())]
    for table, header in others:
        assert not set(declared) & set(table) and not set(declared) & set(header)
        assert set(table) == set(header)                              # the three earlier tables are as they were
    assert len(_lib.exported_symbols_dv()) == 5 and len(_lib.exported_symbols_audio()) == 1
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in declared if not hasattr(so, s)]
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31   # added without an ABI bump
    assert "resample.hip" in _lib.SOURCES
    hdr = open(HEADER_RESAMPLE).read()
    assert int(re.search(r"#define AVC_RESAMPLE_MAX_WEIGHTS (\d+)", hdr).group(1)) == _lib.RESAMPLE_MAX_WEIGHTS
    cache = {}
    for sym, refs in LEDGER_RESAMPLE.items():
        assert refs, sym
        for ref_ in refs:
            fname, func = ref_.split("::")
            if fname not in cache:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert func.startswith("test_") and func in cache[fname], (sym, ref_)


def test_tile_is_host_arithmetic():
    """avc_resample_tile: a multiple of L whose input span fits the kernel's 12288 floats of LDS."""
    from autoformer_amd import _lib
    from autoformer_amd.resample import resample_table

    Lb = _lib.lib()
    for fs in RATES + (8000,):
        tb = resample_table(fs)
        tile = tb.tile()
        assert tile == Lb.avc_resample_tile(tb.L, tb.M, tb.taps) and tile >= 4 * tb.L and tile % (4 * tb.L) == 0
        assert tile // tb.L * tb.M + tb.taps <= 12288
    assert Lb.avc_resample_tile(147, 4000, 277) == -1 and b"LDS budget" in Lb.avc_last_error()
    assert Lb.avc_resample_tile(0, 1, 5) == -1 and b"at least 1" in Lb.avc_last_error()


# ----------------------------------------------------------------------- host refusals, no device
def refusal_cases():
    """(what is wrong, keyword overrides of a valid call, a piece of the message).  Shared with the GPU
    file, which sends the same calls with real device pointers and checks that nothing is written."""
    return [
        ("null x", {"x": None}, b"null"),
        ("null lens", {"lens": None}, b"null"),
        ("null lens_dev", {"lens_dev": None}, b"null"),
        ("null weights", {"weights": None}, b"null"),
        ("null tab", {"tab": None}, b"null"),
        ("null tab_dev", {"tab_dev": None}, b"null"),
        ("null out", {"out": None}, b"null"),
        ("N = 0", {"lens_v": [5000, 0]}, b"lens[1] = 0"),
        ("N < 0", {"lens_v": [-3, 100]}, b"lens[0] = -3"),
        ("N > stride", {"lens_v": [5001, 100]}, b"exceeds the row stride"),
        ("short out_stride", {"out_stride": 2296}, b"gives 2297 samples, out_stride = 2296"),
        ("L = 0", {"L": 0}, b"at least 1"),
        ("M = 0", {"M": 0}, b"at least 1"),
        ("taps = 0", {"taps": 0, "n_weights": 0}, b"taps = 0"),
        ("over-cap table", {"taps": 900, "n_weights": 900 * 147}, b"AVC_RESAMPLE_MAX_WEIGHTS"),
        ("n_weights off", {"n_weights": 40718}, b"expected taps * L"),
        ("B = 0", {"B": 0}, b"bad shape"),
        ("count past the taps", {"tab_v": [-138, 0, 278]}, b"residue 0"),
        ("negative first tap", {"tab_v": [-138, -1, 277]}, b"residue 0"),
        ("offsets apart", {"tab_v": [-5000, 0, 277]}, b"more than M + taps"),
        ("no tile fits", {"M": 4000}, b"LDS budget"),
    ]


def call_resample(Lb, ptrs, **over):
    """avc_resample for two utterances of stride 5000 at 48000 -> 22050, with overrides; ptrs: name -> pointer."""
    from autoformer_amd import _lib
    from autoformer_amd.resample import resample_table

    tb = resample_table(48000)
    a = dict(ptrs)
    tab = [int(v) for v in tb.table.reshape(-1)]
    tab[:3] = over.pop("tab_v", tab[:3])
    a.update(lens=(_lib.c_int * 2)(*over.pop("lens_v", [5000, 100])), tab=(_lib.c_int * len(tab))(*tab), B=2, L=tb.L,
             M=tb.M, taps=tb.taps, n_weights=tb.n_weights, out_stride=2297)
    a.update(over)
    return Lb.avc_resample(a["x"], 5000, a["lens"], a["lens_dev"], a["B"], a["weights"], a["n_weights"], a["tab"],
                           a["tab_dev"], a["L"], a["M"], a["taps"], a["out"], a["out_stride"], None)


def test_resample_host_refusals_without_a_gpu():
    """Every argument check precedes the launch: each bad call comes back as an error, with its message,
    on a machine with no device.  The pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(256)
    ptrs = {k: p for k in ("x", "lens_dev", "weights", "tab_dev", "out")}
    for what, over, msg in refusal_cases():
        assert call_resample(Lb, ptrs, **over) == -1, what
        assert msg in Lb.avc_last_error(), (what, Lb.avc_last_error())


def test_python_refusals_and_the_same_rate_bypass(monkeypatch):
    from autoformer_amd import _lib
    from autoformer_amd.resample import Resample, resample_table

    with pytest.raises(ValueError, match="AVC_RESAMPLE_MAX_WEIGHTS"):
        resample_table(192000)                      # 147 residues x 1129 taps
    with pytest.raises(ValueError, match="AVC_RESAMPLE_MAX_WEIGHTS"):
        Resample(22051)                             # L = 22050
    with pytest.raises(ValueError, match="positive"):
        Resample(0)
    rs = Resample(48000)
    x = torch.zeros(2, 500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.frames(x)                                # host tensors are refused, never computed elsewhere
    with pytest.raises(ValueError, match="exceeds"):
        rs.frames(x, lens=[500, 501])
    with pytest.raises(ValueError, match="at least one sample"):
        rs.frames(x, lens=[500, 0])
    with pytest.raises(ValueError, match="B=2"):
        rs.frames(x, lens=[500])
    with pytest.raises(ValueError, match="fp32 audio"):
        rs.frames(x.double())
    with pytest.raises(ValueError, match="own lengths"):
        rs.frames([x[0]], lens=[500])

    def no_launch(*a, **k):
        raise AssertionError("the same-rate bypass launched something")

    monkeypatch.setattr(_lib, "call", no_launch)
    same = Resample(22050)
    assert same.bypass and same.table is None
    out, lens = same.frames(x, lens=[500, 321])
    assert out is x and lens == [500, 321]
    out, lens = same.frames([torch.ones(3), torch.ones(5)])
    assert lens == [3, 5] and out.shape == (2, 5) and out[0].tolist() == [1, 1, 1, 0, 0]
    assert Resample(44100, 44100).bypass and not Resample(44100).bypass


# ----------------------------------------------------------------------- make_spec bookkeeping
def test_make_spec_resample_bookkeeping(tmp_path):
    """A tree mixing 48000 and 22050 Hz files with resample=True: batches never mix rates, the lengths
    planned and handed on are the resampled ones, a file too short AFTER resampling is refused by name
    before anything is written, and the default still refuses another rate."""
    from autoformer_amd import make_spec as MS
    from autoformer_amd.resample import out_len

    rng = np.random.RandomState(6)
    wavs = {("spkA", "a.wav"): (48000, 2000), ("spkA", "b.wav"): (22050, 700), ("spkA", "c.wav"): (48000, 1100),
            ("spkB", "d.wav"): (22050, 500), ("spkB", "e.wav"): (48000, 1500), ("spkB", "f.wav"): (22050, 900)}
    for (spk, fn), (fs, n) in wavs.items():
        os.makedirs(tmp_path / "wav" / spk, exist_ok=True)
        write_wav(tmp_path / "wav" / spk / fn, 0.2 * rng.randn(n).clip(-3, 3), fs=fs)
    calls, rcalls = [], []

    def resampler(fs, waves, device):
        rcalls.append((fs, [len(w) for w in waves]))
        lens = [out_len(len(w), fs) for w in waves]
        return np.zeros((len(waves), max(lens)), dtype=np.float32), lens

    def recorder(a2m, waves, lens=None):
        lens = [len(w) for w in waves] if lens is None else list(lens)
        calls.append(lens)
        return [np.full((MS.n_frames(n), 80), float(n), dtype=np.float32) for n in lens]

    out = tmp_path / "spmel"
    written = MS.convert_tree(str(tmp_path / "wav"), str(out), max_batch=2, a2m=object(), mels_fn=recorder,
                              resample=True, resample_fn=resampler)
    assert [os.path.relpath(p, out) for p in written] == ["spkA/a..npy", "spkA/b..npy", "spkA/c..npy", "spkB/d..npy",
                                                          "spkB/e..npy", "spkB/f..npy"]
    # 22050 Hz files first (rates ascending), each group sorted by its resampled length, two to a launch
    assert calls == [[500, 700], [900], [506, 690], [919]]
    assert rcalls == [(48000, [1100, 1500]), (48000, [2000])]            # only the 48 kHz files, never mixed
    assert [out_len(n, 48000) for n in (1100, 1500, 2000)] == [506, 690, 919]
    for p, n in zip(written, (919, 700, 506, 500, 690, 900)):
        m = np.load(p)
        assert m.dtype == np.float32 and m.shape == (MS.n_frames(n), 80) and (m == n).all()
    # 800 samples at 48 kHz are long enough as they are (> 384) and too short once resampled (368)
    write_wav(tmp_path / "wav" / "spkB" / "g.wav", np.zeros(800), fs=48000)
    assert out_len(800, 48000) == 368
    with pytest.raises(ValueError, match=r"spkB/g\.wav.*too short.*after resampling 48000"):
        MS.convert_tree(str(tmp_path / "wav"), str(tmp_path / "o2"), a2m=object(), mels_fn=recorder, resample=True,
                        resample_fn=resampler)
    assert not os.path.exists(tmp_path / "o2")
    os.remove(tmp_path / "wav" / "spkB" / "g.wav")
    # a resampler that returns other lengths than planned is an error, not a silent mis-slice
    with pytest.raises(RuntimeError, match="returned lengths"):
        MS.convert_tree(str(tmp_path / "wav"), str(tmp_path / "o3"), a2m=object(), mels_fn=recorder, resample=True,
                        resample_fn=lambda fs, w, d: (None, [1] * len(w)))
    # the default: another rate is still refused by name before anything is written
    with pytest.raises(ValueError, match=r"spkA/a\.wav.*48000 Hz.*resample the file first"):
        MS.convert_tree(str(tmp_path / "wav"), str(tmp_path / "o4"), a2m=object(), mels_fn=recorder)
    os.makedirs(tmp_path / "w2" / "spkB")
    write_wav(tmp_path / "w2" / "spkB" / "t.wav", np.zeros(600))
    write_wav(tmp_path / "w2" / "spkB" / "u0.wav", np.zeros(600), fs=16000)
    with pytest.raises(ValueError, match=r"spkB/u0\.wav.*16000 Hz.*resample the file first"):
        MS.convert_tree(str(tmp_path / "w2"), str(tmp_path / "o4"), a2m=object(), mels_fn=recorder)
    assert not os.path.exists(tmp_path / "o4")
    with pytest.raises(ValueError, match="16000 Hz"):
        MS.wav_to_mel(np.zeros(1000, dtype=np.float32), 16000, a2m=object())
    with pytest.raises(ValueError, match="too short"):
        MS.wav_to_mel(np.zeros(800, dtype=np.float32), 48000, a2m=object(), resample=True)
    assert MS._parser().parse_args(["--wav_dir", "a", "--out_dir", "b"]).resample is False
    assert MS._parser().parse_args(["--wav_dir", "a", "--out_dir", "b", "--resample"]).resample is True
