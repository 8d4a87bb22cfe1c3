"""The MelGAN generator over ragged batches on the GPU: the three entry points of include/autovc_hip_vocoder.h
(csrc/melgan_ragged.hip), each called directly and compared with a float64 numpy restatement written here, then
Generator.frames_ragged / MelVocoder.inverse_ragged / convert_whole(vocoder=...) against the CPU oracle
(oracle/melgan_cpu.py, pinned to the reference fixture by tests/test_melgan.py) run per utterance at its own length.

Kernel bars.  The gather and the masked LeakyReLU move values and apply at most ONE fp32 multiply (v * slope):
the product of two fp32 numbers is exact in float64, so the restatement rounded once to fp32 IS the IEEE result
and the comparison is bit for bit; a bf16 output is that fp32 value rounded once more (round to nearest even,
torch's .to(bfloat16)).  The output layer takes the bar of test_gpu_melgan_glue.py::test_mg_conv_out.
Padding rows: NaN in every input, exactly +0.0 in every output.

Generator bars: those of tests/test_melgan.py, rel-inf < 1e-4 (fp32 mode) and < 5e-2 (bf16 mode), per utterance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import melgan_cpu as O

from .helpers import EPS32, bits_equal, f64, report
from .test_melgan import _rel_inf, _sd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = float(np.float32(0.2))  # the slope as the kernels receive it
HOP = 256
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def _tdt(bf):
    return torch.bfloat16 if bf else torch.float32


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _with_nan_padding(x, lens, scale):
    """x (B, L, C): rows t >= lens[b]*scale of every block become NaN."""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n * scale:] = float("nan")
    return x


def _reflect(s, n):
    return -s if s < 0 else (2 * (n - 1) - s if s >= n else s)


def _leaky64(a):
    return np.where(a >= 0, a, a * SLOPE)


def _lens(lens, Tmax):
    from autoformer_amd import kernels as K

    return K.Lens(lens, Tmax, DEV)


def _as_out(ref64, bf):
    """float64 restatement -> the kernel's output dtype: one rounding to fp32, one more to bf16."""
    t = torch.from_numpy(ref64.astype(np.float32))
    return t.to(torch.bfloat16) if bf else t


# ------------------------------------------------------------------------------------- gather
# conv_in with a row at the 4-frame minimum (every output frame of it reads a reflected one); the widest dilation at
# the first stage, 32 rows against pad 9; a minimal 3-tap
GATHER = [(3, 12, 80, 7, 1, 3, 1, (12, 4, 7)), (3, 6, 16, 3, 9, 9, 8, (6, 4, 5)), (2, 5, 8, 3, 1, 1, 2, (5, 4))]


def _gather_ref(x64, lens, scale, taps, dil, pad, act):
    B, L, C = x64.shape
    out = np.zeros((B, L, taps * C))
    a = _leaky64(x64) if act else x64
    for b in range(B):
        n = lens[b] * scale
        for t in range(n):
            for k in range(taps):
                out[b, t, k * C:(k + 1) * C] = a[b, _reflect(t + k * dil - pad, n)]
    return out


def _gather_call(xd, B, Tmax, C, taps, dil, pad, act, Ln, scale, out_bf):
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    out = torch.full((B * Tmax * scale, taps * C), SENTINEL, device=DEV, dtype=_tdt(out_bf))
    _lib.call("avc_mg_gather_ragged", xd.data_ptr(), K._dt(xd), B, Tmax, C, taps, dil, pad, act, SLOPE, Ln.host,
              Ln.dev.data_ptr(), scale, out.data_ptr(), int(out_bf), K.stream())
    return out


@pytest.mark.parametrize("B,Tmax,C,taps,dil,pad,scale,lens", GATHER)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("in_bf,out_bf", [(False, False), (False, True), (True, False), (True, True)])
def test_gather_against_fp64(B, Tmax, C, taps, dil, pad, scale, lens, act, in_bf, out_bf):
    L = Tmax * scale
    x = _with_nan_padding(_rand(B, L, C, seed=L + C).to(_tdt(in_bf)), lens, scale)
    got = _gather_call(x.to(DEV), B, Tmax, C, taps, dil, pad, act, _lens(lens, Tmax), scale, out_bf)
    ref = _gather_ref(x.double().numpy(), lens, scale, taps, dil, pad, act)
    assert not np.isnan(ref).any()                       # the restatement read no padding row either
    assert bits_equal(got.view(B, L, taps * C), _as_out(ref, out_bf))   # valid rows exact, padding rows +0.0


@pytest.mark.parametrize("B,Tmax,C,taps,dil,pad,scale,lens", GATHER)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("in_bf,out_bf", [(False, False), (False, True), (True, False), (True, True)])
def test_gather_full_lengths_match_the_rectangular_form(B, Tmax, C, taps, dil, pad, scale, lens, act, in_bf, out_bf):
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    L = Tmax * scale
    xd = _rand(B, L, C, seed=3 * L + C).to(_tdt(in_bf)).to(DEV)
    got = _gather_call(xd, B, Tmax, C, taps, dil, pad, act, _lens((Tmax,) * B, Tmax), scale, out_bf)
    rect = torch.full_like(got, SENTINEL)
    _lib.call("avc_mg_gather", xd.data_ptr(), int(in_bf), B, L, C, taps, dil, pad, 1, act, SLOPE, rect.data_ptr(),
              int(out_bf), K.stream())
    assert bits_equal(got, rect)


# ------------------------------------------------------------------------------------- masked LeakyReLU
@pytest.mark.parametrize("B,Tmax,C,scale,lens", [(3, 6, 8, 8, (6, 4, 5)), (2, 5, 4, 1, (2, 5))])
@pytest.mark.parametrize("outs", ["f32", "bf16", "both"])
def test_act_against_fp64(B, Tmax, C, scale, lens, outs):
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    L = Tmax * scale
    x = _with_nan_padding(_rand(B, L, C, seed=L + C), lens, scale)
    ref = np.zeros((B, L, C))
    for b, n in enumerate(lens):
        ref[b, :n * scale] = _leaky64(x[b, :n * scale].double().numpy())
    xd, Ln = x.to(DEV), _lens(lens, Tmax)
    o = torch.full((B, L, C), SENTINEL, device=DEV) if outs != "bf16" else None
    o16 = torch.full((B, L, C), SENTINEL, device=DEV, dtype=torch.bfloat16) if outs != "f32" else None
    _lib.call("avc_mg_act_ragged", xd.data_ptr(), B, Tmax, C, SLOPE, Ln.host, Ln.dev.data_ptr(), scale, K._ptr(o),
              K._ptr(o16), K.stream())
    if o is not None:
        assert bits_equal(o, _as_out(ref, False))
    if o16 is not None:
        assert bits_equal(o16, _as_out(ref, True))
    # full lengths: the rectangular twin, bit for bit
    xf = _rand(B, L, C, seed=5).to(DEV)
    a, b_ = torch.empty_like(xf), torch.empty_like(xf)
    Lf = _lens((Tmax,) * B, Tmax)
    _lib.call("avc_mg_act_ragged", xf.data_ptr(), B, Tmax, C, SLOPE, Lf.host, Lf.dev.data_ptr(), scale, a.data_ptr(), None,
              K.stream())
    _lib.call("avc_mg_act", xf.data_ptr(), xf.numel(), SLOPE, b_.data_ptr(), None, K.stream())
    assert bits_equal(a, b_)


# ------------------------------------------------------------------------------------- output layer
def _conv_out_call(xd, B, Tmax, C, wd, bd, Ln, scale):
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    out = torch.full((B, Tmax * scale), SENTINEL, device=DEV)
    _lib.call("avc_mg_conv_out_ragged", xd.data_ptr(), B, Tmax, C, 7, wd.data_ptr(), bd.data_ptr(), SLOPE, Ln.host,
              Ln.dev.data_ptr(), scale, out.data_ptr(), K.stream())
    return out


@pytest.mark.parametrize("B,Tmax,C,scale,lens", [(3, 6, 32, 4, (6, 4, 5)), (2, 4, 4, 1, (4, 4)), (1, 300, 8, 1, (290,))])
def test_conv_out_against_fp64(B, Tmax, C, scale, lens):
    """(1, 300, 8): a second workgroup of 256 samples, with the utterance's end inside it."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    L = Tmax * scale
    clean = _rand(B, L, C, seed=C)
    x = _with_nan_padding(clean, lens, scale)
    w, bias = _rand(7, C, seed=C + 1, scale=0.2), _rand(1, seed=C + 2, scale=0.1)
    wd, bd = w.to(DEV), bias.to(DEV)
    got = _conv_out_call(x.to(DEV), B, Tmax, C, wd, bd, _lens(lens, Tmax), scale)
    a, w64 = _leaky64(x.double().numpy()), w.double().numpy()
    worst = 0.0
    for b, nf in enumerate(lens):
        n = nf * scale
        pre, sabs = np.full(n, float(bias[0])), np.full(n, abs(float(bias[0])))
        for t in range(n):
            for k in range(7):
                row = a[b, _reflect(t + k - 3, n)]
                pre[t] += row @ w64[k]
                sabs[t] += np.abs(row) @ np.abs(w64[k])
        ref = np.tanh(pre)
        # test_mg_conv_out's bar: 7*C + 2 dependent fp32 roundings on the pre-activation (tanh is 1-Lipschitz) plus
        # the transcendental bar (rtol 1e-5, atol 1e-6)
        err = np.abs(f64(got[b, :n]).numpy() - ref)
        worst = max(worst, float((err / ((7 * C + 2) * EPS32 * sabs + 1e-5 * np.abs(ref) + 1e-6)).max()))
        assert bits_equal(got[b, n:], torch.zeros(L - n))          # padding samples: exactly 0.0
    assert report("conv_out_ragged", f"({B},{Tmax},{C},{scale},{lens})", worst) <= 1.0
    # full lengths: the rectangular kernel, bit for bit
    full = _conv_out_call(clean.to(DEV), B, Tmax, C, wd, bd, _lens((Tmax,) * B, Tmax), scale)
    rect = torch.full((B, L), SENTINEL, device=DEV)
    _lib.call("avc_mg_conv_out", clean.to(DEV).data_ptr(), B, L, C, 7, wd.data_ptr(), bd.data_ptr(), SLOPE, rect.data_ptr(),
              K.stream())
    assert bits_equal(full, rect)


# ------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    """Real device pointers: each refused call returns non-zero with a message and leaves its outputs as they were."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    B, Tmax, C, scale = 2, 6, 8, 2
    L = Tmax * scale
    x = torch.zeros(B * L, C, device=DEV)
    x1 = torch.zeros(B * L * 6 + 1, device=DEV)[1:]           # a base 4 bytes off a 16-byte boundary
    w, bias = torch.zeros(7, C, device=DEV), torch.zeros(1, device=DEV)
    outs = [torch.full((B * L, 7 * C), SENTINEL, device=DEV), torch.full((B * L, C), SENTINEL, device=DEV),
            torch.full((B * L,), SENTINEL, device=DEV)]
    og, oa, oc = (o.data_ptr() for o in outs)
    ok, long_, short = (ctypes.c_int * 2)(6, 4), (ctypes.c_int * 2)(7, 4), (ctypes.c_int * 2)(6, 1)
    ldev = torch.tensor([6, 4], dtype=torch.int32, device=DEV).data_ptr()
    xp = x.data_ptr()

    def gather(x=xp, lens=ok, ld=ldev, C=C, taps=3, dil=1, pad=1, out=og, scale=scale):
        return Lb.avc_mg_gather_ragged(x, 0, B, Tmax, C, taps, dil, pad, 1, SLOPE, lens, ld, scale, out, 0, None)

    def act(x=xp, lens=ok, ld=ldev, C=C, out=oa):
        return Lb.avc_mg_act_ragged(x, B, Tmax, C, SLOPE, lens, ld, scale, out, None, None)

    def conv(x=xp, lens=ok, ld=ldev, C=C, out=oc, scale=scale, w=w.data_ptr()):
        return Lb.avc_mg_conv_out_ragged(x, B, Tmax, C, 7, w, bias.data_ptr(), SLOPE, lens, ld, scale, out, None)

    def err():
        return Lb.avc_last_error().decode()

    for fn, name in ((gather, "avc_mg_gather_ragged"), (act, "avc_mg_act_ragged"), (conv, "avc_mg_conv_out_ragged")):
        assert fn(lens=long_) != 0 and name + ": lens[0] = 7 outside 1..Tmax = 6" in err()
        assert fn(C=6) != 0 and "multiple of 4" in err()
        assert fn(x=None) != 0 and "null pointer" in err()
        assert fn(out=None) != 0 and "null pointer" in err()
        assert fn(lens=None) != 0 and "null pointer" in err()
        assert fn(ld=None) != 0 and "null pointer" in err()
        assert fn(x=x1.data_ptr()) != 0 and "aligned" in err()
    assert gather(taps=3, dil=9, pad=9, scale=1) != 0 and "reflection pad 9" in err()       # pad >= lens[b]*scale
    assert gather(taps=3, dil=2, pad=1) != 0 and "keeps the length" in err()
    assert conv(lens=short, scale=2) != 0 and "reflection pad 3" in err()                   # 1 * 2 <= 3
    assert conv(w=None) != 0 and "null pointer" in err()
    torch.cuda.synchronize()
    for o in outs:
        assert bits_equal(o, torch.full_like(o, SENTINEL).cpu())
    assert gather() == 0 and act() == 0 and conv() == 0                                     # the defaults do run
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- generator
TMAX, LENS = 37, (37, 4, 21, 37)


@functools.lru_cache(maxsize=None)
def _mels():
    """Four (37, 80) frame-major mels; read-only."""
    from autoformer_amd.detinit import det_mel

    m = np.ascontiguousarray(det_mel(4, 80, TMAX, seed=11).transpose(0, 2, 1))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _oracle(row, T):
    """The CPU oracle's B = 1 forward of _mels()[row][:T] at its own length: (T*256,) float32; computed once."""
    mel = torch.from_numpy(_mels()[row, :T].T.copy()).unsqueeze(0)
    out = O.generator(_sd(), mel).reshape(-1).numpy().copy()
    out.setflags(write=False)
    return out


def _gen(comp):
    import autoformer_amd as A
    from autoformer_amd.melgan import Generator

    A.set_compute(comp)
    g = Generator(80, 32, 3)
    g.load_state_dict(_sd())
    return g.to(DEV)


def _batch(fill):
    """(4*37, 80) device mel of LENS with `fill` in the padding rows."""
    x = np.full((4, TMAX, 80), fill, np.float32)
    for b, n in enumerate(LENS):
        x[b, :n] = _mels()[b, :n]
    return torch.from_numpy(x).to(DEV).view(4 * TMAX, 80)


@pytest.mark.parametrize("comp,tol", [("fp32", 1e-4), ("bf16", 5e-2)])
def test_frames_ragged_matches_the_oracle_per_utterance(comp, tol):
    g = _gen(comp)
    audio = g.frames_ragged(_batch(0.0), _lens(LENS, TMAX))
    torch.cuda.synchronize()
    assert audio.shape == (4, TMAX * HOP) and audio.dtype == torch.float32
    rels = [_rel_inf(audio[b, :n * HOP].cpu().numpy(), _oracle(b, n)) for b, n in enumerate(LENS)]
    print(f"frames_ragged {comp} vs oracle per utterance, rel-inf:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < tol, rels
    for b, n in enumerate(LENS):
        assert bits_equal(audio[b, n * HOP:], torch.zeros((TMAX - n) * HOP))
    # and the B = 1 forward of the existing path at the utterance's own length, the function it stands for
    one = g.frames(torch.from_numpy(_mels()[2, :21].copy()).to(DEV), 1, 21)
    print("  row 2 against frames(B = 1): max abs diff", float((one[0] - audio[2, :21 * HOP]).abs().max()))
    assert _rel_inf(audio[2, :21 * HOP].cpu().numpy(), one[0].cpu().numpy()) < tol


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
def test_nothing_leaks_from_the_padding(comp):
    """NaN in the mel's padding rows, then other finite garbage there: the same bits in every valid sample, run
    after run.  A kernel that reflects about the block edge, or a window that reads a short row's padding, fails."""
    g = _gen(comp)
    Ln = _lens(LENS, TMAX)
    a = g.frames_ragged(_batch(float("nan")), Ln)
    b = g.frames_ragged(_batch(1e4), Ln)
    c = g.frames_ragged(_batch(float("nan")), Ln)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert bits_equal(a, b) and bits_equal(a, c)


def test_frames_ragged_refuses_a_short_utterance_and_other_lens():
    from autoformer_amd import _lib

    g = _gen("bf16")
    calls = []
    real = _lib.call
    _lib.call = lambda name, *a: calls.append(name)
    try:
        with pytest.raises(ValueError, match="at least 4"):
            g.frames_ragged(torch.zeros(2 * 6, 80, device=DEV), _lens((6, 3), 6))
        with pytest.raises(TypeError):
            g.frames_ragged(torch.zeros(2 * 6, 80, device=DEV), [6, 4])
        with pytest.raises(ValueError):
            g.frames_ragged(torch.zeros(2 * 7, 80, device=DEV), _lens((6, 4), 6))
    finally:
        _lib.call = real
    assert calls == []


# ------------------------------------------------------------------------------------- MelVocoder.inverse_ragged
ROWS, TS = (2, 1, 0, 3, 1), (21, 4, 37, 9, 21)          # utterance i = _mels()[ROWS[i]][:TS[i]]


def _utts():
    return [np.ascontiguousarray(_mels()[r, :T]) for r, T in zip(ROWS, TS)]


@pytest.mark.parametrize("comp,tol", [("fp32", 1e-4), ("bf16", 5e-2)])
def test_inverse_ragged_order_lengths_and_oracle(comp, tol):
    from autoformer_amd.convert import plan_whole
    from autoformer_amd.melgan import MelVocoder

    voc = MelVocoder(generator=_gen(comp))
    assert plan_whole(TS, 1, 2, 8192) == [([1, 3], 9), ([0, 4], 21), ([2], 37)]       # several batches form
    wavs = voc.inverse_ragged(_utts(), max_batch=2)
    torch.cuda.synchronize()
    assert [tuple(w.shape) for w in wavs] == [(T * HOP,) for T in TS] and all(w.dtype == torch.float32 for w in wavs)
    rels = [_rel_inf(w.cpu().numpy(), _oracle(r, T)) for w, r, T in zip(wavs, ROWS, TS)]
    print(f"inverse_ragged {comp} vs oracle, rel-inf:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < tol, rels
    # a permutation that leaves the batches (and the rows' order inside them) as they were: the same bits.
    # Device tensors this time.
    perm = [2, 1, 0, 3, 4]
    assert plan_whole([TS[p] for p in perm], 1, 2, 8192) == [([1, 3], 9), ([2, 4], 21), ([0], 37)]
    again = voc.inverse_ragged([torch.tensor(_utts()[p]).to(DEV) for p in perm], max_batch=2)
    for j, p in enumerate(perm):
        assert bits_equal(again[j], wavs[p]), (j, p)


def test_inverse_ragged_refuses_three_frames_before_any_launch():
    from autoformer_amd import _lib
    from autoformer_amd.melgan import MelVocoder

    voc = MelVocoder(generator=_gen("bf16"))
    calls = []
    real = _lib.call
    _lib.call = lambda name, *a: calls.append(name)
    try:
        with pytest.raises(ValueError, match="3 frames"):
            voc.inverse_ragged(_utts() + [np.zeros((3, 80), np.float32)], max_batch=2)
    finally:
        _lib.call = real
    assert calls == []


# ------------------------------------------------------------------------------------- convert_whole(vocoder=...)
def test_convert_whole_with_a_vocoder():
    """The mels are those of convert_whole without a vocoder (np.array_equal); the wavs are the oracle's generator
    applied to those mels, per utterance at its true length (13 is padded to 16 for the conversion, not for the
    vocoder)."""
    import autoformer_amd as A
    from autoformer_amd.convert import convert_whole
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.factory.AutoVC import AutoVC
    from autoformer_amd.melgan import MelVocoder

    lengths = (40, 13, 24)
    voc = MelVocoder(generator=_gen("fp32"))
    A.set_compute("fp32")
    m = AutoVC(44, 256, 512, 8)
    det_init_(m)
    m = m.to(DEV).train()
    x, e = det_inputs(3, max(lengths), seed=54)
    mels = [np.ascontiguousarray(x[i][:T]) for i, T in enumerate(lengths)]
    et = np.roll(e, -1, axis=0)
    plain = convert_whole(m, mels, e, et)
    got, wavs = convert_whole(m, mels, e, et, vocoder=voc)
    assert len(got) == len(wavs) == 3
    rels = []
    for i, T in enumerate(lengths):
        assert np.array_equal(got[i], plain[i])
        assert wavs[i].shape == (T * HOP,) and wavs[i].dtype == np.float32
        ref = O.generator(_sd(), torch.from_numpy(got[i].T.copy()).unsqueeze(0)).reshape(-1).numpy()
        rels.append(_rel_inf(wavs[i], ref))
    print("convert_whole(vocoder) wavs vs oracle, rel-inf:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < 1e-4, rels
