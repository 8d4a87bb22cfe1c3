"""The three entry points of include/autovc_hip_ragged.h (csrc/ragged.hip), each called directly and
compared per element with a float64 numpy restatement written here.

avc_bn_seg_ragged: B = 3, T = 12, lens = (12, 2, 7) -- a full segment, the shortest the kernel admits and an
odd one -- at C = 80 in ld = 96 (a partial 64-channel tile, ld > C) and at C = 130 (three tiles); every
AVC_ACT_* code, with and without the residual; fp32-only, bf16-only and both outputs; mean / rstd; and
T = 260 with lens = (260, 241, 5): the re-read form (twice) and the LDS-resident form in ONE launch.  The
input's padding rows hold 1e30 and NaN, so a statistic that read one of them is not finite.  Bars: those
tests/test_gpu_bn_seg.py holds avc_bn_seg_apply to (rel-inf < 1e-5 on the outputs; mean and rstd to 1e-5
per (segment, channel)); padding rows must be == 0.0 exactly; the bf16 output must be the fp32 output
rounded once; with lens = (T,) * B every output is bit-identical to avc_bn_seg_apply's.

avc_row_mask: C = 78 (not a multiple of 4, the scalar form) in ld = 83 and C = 80 in ld = 96 (the 16-byte
form); fp32, bf16 and both; everything outside (row >= lens[b], column < C) keeps its bits.

avc_bilstm_ragged_fwd: H = 32 and 44, B = 3, T = 9, lens = (9, 2, 5) against a float64 loop per utterance
and direction, in both compute modes.  Bars: the ones tests/test_gpu_lstm_paths.py holds the small-H
recurrence to, whose per-step arithmetic this kernel repeats (fp32 compute 1e-4; fast activations
8e-7 rel-Frobenius / 2e-6 max-abs ratio); with lens = (T,) * B, h against avc_lstm_fwd's at the same bars.

Refusals: bad lens, null pointers and C = 0 return non-zero with a message and leave sentinel-filled outputs
as they were."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
BN_BAR = 1e-5
FP32_BAR = 1e-4
FAST_BAR_RELF, FAST_BAR_RINF = 8e-7, 2e-6


@pytest.fixture(autouse=True)
def _fp32():
    import autoformer_amd as A

    A.set_compute("fp32")
    yield
    A.set_compute("bf16")


def rinf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def relf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def act64(z, act):
    if act == 1:
        return np.maximum(z, 0.0)
    if act == 2:
        return np.tanh(z)
    if act == 3:
        return np.where(z > 0, z, 0.01 * z)
    if act == 4:
        return 0.5 * z * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0)))
    if act == 5:
        return 1.0 / (1.0 + np.exp(-z))
    return z


def bn_ref(y, B, T, C, lens, gamma, beta, act, res=None):
    """float64: out (B*T, C) with zeros in the padding rows, mean and rstd (B, C); y's padding rows unread."""
    y = np.asarray(y, np.float64).reshape(B, T, -1)[:, :, :C]
    out = np.zeros((B, T, C))
    mean, rstd = np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        seg = y[b, :lens[b]]
        mean[b] = seg.mean(axis=0)
        rstd[b] = 1.0 / np.sqrt(((seg - mean[b]) ** 2).mean(axis=0) + EPS)
        o = act64((seg - mean[b]) * rstd[b] * gamma + beta, act)
        if res is not None:
            o = o + np.asarray(res, np.float64).reshape(B, T, -1)[b, :lens[b], :C]
        out[b, :lens[b]] = o
    return out.reshape(B * T, C), mean, rstd


def bn_inputs(B, T, C, ld, lens, seed=0, poison=True):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B * T, ld, generator=g) * 2 + 1
    y += torch.randn(B, 1, ld, generator=g).repeat_interleave(T, dim=0).reshape(B * T, ld)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res = torch.randn(B * T, ld, generator=g)
    # A 2-row segment whose two values of a channel nearly coincide is ill-conditioned for ANY fp32
    # evaluation: the mean is rounded to half an ulp of |y| (~1e-7), the centred values are ~|y0 - y1| / 2 and
    # rstd grows to 1 / sqrt(eps) = 316, so a pair 7e-3 apart (one channel in 130 draws one, at random) puts
    # 1.2e-5 on the output whatever the kernel does -- an fp32 restatement of the arithmetic on the CPU and
    # avc_bn_seg_apply itself give the same figure.  The bar is about the kernel, so the rows of a segment
    # shorter than 4 are spaced at least 1 apart per channel.
    y3 = y.view(B, T, ld)
    for b in range(B):
        if lens[b] < 4:
            step = 1 + torch.rand(ld, generator=g)
            for r in range(1, lens[b]):
                y3[b, r] = y3[b, 0] + r * step
    if poison:   # what must never reach a statistic: alternating 1e30 and NaN in the padding rows
        y3 = y.view(B, T, ld)
        for b in range(B):
            y3[b, lens[b]::2] = 1e30
            y3[b, lens[b] + 1::2] = float("nan")
    return y, gamma, beta, res


def pad_rows(B, T, lens):
    m = np.zeros((B, T), bool)
    for b in range(B):
        m[b, lens[b]:] = True
    return m.reshape(B * T)


BN_CASES = [(3, 12, 80, 96, (12, 2, 7)), (3, 12, 130, 130, (12, 2, 7)), (3, 260, 80, 96, (260, 241, 5))]


@pytest.mark.parametrize("B,T,C,ld,lens", BN_CASES)
def test_bn_against_fp64(B, T, C, ld, lens):
    """Every act, with and without the residual: outputs, mean, rstd; zeros in the padding rows."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    assert max(lens) > _lib.BN_SEG_LDS_ROWS or T == 12       # the long case runs both forms in one launch
    y, gamma, beta, res = bn_inputs(B, T, C, ld, lens)
    L = Kr.Lens(lens, T, DEV)
    yd, gd, bd, rd = y.to(DEV), gamma.to(DEV), beta.to(DEV), res.to(DEV)
    pad = pad_rows(B, T, lens)
    for act in range(6):
        for r_host, r_dev in ((None, None), (res, rd)):
            want, mean, rstd = bn_ref(y, B, T, C, lens, gamma.double().numpy(), beta.double().numpy(), act, r_host)
            got, m, r = Kr.bn_seg_ragged(yd, L, gd, bd, EPS, act, r_dev, C=C, want_stats=True, twin16=False)
            o = host(got)[:, :C]
            e = (rinf(o, want), rinf(host(m), mean), rinf(host(r), rstd))
            print(f"B={B} T={T} C={C} ld={ld} lens={lens} act={act} res={r_host is not None}: out {e[0]:.2e} "
                  f"mean {e[1]:.2e} rstd {e[2]:.2e}")
            assert np.isfinite(o).all() and max(e) < BN_BAR, e
            assert (np.abs(host(m) - mean) <= BN_BAR * np.maximum(np.abs(mean), 1.0)).all()
            assert (np.abs(host(r) - rstd) <= BN_BAR * rstd).all()
            assert (o[pad] == 0.0).all() and pad.any()


@pytest.mark.parametrize("B,T,C,ld,lens", BN_CASES)
def test_bn_output_forms(B, T, C, ld, lens):
    """fp32 only, bf16 only, both: the bf16 output is the fp32 one rounded once, whichever are written;
    exact zeros in the padding rows of each; columns >= C and the rows around the statistics keep a
    sentinel."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    S = -768.0   # exact in bf16
    y, gamma, beta, res = bn_inputs(B, T, C, ld, lens, seed=1)
    L = Kr.Lens(lens, T, DEV)
    yd, gd, bd, rd = y.to(DEV), gamma.to(DEV), beta.to(DEV), res.to(DEV)
    pad = torch.from_numpy(pad_rows(B, T, lens))
    want, mean, rstd = bn_ref(y, B, T, C, lens, gamma.double().numpy(), beta.double().numpy(), 2, res)
    outs = {}
    for form in ("fp32", "bf16", "both"):
        o32 = torch.full((B * T, ld), S, device=DEV) if form != "bf16" else None
        o16 = torch.full((B * T, ld), S, device=DEV, dtype=torch.bfloat16) if form != "fp32" else None
        stats = torch.full((2, B + 2, C), S, device=DEV)
        _lib.call("avc_bn_seg_ragged", yd.data_ptr(), _lib.F32, ld, B, T, C, L.host, L.dev.data_ptr(), gd.data_ptr(),
                  bd.data_ptr(), EPS, 2, rd.data_ptr(), Kr._ptr(o32), Kr._ptr(o16), stats[0, 1].data_ptr(),
                  stats[1, 1].data_ptr(), Kr.stream())
        torch.cuda.synchronize()
        for o in (o32, o16):
            if o is not None:
                o = o.cpu()
                assert (o[:, C:] == S).all() and not (o[:, :C] == S).any()
                assert (o[pad][:, :C] == 0).all()
        assert (stats[:, 0] == S).all() and (stats[:, B + 1] == S).all()
        assert rinf(host(stats[0, 1:B + 1]), mean) < BN_BAR and rinf(host(stats[1, 1:B + 1]), rstd) < BN_BAR
        outs[form] = (o32, o16)
    assert rinf(host(outs["fp32"][0])[:, :C], want) < BN_BAR
    assert torch.equal(outs["both"][0], outs["fp32"][0])
    assert torch.equal(outs["both"][1][:, :C], outs["fp32"][0][:, :C].bfloat16())
    assert torch.equal(outs["bf16"][1], outs["both"][1])


@pytest.mark.parametrize("B,T,C,ld", [(3, 12, 80, 96), (2, 260, 130, 130)])
def test_bn_full_lengths_match_bn_seg_apply_bit_for_bit(B, T, C, ld):
    """lens = (T,) * B is avc_bn_seg_apply: the same sums in the same order, resident and re-read."""
    from autoformer_amd import kernels as Kr

    lens = (T,) * B
    y, gamma, beta, res = bn_inputs(B, T, C, ld, lens, seed=2, poison=False)
    yd, gd, bd, rd = y.to(DEV), gamma.to(DEV), beta.to(DEV), res.to(DEV)
    L = Kr.Lens(lens, T, DEV)
    for act in range(6):
        for r in (None, rd):
            a, ma, ra = Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, r, C=C, want_stats=True, twin16=True)
            b, mb, rb = Kr.bn_seg_ragged(yd, L, gd, bd, EPS, act, r, C=C, want_stats=True, twin16=True)
            assert torch.equal(a[:, :C], b[:, :C]) and torch.equal(a._bf16[:, :C], b._bf16[:, :C]), (act, r is not None)
            assert torch.equal(ma, mb) and torch.equal(ra, rb)


def test_bn_segments_are_independent():
    """Another segment's data and length do not move a bit of segment 0 (resident and re-read)."""
    from autoformer_amd import kernels as Kr

    B, T, C = 2, 260, 80
    y, gamma, beta, _ = bn_inputs(B, T, C, C, (T, T), seed=5, poison=False)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for l0 in (250, 31):
        a = Kr.bn_seg_ragged(y.to(DEV), Kr.Lens((l0, T), T, DEV), gd, bd, EPS, 2)
        y2 = y.clone()
        y2[T:] = y2[T:] * 3 - 7
        b = Kr.bn_seg_ragged(y2.to(DEV), Kr.Lens((l0, 9), T, DEV), gd, bd, EPS, 2)
        one = Kr.bn_seg_ragged(y[:T].contiguous().to(DEV), Kr.Lens((l0,), T, DEV), gd, bd, EPS, 2)
        assert torch.equal(a[:T], b[:T]) and torch.equal(a[:T], one)


# ----------------------------------------------------------------------- row mask
@pytest.mark.parametrize("C,ld", [(78, 83), (80, 96)])
@pytest.mark.parametrize("form", ["fp32", "bf16", "both"])
def test_row_mask(C, ld, form):
    from autoformer_amd import kernels as Kr

    B, T, lens = 3, 12, (12, 2, 7)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B * T, ld, generator=g)
    x.view(B, T, ld)[1, 5] = float("nan")                 # a padding row: overwritten, not multiplied
    xd = x.to(DEV)
    x16 = x.bfloat16()
    if form == "bf16":
        xd = x16.to(DEV)
    elif form == "both":
        Kr.attach_twin(xd, x16.to(DEV))
    out = Kr.row_mask(xd, Kr.Lens(lens, T, DEV), C=C)
    torch.cuda.synchronize()
    assert out is xd
    pad = torch.from_numpy(pad_rows(B, T, lens))
    checks = []
    if form != "bf16":
        checks.append((xd.cpu(), x))
    if form != "fp32":
        checks.append(((xd if form == "bf16" else xd._bf16).cpu(), x16))
    for got, before in checks:
        assert (got[pad][:, :C] == 0).all()
        keep = torch.ones(B * T, ld, dtype=torch.bool)
        keep[pad, :C] = False
        assert _same_bits(got[keep], before[keep])   # (bits: the NaN row's columns >= C stay NaN)


def _same_bits(a, b):
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def test_row_mask_full_lengths_write_nothing():
    from autoformer_amd import kernels as Kr

    x = torch.randn(2 * 8, 20, device=DEV)
    ref = x.clone()
    Kr.row_mask(x, Kr.Lens((8, 8), 8, DEV))
    assert torch.equal(x, ref)


# ----------------------------------------------------------------------- BiLSTM
def sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def bilstm_ref(xp, w, B, T, H, lens):
    """float64: h (B, T, 2H), zeros from lens[b] on; direction 1 runs lens[b] - 1 .. 0 from zero state."""
    G = 4 * H
    xp = np.asarray(xp, np.float64).reshape(B, T, 2 * G)
    w = np.asarray(w, np.float64)
    out = np.zeros((B, T, 2 * H))
    for b in range(B):
        for d in range(2):
            h, c = np.zeros(H), np.zeros(H)
            order = range(lens[b]) if d == 0 else range(lens[b] - 1, -1, -1)
            for t in order:
                pre = xp[b, t, d * G:(d + 1) * G] + w[d * G:(d + 1) * G] @ h
                i, f, g, o = sig(pre[:H]), sig(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), sig(pre[3 * H:])
                c = f * c + i * g
                h = o * np.tanh(c)
                out[b, t, d * H:(d + 1) * H] = h
    return out


def bilstm_inputs(H, B, T, lens, poison=True):
    G = 4 * H
    gen = torch.Generator().manual_seed(100 * T + H)
    xp = torch.randn(B, T, 2 * G, generator=gen) * 0.8
    w = (torch.rand(2 * G, H, generator=gen) * 2 - 1) / H ** 0.5
    if poison:
        for b in range(B):
            xp[b, lens[b]:] = float("nan")
    return xp, w


def _lstm_bars(comp):
    return (FP32_BAR, FP32_BAR) if comp == "fp32" else (FAST_BAR_RELF, FAST_BAR_RINF)


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [32, 44])
def test_bilstm_against_fp64(H, comp):
    import autoformer_amd as A
    from autoformer_amd import kernels as Kr

    A.set_compute(comp)
    B, T, lens = 3, 9, (9, 2, 5)
    xp, w = bilstm_inputs(H, B, T, lens)
    want = bilstm_ref(torch.nan_to_num(xp), w, B, T, H, lens)
    h = Kr.bilstm_ragged_fwd(xp.reshape(B * T, -1).to(DEV), w.to(DEV), Kr.Lens(lens, T, DEV), H, want_h16=True)
    torch.cuda.synchronize()
    got = host(h).reshape(B, T, 2 * H)
    e = (relf(got, want), rinf(got, want))
    print(f"H={H} {comp}: rel-Frobenius {e[0]:.2e} max-abs ratio {e[1]:.2e}")
    bar_f, bar_i = _lstm_bars(comp)
    assert np.isfinite(got).all() and e[0] < bar_f and e[1] < bar_i, e
    pad = pad_rows(B, T, lens)
    assert (got.reshape(B * T, -1)[pad] == 0.0).all()
    assert (h._bf16.cpu()[torch.from_numpy(pad)] == 0).all() and torch.equal(h._bf16, h.bfloat16())
    # the backward direction's first step is the utterance's own last frame: one LSTM step from zero state
    G = 4 * H
    for b in range(B):
        pre = xp[b, lens[b] - 1, G:].double().numpy()
        one = sig(pre[3 * H:]) * np.tanh(sig(pre[:H]) * np.tanh(pre[2 * H:3 * H]))
        assert np.abs(got[b, lens[b] - 1, H:] - one).max() < bar_i * np.abs(want).max(), b
    only16 = Kr.bilstm_ragged_fwd(xp.reshape(B * T, -1).to(DEV), w.to(DEV), Kr.Lens(lens, T, DEV), H, want_h32=False,
                                  want_h16=True)
    assert only16.dtype == torch.bfloat16 and torch.equal(only16, h._bf16)


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [32, 44])
def test_bilstm_full_lengths_match_lstm_fwd(H, comp):
    import autoformer_amd as A
    from autoformer_amd import kernels as Kr

    A.set_compute(comp)
    B, T = 3, 9
    xp, w = bilstm_inputs(H, B, T, (T,) * B, poison=False)
    xd, wd = xp.reshape(B * T, -1).to(DEV), w.to(DEV)
    h0, _, _ = Kr.lstm_fwd(xd, wd, B, T, H, 2)
    h1 = Kr.bilstm_ragged_fwd(xd, wd, Kr.Lens((T,) * B, T, DEV), H)
    torch.cuda.synchronize()
    e = (relf(host(h1), host(h0)), rinf(host(h1), host(h0)))
    print(f"H={H} {comp}: against avc_lstm_fwd rel-Frobenius {e[0]:.2e} max-abs ratio {e[1]:.2e}")
    bar_f, bar_i = _lstm_bars(comp)
    assert e[0] < bar_f and e[1] < bar_i, e


# ----------------------------------------------------------------------- refusals
def _refused(Lb, rc, needle):
    msg = Lb.avc_last_error().decode()
    assert rc != 0 and needle in msg, (rc, msg)


def test_refusals_leave_the_outputs_alone():
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    Lb = _lib.lib()
    B, T, C, H, S = 3, 12, 80, 32, -768.0
    ok = Kr.Lens((12, 2, 7), T, DEV)
    y = torch.randn(B * T, C, device=DEV)
    gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    o32 = torch.full((B * T, C), S, device=DEV)
    o16 = torch.full((B * T, C), S, device=DEV, dtype=torch.bfloat16)
    xp = torch.randn(B * T, 8 * H, device=DEV)
    w = torch.randn(8 * H, H, device=DEV)
    h32 = torch.full((B * T, 2 * H), S, device=DEV)
    st = Kr.stream()

    def arr(*v):
        return (ctypes.c_int * len(v))(*v)

    def bn(yp=y.data_ptr(), lens=ok.host, ldev=ok.dev.data_ptr(), c=C, o=o32.data_ptr()):
        return Lb.avc_bn_seg_ragged(yp, _lib.F32, C, B, T, c, lens, ldev, gam.data_ptr(), bet.data_ptr(), EPS, 1, None, o,
                                    o16.data_ptr(), None, None, st)

    def mask(lens=ok.host, ldev=ok.dev.data_ptr(), c=C, x=o32.data_ptr()):
        return Lb.avc_row_mask(x, o16.data_ptr(), C, B, T, c, lens, ldev, st)

    def rnn(xpp=xp.data_ptr(), lens=ok.host, ldev=ok.dev.data_ptr(), hh=H):
        return Lb.avc_bilstm_ragged_fwd(xpp, w.data_ptr(), lens, ldev, B, T, hh, h32.data_ptr(), None, _lib.F32, st)

    for fn, name in ((bn, "avc_bn_seg_ragged"), (mask, "avc_row_mask"), (rnn, "avc_bilstm_ragged_fwd")):
        _refused(Lb, fn(lens=arr(12, 1, 7)), "lens[1] = 1 outside 2..T")
        _refused(Lb, fn(lens=arr(13, 2, 7)), "lens[0] = 13 outside 2..T")
        _refused(Lb, fn(lens=None), name + ": null pointer")
        _refused(Lb, fn(ldev=None), name + ": null pointer")
    _refused(Lb, bn(yp=None), "null pointer")
    _refused(Lb, bn(c=0), "C = 0")
    _refused(Lb, mask(c=0), "C = 0")
    _refused(Lb, rnn(xpp=None), "null pointer")
    _refused(Lb, rnn(hh=65), "H = 65")
    _refused(Lb, Lb.avc_row_mask(None, None, C, B, T, C, ok.host, ok.dev.data_ptr(), st), "null pointer")
    torch.cuda.synchronize()
    assert (o32 == S).all() and (o16 == S).all() and (h32 == S).all()
    # the wrappers refuse a length outside 2..T before the library sees it
    with pytest.raises(ValueError, match="2..T"):
        Kr.Lens((12, 1, 7), T, DEV)
