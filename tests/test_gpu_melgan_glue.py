"""The MelGAN generator's glue kernels (csrc/melgan.hip: avc_mg_gather, avc_mg_act, avc_mg_wn_pack,
avc_mg_conv_out), each called through _lib.call and compared with a float64 computation on the CPU
(F.pad / F.conv1d / F.conv_transpose1d / the weight_norm formula) from the same inputs.

Bars: a gather without activation is data movement (bit-exact; a bf16 output equals torch's .to(bfloat16));
LeakyReLU is one fp32 rounding (k = 1), and its bf16 copy one more round-to-nearest to bf16 (2^-8);
the weight-norm pack and the output convolution are fp32 sums, |err| <= d * 2^-24 * sum|terms|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .helpers import BF16_ULP, EPS32, bits_equal, close_ratio, f64, report, roundings_ratio, sum_ratio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = float(np.float32(0.2))  # the slope as the kernels receive it
# LeakyReLU in fp32 then round-to-nearest to bf16 (8 significand bits: unit roundoff 2^-8):
# (1 + 2^-24)(1 + 2^-8) - 1 < 2^-8 + 2^-23
LEAKY_BF16 = BF16_ULP + 2 * EPS32


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _tdt(bf):
    return torch.bfloat16 if bf else torch.float32


def _leaky(x64):
    return torch.where(x64 >= 0, x64, x64 * SLOPE)


# ------------------------------------------------------------------------------------- mg_gather
# (B, L, C, taps, dil, pad): L = pad + 1, so every output frame reads a reflected one (the last residual
# block's dilation 9); the 7-tap input / output convolutions with C / 4 = 9 channel quads; a minimal 3-tap
@pytest.mark.parametrize("B,L,C,taps,dil,pad", [(2, 10, 4, 3, 9, 9), (1, 7, 36, 7, 1, 3), (3, 5, 8, 3, 1, 1)])
@pytest.mark.parametrize("reflect", [1, 0])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("in_bf,out_bf", [(False, False), (False, True), (True, False), (True, True)])
def test_mg_gather(B, L, C, taps, dil, pad, reflect, act, in_bf, out_bf):
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    x = _rand(B, L, C, seed=L + C).to(_tdt(in_bf))
    Lo = L + 2 * pad - dil * (taps - 1)
    out = torch.full((B * Lo, taps * C), 7.0, device=DEV, dtype=_tdt(out_bf))
    xd = x.to(DEV)
    L_.call("avc_mg_gather", xd.data_ptr(), int(in_bf), B, L, C, taps, dil, pad, reflect, act, SLOPE, out.data_ptr(),
            int(out_bf), K.stream())
    # reference: pad the (B, C, L) sequence, then one slice per tap, tap-major columns
    x64 = x.double()
    a64 = _leaky(x64) if act else x64
    xp = F.pad(a64.transpose(1, 2), (pad, pad), mode="reflect" if reflect else "constant")
    ref = torch.cat([xp[:, :, k * dil:k * dil + Lo].transpose(1, 2) for k in range(taps)], -1).reshape(B * Lo, taps * C)
    what = f"({B},{L},{C},{taps},{dil},{pad}) reflect={reflect} act={act} {in_bf}->{out_bf}"
    if not act:
        # every element is a copy of an input element (or 0): float64 holds it exactly
        assert bits_equal(out, ref.float().to(_tdt(out_bf))), what
    elif not out_bf:
        assert report("mg_gather", what, roundings_ratio(out, ref, 1)) <= 1.0  # k = 1: v * slope
    else:
        assert report("mg_gather", what, close_ratio(out, ref, LEAKY_BF16, 0.0)) <= 1.0


# ---------------------------------------------------------------------------------------- mg_act
@pytest.mark.parametrize("n", [4, 1028])
@pytest.mark.parametrize("outs", ["f32", "bf16", "both"])
def test_mg_act(n, outs):
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    x = _rand(n, seed=n)
    ref = _leaky(x.double())
    xd = x.to(DEV)
    o = torch.full((n,), 7.0, device=DEV) if outs != "bf16" else None
    o16 = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16) if outs != "f32" else None
    L_.call("avc_mg_act", xd.data_ptr(), n, SLOPE, K._ptr(o), K._ptr(o16), K.stream())
    if o is not None:
        assert report("mg_act", f"n={n} fp32", roundings_ratio(o, ref, 1)) <= 1.0  # k = 1
    if o16 is not None:
        assert report("mg_act", f"n={n} bf16", close_ratio(o16, ref, LEAKY_BF16, 0.0)) <= 1.0
    if o is not None and o16 is not None:
        assert bits_equal(o16, o.to(torch.bfloat16))


# ------------------------------------------------------------------------------------ mg_wn_pack
def _norm_k(n):
    """mg_norm_kernel sums n squares: ceil(n / 256) serial adds per thread, the 6-level wave tree, 3 adds over
    the waves, and the square's own rounding: d.  All terms are positive, so the sum's relative error is
    <= d * 2^-24; the square root halves it and rounds once: k = d / 2 + 1."""
    return (-(-n // 256) + 6 + 3 + 1) / 2 + 1


def _wn_call(v, g, bias, d0, d1, Kw, stride, pad, out_bf):
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    rows, cols = (stride * d1, 3 * d0) if stride else (d0, Kw * d1)
    norms = torch.full((d0,), 7.0, device=DEV)
    out = torch.full((rows, cols), 7.0, device=DEV, dtype=_tdt(out_bf))
    bias_out = torch.full((rows,), 7.0, device=DEV) if stride else None
    vd, gd = v.to(DEV), g.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    L_.call("avc_mg_wn_pack", vd.data_ptr(), gd.data_ptr(), K._ptr(bd), d0, d1, Kw, stride, pad, norms.data_ptr(),
            out.data_ptr(), int(out_bf), K._ptr(bias_out), K.stream())
    return norms, out, bias_out


def _check_pack(what, norms, out, v, ref, out_bf, n):
    kn = _norm_k(n)
    assert report("mg_wn_pack", f"{what} norms", roundings_ratio(norms, v.double().flatten(1).norm(dim=1), kn)) <= 1.0
    zeros = out.cpu()[ref == 0]
    assert bits_equal(zeros, torch.zeros_like(zeros)), "structural zeros of the pack"
    # w = g * v / norm: the norm's kn roundings, one product, one division
    if out_bf:
        assert report("mg_wn_pack", f"{what} bf16", close_ratio(out, ref, BF16_ULP + (kn + 3) * EPS32, 0.0)) <= 1.0
    else:
        assert report("mg_wn_pack", f"{what} fp32", roundings_ratio(out, ref, kn + 2)) <= 1.0


@pytest.mark.parametrize("d0,d1,Kw", [(5, 6, 3), (3, 100, 7)])
@pytest.mark.parametrize("out_bf", [False, True])
def test_mg_wn_pack_conv(d0, d1, Kw, out_bf):
    """Conv1d v [Co][Ci][K] -> [Co][K*Ci], tap-major; (3, 100, 7): a slice of 700 elements, three passes of
    the norm's 256-thread loop."""
    v, g = _rand(d0, d1, Kw, seed=d1), _rand(d0, seed=d1 + 1)
    norms, out, _ = _wn_call(v, g, None, d0, d1, Kw, 0, 0, out_bf)
    v64 = v.double()
    w64 = g.double().view(-1, 1, 1) * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
    ref = w64.permute(0, 2, 1).reshape(d0, Kw * d1)
    _check_pack(f"conv ({d0},{d1},{Kw})", norms, out, v, ref, out_bf, d1 * Kw)


@pytest.mark.parametrize("r", [2, 8])
@pytest.mark.parametrize("out_bf", [False, True])
@pytest.mark.parametrize("with_bias", [True, False])
def test_mg_wn_pack_transposed(r, out_bf, with_bias):
    """ConvTranspose1d v [Ci][Co][2r], padding r/2 + r%2 -> the polyphase [r*Co][3*Ci] pack and the phase-major
    bias, assembled as tests/test_melgan.py test_polyphase_conv_transpose_decomposition builds Wp; A @ pack^T
    over the zero-padded 3-tap window must then equal F.conv_transpose1d."""
    Ci, Co, Kw, pad, L = 6, 5, 2 * r, r // 2 + r % 2, 9
    v, g, bias = _rand(Ci, Co, Kw, seed=r), _rand(Ci, seed=r + 1), _rand(Co, seed=r + 2)
    norms, out, bias_out = _wn_call(v, g, bias if with_bias else None, Ci, Co, Kw, r, pad, out_bf)
    v64 = v.double()
    w = g.double().view(-1, 1, 1) * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
    Wp = torch.zeros(r * Co, 3 * Ci, dtype=torch.float64)
    for p in range(r):
        dl, rho = (p + pad) // r, (p + pad) % r
        for co in range(Co):
            Wp[p * Co + co, (dl + 1) * Ci:(dl + 2) * Ci] = w[:, co, rho]
            Wp[p * Co + co, dl * Ci:(dl + 1) * Ci] = w[:, co, rho + r]
    _check_pack(f"transposed r={r}", norms, out, v, Wp, out_bf, Co * Kw)
    assert bits_equal(bias_out, (bias if with_bias else torch.zeros(Co)).repeat(r))
    if not out_bf:
        x = _rand(2, Ci, L, seed=r + 3).double()
        ref = F.conv_transpose1d(x, w, stride=r, padding=pad, output_padding=r % 2)
        xf = F.pad(x, (1, 1)).transpose(1, 2)
        A = torch.cat([xf[:, t:t + L] for t in range(3)], -1)
        got = (A @ f64(out).T).reshape(2, L * r, Co).transpose(1, 2)
        # the product itself is float64: the error is the pack's, kn + 2 roundings per weight
        sabs = (A.abs() @ Wp.abs().T).reshape(2, L * r, Co).transpose(1, 2)
        assert report("mg_wn_pack", f"transposed r={r} product", sum_ratio(got, ref, sabs, _norm_k(Co * Kw) + 2)) <= 1.0


# ----------------------------------------------------------------------------------- mg_conv_out
@pytest.mark.parametrize("B,L,C", [(2, 4, 4), (1, 300, 32)])
def test_mg_conv_out(B, L, C):
    """L = 4 = pad + 1: both edges reflect in every window; (1, 300, 32): a second block of 256 samples."""
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    x, w, bias = _rand(B, L, C, seed=C), _rand(7, C, seed=C + 1, scale=0.2), _rand(1, seed=C + 2, scale=0.1)
    out = torch.full((B * L,), 7.0, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    L_.call("avc_mg_conv_out", xd.data_ptr(), B, L, C, 7, wd.data_ptr(), bd.data_ptr(), SLOPE, out.data_ptr(), K.stream())
    a = F.pad(_leaky(x.double()).transpose(1, 2), (3, 3), mode="reflect")
    wc = w.double().t().unsqueeze(0)  # [7][C] -> Conv1d weight (1, C, 7)
    pre = F.conv1d(a, wc, bias.double())
    sabs = F.conv1d(a.abs(), wc.abs(), bias.double().abs())
    ref = torch.tanh(pre).reshape(B * L)
    # the accumulator takes 7*C dependent additions, each product carries its own rounding and LeakyReLU's:
    # d = 7*C + 2 on the pre-activation; tanh is 1-Lipschitz and has the transcendental bar (rtol 1e-5, atol 1e-6)
    err = (f64(out) - ref).abs()
    bar = (7 * C + 2) * EPS32 * sabs.reshape(B * L) + 1e-5 * ref.abs() + 1e-6
    assert report("mg_conv_out", f"({B},{L},{C})", float((err / bar).max())) <= 1.0
