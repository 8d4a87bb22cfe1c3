"""The critic step's fused loss tail (csrc/critic_loss.hip) on the device against fp64 torch on the CPU:
F.cosine_embedding_loss and F.binary_cross_entropy with autograd.

Bars (1e-5, the bar tests/test_gpu_xent.py holds its kernel to): the losses relative; de per row against the
row's natural scale |g_c| / (B sqrt(m1_b)) -- every term of the row's gradient is at most that, and a rel-inf over
the whole tensor would let the zero row (gradient about 1e6 / |t|) hide every other row, while the parallel rows'
true gradient is a cancellation to about 1e-18; dp relative, element by element.  The fp32 formula evaluated on
the CPU sits at 1e-7 to 2e-7 of that scale on generic rows and 2e-9 on the parallel rows."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .helpers import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5
LC, LD = 0.1, 1.0
# (B, E, n_r, n_f, lde, misalign)
SHAPES = [
    (1, 1, 1, 1, None, False),          # smallest
    (2, 256, 2, 2, None, False),        # the training shape
    (4, 256, 4, 4, None, False),        # one row per wave
    (5, 255, 3, 7, None, False),        # odd sizes: the scalar form
    (5, 260, 300, 257, 264, False),     # padded strides, counts across the 256 boundary
    (9, 4096, 1, 513, None, False),     # E at the cap
    (64, 256, 64, 64, None, False),     # the benchmark shape
    (130, 68, 1000, 999, None, True),   # many rows per wave; a misaligned base forces the scalar form
]
IDS = ["%dx%d_%d_%d" % s[:4] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def case(B, E, n_r, n_f, special=False):
    """Inputs (fp32, CPU) and the fp64 reference for upstream gradients (g_total, g_closs, g_dloss) = (1.5, 0.25,
    -0.5): losses, de, dp_real, dp_fake, and m1 per row.  Computed once per shape and left unchanged."""
    g = torch.Generator().manual_seed(1000 * B + E + n_r)
    e, t = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    pr = 0.02 + 0.96 * torch.rand(n_r, generator=g)
    pf = 0.02 + 0.96 * torch.rand(n_f, generator=g)
    if E == 1:
        # a one-element row's cosine is +-1, and +1 makes c_loss a cancellation to 0 that no relative bar measures
        t = -t.abs() * e.sign()
    if special:
        e[0] = t[0]           # parallel: true gradient about 0
        e[1] = -2 * t[1]       # antiparallel
        e[2] = 0               # the 1e-12 makes the loss 1 and the gradient about 1e6 / |t|
        for p in (pr, pf):
            p[:4] = torch.tensor([0.0, 1.0, 1e-30, 0.5])
    base = torch.tensor(0.7310586)
    e64, pr64, pf64 = (v.double().requires_grad_(True) for v in (e, pr, pf))
    c = F.cosine_embedding_loss(e64, t.double(), torch.ones(B, dtype=torch.float64))
    d = F.binary_cross_entropy(pr64, torch.ones_like(pr64)) + F.binary_cross_entropy(pf64, torch.zeros_like(pf64))
    extra = LC * c + LD * d
    total = base.double() + extra
    (1.5 * total + 0.25 * c - 0.5 * d).backward()
    ref = dict(c=c.item(), d=d.item(), extra=extra.item(), total=total.item(), de=e64.grad, dr=pr64.grad, df=pf64.grad,
               m1=(e.double() ** 2).sum(1) + 1e-12, g_c=LC * 1.5 + 0.25)
    return (e, t, pr, pf, base), ref


def _place(v, ld=None, misalign=False):
    """v (B, E) on the device inside a NaN-poisoned buffer with row stride ld, optionally one float off 16-byte
    alignment; returns (view, whole buffer)."""
    B, E = v.shape
    ld = ld or E
    buf = torch.full((B * ld + 1,), float("nan"), device=DEV)
    off = 1 if misalign else 0
    view = buf[off:off + B * ld].view(B, ld)[:, :E]
    view.copy_(v)
    return view, buf


def _run(inputs, ld=None, misalign=False, need=(True, True, True), d=None, use_base=True):
    from autoformer_amd import kernels as K

    e, t, pr, pf, base = inputs
    ed, _ = _place(e, ld, misalign)
    td, _ = _place(t, ld, misalign)
    prd, pfd, bd = pr.to(DEV), pf.to(DEV), base.to(DEV)
    out, ws = K.critic_loss(ed, td, prd, pfd, LC, LD, base=bd if use_base else None)
    if d is None:
        d = [torch.tensor(v, device=DEV) for v in (0.25, -0.5)] + [None, torch.tensor(1.5, device=DEV)]
    de, dr, df = K.critic_loss_grad(ed, td, prd, pfd, LC, LD, ws, d, need)
    torch.cuda.synchronize()
    return out, de, dr, df, ws[:3 * e.shape[0]]                                    # (the rounding-up of ws is unwritten)


def _check(inputs, ref, got, what):
    out, de, dr, df, _ = got
    o = out.double().cpu()
    for k, name in enumerate(("c", "d", "extra", "total")):
        err = abs(o[k].item() - ref[name]) / abs(ref[name])
        print(f"{what} {name}: {o[k].item():.9g} vs {ref[name]:.9g} rel {err:.2e}")
        assert err <= BAR, (what, name, err)
    B = inputs[0].shape[0]
    scale = abs(ref["g_c"]) / (B * ref["m1"].sqrt())
    row_err = ((de.double().cpu() - ref["de"]).abs().max(1).values / scale)
    print(f"{what} de: worst row {row_err.max().item():.2e} of scale (row {row_err.argmax().item()})")
    assert row_err.max().item() <= BAR, (what, row_err)
    for name, g, r in (("dp_real", dr, ref["dr"]), ("dp_fake", df, ref["df"])):
        err = ((g.double().cpu() - r).abs() / r.abs().clamp_min(1e-300))[r != 0]
        worst = err.max().item() if err.numel() else 0.0
        print(f"{what} {name}: worst rel {worst:.2e}")
        assert worst <= BAR, (what, name, worst)
        assert bool((g.cpu()[r == 0] == 0).all()), (what, name)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_losses_and_gradients_match_fp64(shape):
    B, E, n_r, n_f, ld, mis = shape
    inputs, ref = case(B, E, n_r, n_f)
    got = _run(inputs, ld, mis)
    _check(inputs, ref, got, IDS[SHAPES.index(shape)])
    again = _run(inputs, ld, mis)
    for a, b in zip(got, again):                                                   # two calls: identical bits
        assert bits_equal(a, b)


def test_special_rows_and_probabilities():
    inputs, ref = case(6, 256, 9, 9, special=True)
    got = _run(inputs)
    _check(inputs, ref, got, "special")
    de = got[1].cpu()
    zero_row = de[2].abs().max().item()
    print("special: |de| of the zero row %.4g, of the parallel row %.3g" % (zero_row, de[0].abs().max().item()))
    assert 1e3 < zero_row < 1e6 and torch.isfinite(de).all()


def test_float4_and_scalar_forms_give_the_same_bits():
    """The same data read as float4 (aligned, E % 4 == 0) and as single elements (base one float off)."""
    for B, E, n in ((5, 260, 300), (64, 256, 64), (9, 4096, 1)):
        inputs, _ = case(B, E, n, n + 1)
        for a, b in zip(_run(inputs), _run(inputs, misalign=True)):
            assert bits_equal(a, b), (B, E)
        for a, b in zip(_run(inputs), _run(inputs, ld=E + 3)):                     # an odd stride: scalar again
            assert bits_equal(a, b), (B, E)


def test_padding_is_untouched_and_unread():
    """Row stride 264 over E = 260: the NaN padding reaches no loss, and de's own padding keeps its bits."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    inputs, ref = case(5, 260, 300, 257)
    e, t, pr, pf, base = inputs
    ed, _ = _place(e, 264)
    td, _ = _place(t, 264)
    prd, pfd = pr.to(DEV), pf.to(DEV)
    out, ws = K.critic_loss(ed, td, prd, pfd, LC, LD)
    assert torch.isfinite(out).all()
    de_buf = torch.full((5, 264), float("nan"), device=DEV)
    one = torch.ones((), device=DEV)
    L.call("avc_critic_loss_grad", ed.data_ptr(), 264, td.data_ptr(), 264, 5, 260, prd.data_ptr(), 300, pfd.data_ptr(),
           257, LC, LD, ws.data_ptr(), None, None, None, one.data_ptr(), de_buf.data_ptr(), 264, None, None, K.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(de_buf[:, :260]).all() and torch.isnan(de_buf[:, 260:]).all()
    tight = K.critic_loss_grad(ed, td, prd, pfd, LC, LD, ws, [None, None, None, one], (True, False, False))[0]
    assert bits_equal(de_buf[:, :260].contiguous(), tight)


def test_optional_outputs_and_gradients_leave_the_rest_alone():
    inputs, _ = case(5, 255, 3, 7)
    full = _run(inputs)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        part = _run(inputs, need=need)
        for k, on in enumerate(need):
            assert (part[1 + k] is None) == (not on)
            if on:
                assert bits_equal(part[1 + k], full[1 + k]), need
    z = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
    # an absent upstream gradient is a zero one
    for absent, explicit in (([None, z(-0.5), None, z(1.5)], [z(0.0), z(-0.5), z(0.0), z(1.5)]),
                             ([z(0.25), None, z(2.0), None], [z(0.25), z(0.0), z(2.0), z(0.0)])):
        for a, b in zip(_run(inputs, d=absent)[1:4], _run(inputs, d=explicit)[1:4]):
            assert bits_equal(a, b)
    # de does not depend on g_dloss, dp not on g_closs
    assert bits_equal(_run(inputs, d=[z(0.25), None, None, z(1.5)])[1], full[1])
    other = _run(inputs, d=[None, z(-0.5), None, z(1.5)])
    assert bits_equal(other[2], full[2]) and bits_equal(other[3], full[3])


def test_base_adds_exactly():
    inputs, _ = case(4, 256, 4, 4)
    with_base, without = _run(inputs)[0].cpu(), _run(inputs, use_base=False)[0].cpu()
    assert bits_equal(with_base[:3], without[:3])
    assert without[3].item() == without[2].item()
    assert with_base[3].item() == (inputs[4] + without[2]).item()                   # one fp32 addition


def test_autograd_block():
    """critic_loss_block: the gradients reach trans_style, real, fake and base; target_style gets none; a loss
    part used alone drives only its own inputs."""
    from autoformer_amd.critic import critic_loss_block

    inputs, ref = case(5, 255, 3, 7)
    e, t, pr, pf, base = (v.to(DEV) for v in inputs)
    e, pr, pf, base = (v.requires_grad_(True) for v in (e, pr, pf, base))
    t.requires_grad_(True)
    total, c, d = critic_loss_block(e, t, pr.view(-1, 1), pf.view(-1, 1), LC, LD, base=base)
    (1.5 * total + 0.25 * c - 0.5 * d).backward()
    got = (torch.stack([c, d, total - base, total]).detach(), e.grad, pr.grad, pf.grad, None)
    _check(inputs, dict(ref, extra=ref["extra"]), got, "autograd")
    assert t.grad is None and abs(base.grad.item() - 1.5) < 1e-6
    e2, pr2, pf2 = (v.detach().clone().requires_grad_(True) for v in (e, pr, pf))
    _, c2, _ = critic_loss_block(e2, t.detach(), pr2, pf2, LC, LD)
    c2.backward()
    assert e2.grad is not None and pr2.grad is None and pf2.grad is None
