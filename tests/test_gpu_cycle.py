"""The cycle step's fused loss tail (csrc/cycle_loss.hip) on the device against fp64 torch on the CPU:
F.cosine_embedding_loss, F.binary_cross_entropy and F.mse_loss with autograd.

Bars (1e-5, tests/test_gpu_critic.py's, and for its reasons): the losses relative; de per row against the row's
natural scale |g_c| / (B sqrt(m1_b)); dp relative, element by element; dy per element against the gradient's
natural scale |g| 2 max|y - x| / n_x (an element whose y - x is a cancellation has no relative error to speak of).
The cycle MSE of y = x is exactly 0 and is compared as such."""
import functools

import pytest
import torch
import torch.nn.functional as F

from .helpers import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5
LC, LD, LY = 0.1, 1.0, 0.7
# upstream gradients of (c_trans, c_reconst, d_loss, cycle, extra, total)
UP = (0.25, -0.75, -0.5, 0.5, 0.125, 1.5)
# (B, E, n_r, n_f, n_x, row stride)
SHAPES = [
    (1, 1, 1, 1, 1, None),                 # the smallest call
    (2, 256, 2, 2, 28160, None),           # the trainer's own shape
    (5, 255, 3, 7, 1023, None),            # odd sizes: the single-element form
    (5, 260, 300, 257, 4100, 264),         # strided rows, counts across the 256 boundary, five workgroups
    (4, 256, 4, 4, 266243, None),          # 256 workgroups (the cap), a second grid-stride trip, and a tail
    (64, 256, 64, 64, 901120, None),       # B = 64, T = 176: float4, three trips and a part of a fourth
]
IDS = ["%dx%d_%d_%d_%d" % s[:5] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def case(B, E, n_r, n_f, n_x, special=False):
    """Inputs (fp32, CPU) and the fp64 reference for the upstream gradients UP.  Computed once per shape and left
    unchanged."""
    g = torch.Generator().manual_seed(1000 * B + E + n_r + n_x)
    e1, t1, e2, t2 = (torch.randn(B, E, generator=g) for _ in range(4))
    pr = 0.02 + 0.96 * torch.rand(n_r, generator=g)
    pf = 0.02 + 0.96 * torch.rand(n_f, generator=g)
    x = torch.randn(n_x, generator=g)
    y = x + 0.5 * torch.randn(n_x, generator=g)
    if E == 1:
        # a one-element row's cosine is +-1, and +1 makes the loss a cancellation to 0 that no relative bar measures
        t1, t2 = -t1.abs() * e1.sign(), -t2.abs() * e2.sign()
    if special:
        for e, t in ((e1, t1), (e2, t2)):
            e[0] = t[0]            # parallel: true gradient about 0
            e[1] = -2 * t[1]        # antiparallel
            e[2] = 0                # the 1e-12 makes the loss 1 and the gradient about 1e6 / |t|
        for p in (pr, pf):
            p[:4] = torch.tensor([0.0, 1.0, 1e-30, 0.5])
        y = x.clone()               # cycle exactly 0, dy exactly 0
    base = torch.tensor(0.7310586)
    ones = torch.ones(B, dtype=torch.float64)
    e1d, e2d, prd, pfd, yd = (v.double().requires_grad_(True) for v in (e1, e2, pr, pf, y))
    c1 = F.cosine_embedding_loss(e1d, t1.double(), ones)
    c2 = F.cosine_embedding_loss(e2d, t2.double(), ones)
    d = F.binary_cross_entropy(prd, torch.ones_like(prd)) + F.binary_cross_entropy(pfd, torch.zeros_like(pfd))
    cyc = F.mse_loss(x.double(), yd)
    extra = LC * (c1 + c2) + LD * d + LY * cyc
    total = base.double() + extra
    sum(u * v for u, v in zip(UP, (c1, c2, d, cyc, extra, total))).backward()
    g_s = UP[4] + UP[5]
    ref = dict(out=[v.item() for v in (c1, c2, d, cyc, extra, total)], de1=e1d.grad, de2=e2d.grad, dr=prd.grad,
               df=pfd.grad, dy=yd.grad, m1=((e1.double() ** 2).sum(1) + 1e-12, (e2.double() ** 2).sum(1) + 1e-12),
               g_c=(LC * g_s + UP[0], LC * g_s + UP[1]), g_y=LY * g_s + UP[3],
               dmax=(y.double() - x.double()).abs().max().item())
    return (e1, t1, e2, t2, pr, pf, x, y, base), ref


def _place(v, ld=None, misalign=False):
    """v (B, E) on the device inside a NaN-poisoned buffer with row stride ld, optionally one float off 16-byte
    alignment."""
    B, E = v.shape
    ld = ld or E
    buf = torch.full((B * ld + 1,), float("nan"), device=DEV)
    off = 1 if misalign else 0
    view = buf[off:off + B * ld].view(B, ld)[:, :E]
    view.copy_(v)
    return view


def _flat(v, misalign=False):
    buf = torch.full((v.numel() + 1,), float("nan"), device=DEV)
    off = 1 if misalign else 0
    view = buf[off:off + v.numel()]
    view.copy_(v)
    return view


def _up(vals=UP):
    return [None if v is None else torch.tensor(v, device=DEV) for v in vals]


def _run(inputs, ld=None, misalign=False, need=(True,) * 5, d=None, use_base=True):
    """(out, de1, de2, dp_real, dp_fake, dy, the rows' part of ws)."""
    from autoformer_amd import kernels as K

    e1, t1, e2, t2, pr, pf, x, y, base = inputs
    rows = [_place(v, ld, misalign) for v in (e1, t1, e2, t2)]
    prd, pfd, bd = pr.to(DEV), pf.to(DEV), base.to(DEV)
    xd, yd = _flat(x, misalign), _flat(y, misalign)
    out, ws = K.cycle_loss(*rows, prd, pfd, xd, yd, LC, LD, LY, base=bd if use_base else None)
    grads = K.cycle_loss_grad(*rows, prd, pfd, xd, yd, LC, LD, LY, ws, _up() if d is None else d, need)
    torch.cuda.synchronize()
    return (out, *grads, ws[:6 * e1.shape[0]])


def _check(inputs, ref, got, what):
    out, de1, de2, dr, df, dy, _ = got
    o = out.double().cpu()
    for k, name in enumerate(("c_trans", "c_reconst", "d_loss", "cycle", "extra", "total")):
        r = ref["out"][k]
        if r == 0.0:
            print(f"{what} {name}: {o[k].item():.9g} vs exactly 0")
            assert o[k].item() == 0.0, (what, name)
            continue
        err = abs(o[k].item() - r) / abs(r)
        print(f"{what} {name}: {o[k].item():.9g} vs {r:.9g} rel {err:.2e}")
        assert err <= BAR, (what, name, err)
    B = inputs[0].shape[0]
    for k, (de, name) in enumerate(((de1, "de1"), (de2, "de2"))):
        scale = abs(ref["g_c"][k]) / (B * ref["m1"][k].sqrt())
        row_err = (de.double().cpu() - ref[name]).abs().max(1).values / scale
        print(f"{what} {name}: worst row {row_err.max().item():.2e} of scale (row {row_err.argmax().item()})")
        assert row_err.max().item() <= BAR, (what, name, row_err)
    for name, g, r in (("dp_real", dr, ref["dr"]), ("dp_fake", df, ref["df"])):
        err = ((g.double().cpu() - r).abs() / r.abs().clamp_min(1e-300))[r != 0]
        worst = err.max().item() if err.numel() else 0.0
        print(f"{what} {name}: worst rel {worst:.2e}")
        assert worst <= BAR, (what, name, worst)
        assert bool((g.cpu()[r == 0] == 0).all()), (what, name)
    n_x = inputs[6].numel()
    scale = abs(ref["g_y"]) * 2 * ref["dmax"] / n_x
    if scale == 0.0:
        assert bool((dy == 0).all()), what                                          # y = x: exactly 0
        print(f"{what} dy: exactly 0")
    else:
        err = ((dy.double().cpu() - ref["dy"]).abs().max() / scale).item()
        print(f"{what} dy: worst {err:.2e} of scale")
        assert err <= BAR, (what, err)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_losses_and_gradients_match_fp64(shape):
    B, E, n_r, n_f, n_x, ld = shape
    inputs, ref = case(B, E, n_r, n_f, n_x)
    got = _run(inputs, ld)
    _check(inputs, ref, got, IDS[SHAPES.index(shape)])
    again = _run(inputs, ld)
    for a, b in zip(got, again):                                                   # two calls: identical bits
        assert bits_equal(a, b)


def test_special_rows_probabilities_and_an_exact_cycle():
    """Rows e = t, e = -2t, e = 0; probabilities 0, 1, 1e-30, 0.5; y = x: cycle exactly 0 and dy exactly 0."""
    inputs, ref = case(6, 256, 9, 9, 1500, special=True)
    got = _run(inputs)
    _check(inputs, ref, got, "special")
    assert got[0][3].item() == 0.0 and bool((got[5] == 0).all())
    for de in (got[1].cpu(), got[2].cpu()):
        zero_row = de[2].abs().max().item()
        assert 1e3 < zero_row < 1e6 and torch.isfinite(de).all()


def test_float4_and_scalar_forms_give_the_same_bits():
    """The same data read as float4 (aligned, E % 4 == 0, n_x % 4 == 0) and as single elements (every base one
    float off; rows also at an odd stride), one workgroup to the capped grid with several trips."""
    for B, E, n, n_x in ((5, 260, 300, 4100), (2, 256, 2, 28160), (4, 256, 4, 266244), (64, 256, 64, 901120)):
        inputs, _ = case(B, E, n, n + 1, n_x)
        vec = _run(inputs)
        for a, b in zip(vec, _run(inputs, misalign=True)):
            assert bits_equal(a, b), (B, E, n_x)
        for a, b in zip(vec, _run(inputs, ld=E + 3)):                              # an odd stride: rows scalar, x float4
            assert bits_equal(a, b), (B, E, n_x)


def test_the_shared_terms_carry_the_critic_kernels_bits():
    """out[0], out[2], de1, dp_real, dp_fake against avc_critic_loss / avc_critic_loss_grad on (e1, t1, p_real,
    p_fake) with the same upstream gradients; the second pair against the same kernels on (e2, t2)."""
    from autoformer_amd import kernels as K

    for shape in ((5, 255, 3, 7, 1023), (5, 260, 300, 257, 4100), (64, 256, 64, 64, 901120)):
        inputs, _ = case(*shape)
        e1, t1, e2, t2, pr, pf = (v.to(DEV) for v in inputs[:6])
        out, de1, de2, dr, df, _, _ = _run(inputs)
        u = _up()
        for e, t, k, de in ((e1, t1, 0, de1), (e2, t2, 1, de2)):
            c_out, c_ws = K.critic_loss(e, t, pr, pf, LC, LD)
            c_de, c_dr, c_df = K.critic_loss_grad(e, t, pr, pf, LC, LD, c_ws, [u[k], u[2], u[4], u[5]], (True,) * 3)
            assert bits_equal(out[k:k + 1], c_out[0:1]) and bits_equal(out[2:3], c_out[1:2]), shape
            assert bits_equal(de, c_de) and bits_equal(dr, c_dr) and bits_equal(df, c_df), shape


def test_padding_is_untouched_and_unread():
    """Row stride 264 over E = 260: the NaN padding reaches no loss, and both de's own padding keeps its bits."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    inputs, _ = case(5, 260, 300, 257, 4100)
    e1, t1, e2, t2, pr, pf, x, y, _ = inputs
    rows = [_place(v, 264) for v in (e1, t1, e2, t2)]
    prd, pfd, xd, yd = pr.to(DEV), pf.to(DEV), x.to(DEV), y.to(DEV)
    out, ws = K.cycle_loss(*rows, prd, pfd, xd, yd, LC, LD, LY)
    assert torch.isfinite(out).all()
    bufs = [torch.full((5, 264), float("nan"), device=DEV) for _ in range(2)]
    one = torch.ones((), device=DEV)
    ptrs = []
    for v in rows:
        ptrs += [v.data_ptr(), 264]
    L.call("avc_cycle_loss_grad", *ptrs, 5, 260, prd.data_ptr(), 300, pfd.data_ptr(), 257, xd.data_ptr(), yd.data_ptr(),
           4100, LC, LD, LY, ws.data_ptr(), None, None, None, None, None, one.data_ptr(), bufs[0].data_ptr(), 264,
           bufs[1].data_ptr(), 264, None, None, None, K.stream())
    torch.cuda.synchronize()
    tight = K.cycle_loss_grad(*rows, prd, pfd, xd, yd, LC, LD, LY, ws, [None] * 5 + [one],
                              (True, True, False, False, False))
    for buf, t in zip(bufs, tight[:2]):
        assert torch.isfinite(buf[:, :260]).all() and torch.isnan(buf[:, 260:]).all()
        assert bits_equal(buf[:, :260].contiguous(), t)


def test_optional_outputs_and_gradients_leave_the_rest_alone():
    inputs, _ = case(5, 255, 3, 7, 1023)
    full = _run(inputs)
    for need in ((True, False, False, False, False), (False, True, False, False, False),
                 (False, False, True, False, False), (False, False, False, True, False),
                 (False, False, False, False, True), (True, False, False, True, True)):
        part = _run(inputs, need=need)
        for k, on in enumerate(need):
            assert (part[1 + k] is None) == (not on)
            if on:
                assert bits_equal(part[1 + k], full[1 + k]), need
    # an absent upstream gradient is a zero one
    for absent in ((None, -0.75, None, 0.5, None, 1.5), (0.25, None, -0.5, None, 0.125, None)):
        explicit = tuple(0.0 if v is None else v for v in absent)
        for a, b in zip(_run(inputs, d=_up(absent))[1:6], _run(inputs, d=_up(explicit))[1:6]):
            assert bits_equal(a, b)
    # each gradient depends on its own term's upstream only (and on extra's and total's)
    for k, outs in ((0, (2, 3, 4, 5)), (1, (1, 3, 4, 5)), (2, (1, 2, 5)), (3, (1, 2, 3, 4))):
        vals = list(UP)
        vals[k] = None
        other = _run(inputs, d=_up(vals))
        for j in outs:
            assert bits_equal(other[j], full[j]), (k, j)


def test_base_adds_exactly():
    inputs, _ = case(4, 256, 4, 4, 266243)
    with_base, without = _run(inputs)[0].cpu(), _run(inputs, use_base=False)[0].cpu()
    assert bits_equal(with_base[:5], without[:5])
    assert without[5].item() == without[4].item()
    assert with_base[5].item() == (inputs[8] + without[4]).item()                   # one fp32 addition


def test_refusals_launch_nothing():
    """-1 through the binding (a RuntimeError with the library's message), and the outputs keep their bits."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    inputs, _ = case(5, 255, 3, 7, 1023)
    e1, t1, e2, t2, pr, pf, x, y, _ = (v.to(DEV) for v in inputs)
    out = torch.full((6,), float("nan"), device=DEV)
    ws = torch.full((int(L.lib().avc_cycle_loss_ws(5, 1023)) // 4,), float("nan"), device=DEV)
    dy = torch.full((1023,), float("nan"), device=DEV)
    rows = (e1.data_ptr(), 255, t1.data_ptr(), 255, e2.data_ptr(), 255, t2.data_ptr(), 255)
    tail = (pr.data_ptr(), 3, pf.data_ptr(), 7, x.data_ptr(), y.data_ptr())
    lib = L.lib()
    for B, E, n_x, what in ((0, 255, 1023, "bad shape B = 0"), (5, 256, 1023, "lde1 = 255 is below E = 256"),
                            (5, 255, 0, "n_x = 0"), (5, 255, 2 ** 31, "n_x = 2147483648")):
        rc = lib.avc_cycle_loss(*rows, B, E, *tail, n_x, None, LC, LD, LY, out.data_ptr(), ws.data_ptr(), K.stream())
        assert rc == -1 and what in lib.avc_last_error().decode(), what
        rc = lib.avc_cycle_loss_grad(*rows, B, E, *tail, n_x, LC, LD, LY, ws.data_ptr(), None, None, None, None, None,
                                     None, None, 0, None, 0, None, None, dy.data_ptr(), K.stream())
        assert rc == -1 and what in lib.avc_last_error().decode(), what
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all() and torch.isnan(dy).all()
    with pytest.raises(ValueError, match="one shape"):
        K.cycle_loss(e1, t1, e2[:4], t2[:4], pr, pf, x, y, LC, LD, LY)
    with pytest.raises(ValueError, match="same 1 <= n_x"):
        K.cycle_loss(e1, t1, e2, t2, pr, pf, x, y[:-1], LC, LD, LY)


def test_autograd_block():
    """cycle_loss_block: the gradients reach both styles, real, fake, x_rec and base; the targets and x_source get
    none; a loss part used alone drives only its own inputs."""
    from autoformer_amd.cycle import cycle_loss_block

    inputs, ref = case(5, 255, 3, 7, 1023)
    e1, t1, e2, t2, pr, pf, x, y, base = (v.to(DEV).requires_grad_(True) for v in inputs)
    total, c1, c2, d, cyc = cycle_loss_block(e1, t1, e2, t2, pr.view(-1, 1), pf.view(-1, 1), x.view(3, 341),
                                             y.view(3, 341), LC, LD, LY, base=base)
    extra = total - base
    sum(u * v for u, v in zip(UP, (c1, c2, d, cyc, extra, total))).backward()
    got = (torch.stack([c1, c2, d, cyc, extra, total]).detach(), e1.grad, e2.grad, pr.grad, pf.grad, y.grad, None)
    _check(inputs, ref, got, "autograd")
    assert t1.grad is None and t2.grad is None and x.grad is None
    assert abs(base.grad.item() - UP[5]) < 1e-6         # total's upstream, less extra's through extra = total - base
    leaves = [v.detach().clone().requires_grad_(True) for v in (e1, e2, pr, pf, y)]
    a, b, p, q, w = leaves
    for k, driven in ((1, (0,)), (2, (1,)), (3, (2, 3)), (4, (4,))):
        for v in leaves:
            v.grad = None
        cycle_loss_block(a, t1.detach(), b, t2.detach(), p, q, x.detach(), w, LC, LD, LY)[k].backward()
        assert [i for i, v in enumerate(leaves) if v.grad is not None] == list(driven), k
