"""The elementwise, loss, optimizer and layout-glue entry points of csrc/elem.hip, csrc/variants.hip
(pad_cols, crop_add, gelu_twin) and csrc/bn.hip (bn_eval), each called directly and compared with a
float64 computation on the CPU from the same fp32 inputs.

Bars (tests/helpers.py; every check reports error / bar):
  data movement            bit-exact; a bf16 output equals torch's .to(bfloat16) of the fp32 value
  k fp32 roundings         |err| <= k * 2^-24 * |ref|, k counted from the kernel's expression
  tanh / exp / log / erf   rtol 1e-5, atol 1e-6 (test_gelu_fwd_bwd's bar); a bf16 twin: one bf16 ulp
  fp32 sums                |err| <= d * 2^-24 * sum|terms|, d = longest chain of dependent additions
  Adam                     rel-inf < 1e-6 (test_losses_and_adam's bar), here also for m and v
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .helpers import (BF16_ULP, EPS32, bits_equal, close_ratio, f64, report, rinf_ratio, roundings_ratio, sum_ratio)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fp32():
    import autoformer_amd as A

    A.set_compute("fp32")
    yield
    A.set_compute("fp32")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _f32(v):
    """The value an fp32 kernel argument takes, as a Python float."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------ Adam
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-8


def _adam_ref(p, g, m, v, step_size, bc2s):
    """adam_elem of elem.hip in float64 (fp32 hyper-parameters, as the kernel receives them)."""
    b1, b2, eps = _f32(B1), _f32(B2), _f32(AEPS)
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    p = p - step_size * (m / (v.sqrt() / bc2s + eps))
    return p, m, v


def _adam_state_ref(step):
    return [float(step), _f32(LR) / (1 - _f32(B1) ** step), (1 - _f32(B2) ** step) ** 0.5]


def _adam_run(n, max_blocks, offs):
    """Three steps on views buf[o:o+n] of padded parents (offs: p, g, m, v element offsets); returns the
    worst error / bar over p, m, v, state, and checks the parents outside the views."""
    from autoformer_amd import kernels as K

    pad = 8
    par = [_rand(n + 2 * pad, seed=s).to(DEV) for s in (1, 2, 3, 4)]
    par[2].zero_()
    par[3].zero_()
    views = [t[pad + o:pad + o + n] for t, o in zip(par, offs)]
    before = [t.clone() for t in par]
    pr, mr, vr = f64(views[0]), f64(views[2]), f64(views[3])
    st = torch.zeros(4, device=DEV)
    worst = 0.0
    for step in (1, 2, 3):
        g = _rand(n, seed=10 + step)
        views[1].copy_(g)
        K.adam(views[0], views[1], views[2], views[3], LR, B1, B2, AEPS, st, max_blocks=max_blocks)
        sref = _adam_state_ref(step)
        pr, mr, vr = _adam_ref(pr, g.double(), mr, vr, sref[1], sref[2])
        assert st[0].item() == step and st[3].item() == 0.0
        # state[1..2]: a double expression rounded once to fp32 (k = 1)
        worst = max(worst, roundings_ratio(st[1:3], torch.tensor(sref[1:]), 1))
    for name, got, ref in (("p", views[0], pr), ("m", views[2], mr), ("v", views[3], vr)):
        worst = max(worst, report("adam", f"n={n} mb={max_blocks} offs={offs} {name}", rinf_ratio(got, ref, 1e-6)))
    for i, (t, b, o) in enumerate(zip(par, before, offs)):
        if i == 1:
            continue  # g's view was written by the test itself
        lo, hi = pad + o, pad + o + n
        assert bits_equal(t[:lo], b[:lo]) and bits_equal(t[hi:], b[hi:]), f"array {i}: written outside its slice"
    return worst


@pytest.mark.parametrize("n", [1, 3, 1000, 5000, 5003])
def test_adam_sizes_default_blocks(n):
    """n = 1, 3: the scalar tail alone; 1000: one vector per thread; 5000 / 5003: the two-vector loop body
    (1250 vectors over 3 blocks of 256 threads), without / with a 3-element tail."""
    assert _adam_run(n, 0, (0, 0, 0, 0)) <= 1.0


def test_adam_one_block_paired_loop_single_vector_and_tail():
    """max_blocks = 1 at n = 5003: 1250 vectors over 256 threads = two passes of the paired loop, the
    single vector for threads < 226, then the 3-element tail."""
    assert _adam_run(5003, 1, (0, 0, 0, 0)) <= 1.0


def test_adam_misaligned_views_take_the_scalar_form():
    """All four arrays one element off 16-byte alignment (the training step's flat[split:] slices),
    max_blocks = 2: the scalar grid-stride form; then only g misaligned."""
    assert _adam_run(5003, 2, (1, 1, 1, 1)) <= 1.0
    assert _adam_run(5003, 0, (0, 1, 0, 0)) <= 1.0


def test_adam_without_advance_uses_the_stored_step_size():
    from autoformer_amd import kernels as K

    n = 1027
    p, g = _rand(n, seed=1).to(DEV), _rand(n, seed=2).to(DEV)
    m, v = _rand(n, seed=3).mul(0.1).to(DEV), _rand(n, seed=4).abs().to(DEV)
    st = torch.tensor([5.0, 0.0123, 0.77, 0.0], device=DEV)
    st0 = st.clone()
    pr, mr, vr = _adam_ref(f64(p), f64(g), f64(m), f64(v), f64(st)[1].item(), f64(st)[2].item())
    K.adam(p, g, m, v, LR, B1, B2, AEPS, st, advance=False)
    assert bits_equal(st, st0)
    for name, got, ref in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        assert report("adam", f"advance=False {name}", rinf_ratio(got, ref, 1e-6)) <= 1.0


def test_adam_empty_slice_only_advances_the_state():
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    arrs = [_rand(8, seed=s).to(DEV) for s in (1, 2, 3, 4)]
    before = [t.clone() for t in arrs]
    st = torch.zeros(4, device=DEV)
    L.call("avc_adam_blocks", *[t.data_ptr() for t in arrs], 0, LR, B1, B2, AEPS, st.data_ptr(), 1, 0, K.stream())
    assert all(bits_equal(t, b) for t, b in zip(arrs, before))
    assert st[0].item() == 1.0
    assert roundings_ratio(st[1:3], torch.tensor(_adam_state_ref(1)[1:]), 1) <= 1.0


def test_adam_plain_entry_point():
    """avc_adam (no block cap) is the entry point the wrapper does not use: one step through _lib.call."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    n = 1003
    p, g = _rand(n, seed=1).to(DEV), _rand(n, seed=2).to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    st = torch.zeros(4, device=DEV)
    sref = _adam_state_ref(1)
    pr, mr, vr = _adam_ref(f64(p), f64(g), f64(m), f64(v), sref[1], sref[2])
    L.call("avc_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, AEPS, st.data_ptr(), 1,
           K.stream())
    for name, got, ref in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        assert report("adam", f"avc_adam {name}", rinf_ratio(got, ref, 1e-6)) <= 1.0


# ---------------------------------------------------------------------------------------- losses
def _loss_d(n, cap, per_block):
    """Longest addition chain of loss_kernel / bce_kernel: the thread's grid-stride loop, the 6-level
    wave tree, 3 adds over the block's 4 waves, the division by n, and up to `grid` atomic adds."""
    grid = min(cap, -(-n // per_block))
    return -(-n // (grid * 256)) + 6 + 3 + 1 + grid


@pytest.mark.parametrize("n", [1, 1023, 1025, 262145])
@pytest.mark.parametrize("mode", ["mse", "l1"])
def test_mse_l1_loss(n, mode):
    """262145 > 256 blocks x 1024 elements: the grid-stride loop runs a second time.  The second call goes
    through _lib.call with `out` preloaded to 1e9: the zeroing launch must clear it."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    a, b = _rand(n, seed=1), _rand(n, seed=2)
    dd = a.double() - b.double()
    terms = dd * dd if mode == "mse" else dd.abs()
    ref, sabs = terms.sum() / n, terms.sum() / n
    # d: the chain above + the term's own roundings (a - b, and d * d for the MSE)
    d = _loss_d(n, 256, 1024) + (2 if mode == "mse" else 1)
    ad, bd = a.to(DEV), b.to(DEV)
    got = (K.mse_loss if mode == "mse" else K.l1_loss)(ad, bd)
    assert report("loss", f"{mode} n={n}", sum_ratio(got, ref, sabs, d)) <= 1.0
    out = torch.full((1,), 1e9, device=DEV)
    L.call("avc_mse_loss" if mode == "mse" else "avc_l1_loss", ad.data_ptr(), bd.data_ptr(), n, out.data_ptr(),
           K.stream())
    assert report("loss", f"{mode} n={n} preloaded", sum_ratio(out[0], ref, sabs, d)) <= 1.0


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_loss_grad(n, mode, sign):
    from autoformer_amd import kernels as K

    a, b = _rand(n, seed=3), _rand(n, seed=4)
    b[::3] = a[::3]  # a == b: the L1 gradient is exactly 0 there
    dl = torch.tensor([0.37])
    dd = a.double() - b.double()
    ref = sign * dl.double() * (2 * dd if mode == 0 else dd.sign()) / n
    got = K.loss_grad(a.to(DEV), b.to(DEV), dl.to(DEV), mode, sign)
    # k: mode 0: a - b, sign*dloss, * f, / n = 4 (2 * d is exact); mode 1: f = +-1 / 0 exactly: 3
    k = 4 if mode == 0 else 3
    assert report("loss", f"loss_grad n={n} mode={mode} sign={sign}", roundings_ratio(got, ref, k)) <= 1.0
    assert (f64(got)[::3] == 0).all()


def _bce_p(n):
    g = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=g)
    if n >= 3:
        p[0], p[n // 2], p[n - 1] = 0.0, 1.0, 0.0
        p[1] = 1.0
    else:
        p[0] = 0.0
    return p


@pytest.mark.parametrize("n", [1, 255, 262147])
@pytest.mark.parametrize("target", [0.0, 1.0, 0.3])
def test_bce_loss(n, target):
    """p holds exact 0.0 and 1.0: log clamps at -100 as nn.BCELoss does.  262147 > 1024 blocks x 256: the
    grid-stride loop runs twice for three threads."""
    from autoformer_amd import kernels as K

    p = _bce_p(n)
    t = _f32(target)
    p64 = p.double()
    ref = F.binary_cross_entropy(p64, torch.full_like(p64, t))
    sabs = (t * p64.log().clamp_min(-100).abs() + (1 - t) * (1 - p64).log().clamp_min(-100).abs()).sum() / n
    # each term: two logs (rtol 1e-5 each, the transcendental bar) and 1 - p, two products, one add, the
    # negation-free sum: 4 roundings on top of the chain
    d = _loss_d(n, 1024, 256) + 4
    got = K.bce_loss(p.to(DEV), target)
    err = abs(f64(got).item() - ref.item())
    bar = (d * EPS32 + 1e-5) * sabs.item() + 1e-6
    assert report("loss", f"bce n={n} t={target}", err / bar) <= 1.0


@pytest.mark.parametrize("n", [1, 255, 262147])
@pytest.mark.parametrize("target", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("through", [False, True])
def test_bce_grad(n, target, through):
    from autoformer_amd import kernels as K

    p = _bce_p(n)
    t, p64, dl = _f32(target), p.double(), torch.tensor([-0.81])
    ref = dl.double() * (p64 - t) / ((1 - p64) * p64).clamp_min(_f32(1e-12)) / n
    if through:
        ref = ref * p64 * (1 - p64)
    got = K.bce_grad(p.to(DEV), target, dl.to(DEV), through_sigmoid=through)
    # k: p - t, dloss *, 1 - p, * p, the division, / n = 6; through the sigmoid: p (1 - p) and the product = 9
    k = 9 if through else 6
    assert report("loss", f"bce_grad n={n} t={target} through={through}", roundings_ratio(got, ref, k)) <= 1.0


# ----------------------------------------------------------------------------------- activations
def _act_ref(x, act):
    return [x, x.clamp_min(0), x.tanh(), torch.where(x > 0, x, _f32(0.01) * x),
            0.5 * x * (1 + torch.erf(x / 2 ** 0.5)), torch.sigmoid(x)][act]


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4, 5])
def test_act_fwd(n, act):
    from autoformer_amd import kernels as K

    x = _rand(n, seed=act, scale=2.0)
    got = K.act_fwd(x.to(DEV), act)
    ref = _act_ref(x.double(), act)
    if act in (0, 1):
        assert bits_equal(got, ref.float())
    elif act == 3:  # k = 1: 0.01f * x
        assert report("act", f"leaky fwd n={n}", roundings_ratio(got, ref, 1)) <= 1.0
    else:
        assert report("act", f"fwd act={act} n={n}", close_ratio(got, ref, 1e-5, 1e-6)) <= 1.0


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 5])
def test_act_bwd_from_output(n, act):
    from autoformer_amd import kernels as K

    x, g = _rand(n, seed=act + 10, scale=2.0), _rand(n, seed=act + 20)
    a = _act_ref(x.double(), act).float()  # the stored fp32 activation output
    a64, g64 = a.double(), g.double()
    got = K.act_bwd(g.to(DEV), a.to(DEV), act)
    if act in (0, 1):
        assert bits_equal(got, g if act == 0 else torch.where(a > 0, g, torch.zeros_like(g)))
    elif act == 3:  # k = 1
        assert report("act", f"leaky bwd n={n}", roundings_ratio(got, torch.where(a64 > 0, g64, _f32(0.01) * g64), 1)) <= 1.0
    elif act == 5:  # k = 3: g * a, 1 - a, their product
        assert report("act", f"sigmoid bwd n={n}", roundings_ratio(got, g64 * a64 * (1 - a64), 3)) <= 1.0
    else:
        # g (1 - a a): the rounding of a*a is not relative to 1 - a*a.  With e1, e2, e3 <= 2^-24:
        # g (1 + e3) [(1 - a^2)(1 + e2) - a^2 e1]  ->  |err| <= 2^-24 |g| (a^2 + 2 |1 - a^2|)
        ref = g64 * (1 - a64 * a64)
        r = sum_ratio(got, ref, g64.abs() * (a64 * a64 + 2 * (1 - a64 * a64).abs()), 1)
        assert report("act", f"tanh bwd n={n}", r) <= 1.0


def _gelu_grid():
    """>= 100k points over [-10, 10], +-0, 64 fp32 neighbours on each side of +-sqrt(2) (erf_nb switches
    pieces at |x| / sqrt(2) = 1), +-1e-4, +-6."""
    pts = [torch.linspace(-10, 10, 100001), torch.tensor([0.0, -0.0, 1e-4, -1e-4, 6.0, -6.0])]
    for s in (1.0, -1.0):
        c = np.float32(s * 2 ** 0.5)
        for toward in (np.float32(np.inf), np.float32(-np.inf)):
            v, run = c, []
            for _ in range(64):
                v = np.nextafter(v, toward)
                run.append(v)
            pts.append(torch.tensor(np.array(run + [c], dtype=np.float32)))
    return torch.cat(pts)


def _gelu_refs(x64, g64):
    cdf = 0.5 * (1 + torch.erf(x64 / 2 ** 0.5))
    pdf = torch.exp(-0.5 * x64 * x64) / (2 * np.pi) ** 0.5
    return x64 * cdf, g64 * (cdf + x64 * pdf)


def test_gelu_dense_grid_seam_and_tails():
    from autoformer_amd import kernels as K

    x = _gelu_grid()
    g = _rand(x.numel(), seed=5)
    yr, dr = _gelu_refs(x.double(), g.double())
    xd = x.to(DEV)
    assert report("gelu", "fwd grid", close_ratio(K.act_fwd(xd, K.ACT_GELU), yr, 1e-5, 1e-6)) <= 1.0
    assert report("gelu", "bwd grid", close_ratio(K.gelu_bwd(g.to(DEV), xd), dr, 1e-5, 1e-6)) <= 1.0


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1025])
@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("outs", ["f32", "bf16", "both"])
def test_gelu_twin(n, bwd, outs):
    """n = 1, 3: the scalar tail alone; 4: one full vector; 1023 / 1025: a block boundary and a 3- / 1-element
    tail.  The bf16 twin is the same fp32 value rounded: one bf16 ulp against float64."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    x, g = _rand(n, seed=n, scale=2.5), _rand(n, seed=n + 1)
    yr, dr = _gelu_refs(x.double(), g.double())
    ref = dr if bwd else yr
    xd, gd = x.to(DEV), g.to(DEV)
    y = torch.full((n,), 7.0, device=DEV) if outs != "bf16" else None
    y16 = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16) if outs != "f32" else None
    L.call("avc_gelu_twin", gd.data_ptr() if bwd else None, xd.data_ptr(), K._ptr(y), K._ptr(y16), n, bwd, K.stream())
    if y is not None:
        assert report("gelu", f"twin n={n} bwd={bwd} fp32", close_ratio(y, ref, 1e-5, 1e-6)) <= 1.0
    if y16 is not None:
        assert report("gelu", f"twin n={n} bwd={bwd} bf16", close_ratio(y16, ref, BF16_ULP, 1e-6)) <= 1.0
    if y is not None and y16 is not None:
        assert bits_equal(y16, y.to(torch.bfloat16))


@pytest.mark.parametrize("act", [4, 6, -1, 99])
def test_act_bwd_refuses_codes_without_a_from_output_derivative(act):
    """GELU (4) has no derivative from its output and fell into `default:` (dx = g) before; so did any code
    outside 0..5.  The entry point now refuses on the host, naming the code."""
    from autoformer_amd import kernels as K

    g, a = _rand(5, seed=1).to(DEV), _rand(5, seed=2).to(DEV)
    with pytest.raises(RuntimeError, match=rf"code {act}\b"):
        K.act_bwd(g, a, act)


@pytest.mark.parametrize("act", [6, -1, 99])
def test_act_fwd_refuses_unknown_codes(act):
    from autoformer_amd import kernels as K

    with pytest.raises(RuntimeError, match=rf"code {act}\b"):
        K.act_fwd(_rand(5, seed=1).to(DEV), act)


def test_abi_version_unchanged():
    from autoformer_amd import _lib as L

    assert L.lib().avc_abi_version() == 31


# ------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("B,nc,cd,de", [(3, 4, 6, 5), (1, 1, 1, 1)])
def test_code_cat(B, nc, cd, de):
    from autoformer_amd import kernels as K

    codes, emb = _rand(B, nc * cd, seed=1), _rand(B, de, seed=2)
    got = K.code_cat(codes.to(DEV), emb.to(DEV), B, nc, cd)
    ref = torch.cat((codes.view(B, nc, cd), emb.unsqueeze(1).expand(B, nc, de)), -1).reshape(B * nc, cd + de)
    assert bits_equal(got, ref.to(torch.bfloat16))


@pytest.mark.parametrize("B,T,nc,cd,de", [(3, 12, 4, 6, 5), (3, 12, 12, 6, 5)])
def test_dec_concat_bwd(B, T, nc, cd, de):
    """Reference: autograd through the torch expansion (AutoVC.py:197-204) in float64.  nc = T: one frame
    per code, a copy."""
    from autoformer_amd import kernels as K

    rep = T // nc
    dout = _rand(B * T, cd + de, seed=3)

    def through(d):
        c = torch.zeros(B, nc * cd, dtype=torch.float64, requires_grad=True)
        e = torch.zeros(B, de, dtype=torch.float64)
        x = torch.cat((c.view(B, nc, cd).repeat_interleave(rep, dim=1), e.unsqueeze(1).expand(B, T, de)), -1)
        x.backward(d.view(B, T, cd + de))
        return c.grad

    got = K.dec_concat_bwd(dout.to(DEV), B, T, nc, cd, de)
    # d = rep: one serial loop over the code's frames
    ratio = sum_ratio(got, through(dout.double()), through(dout.double().abs()), rep)
    assert report("glue", f"dec_concat_bwd rep={rep}", ratio) <= 1.0


def test_enc_concat_reads_a_column_slice_of_a_wider_buffer():
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    B, T, nm, de, ld, c0 = 2, 5, 7, 3, 12, 4
    wide, emb = _rand(B * T, ld, seed=4), _rand(B, de, seed=5)
    wd, ed = wide.to(DEV), emb.to(DEV)
    out = torch.empty(B * T, nm + de, device=DEV)
    L.call("avc_enc_concat", wd.data_ptr() + 4 * c0, ld, ed.data_ptr(), out.data_ptr(), B, T, nm, de, K.stream())
    ref = torch.cat((wide[:, c0:c0 + nm].view(B, T, nm), emb.unsqueeze(1).expand(B, T, de)), -1).reshape(B * T, nm + de)
    assert bits_equal(out, ref)


@pytest.mark.parametrize("C", [1, 257])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_eval(C, affine):
    from autoformer_amd import kernels as K

    rm, rv = _rand(C, seed=6), _rand(C, seed=7).abs() + 0.05
    ga, be = (_rand(C, seed=8) * 0.5 + 1, _rand(C, seed=9)) if affine else (None, None)
    eps = 1e-5
    mean, rstd, scale, shift = K.bn_eval(rm.to(DEV), rv.to(DEV), ga.to(DEV) if affine else None,
                                         be.to(DEV) if affine else None, eps)
    g64 = ga.double() if affine else torch.ones(C, dtype=torch.float64)
    b64 = be.double() if affine else torch.zeros(C, dtype=torch.float64)
    rs = 1 / (rv.double() + _f32(eps)).sqrt()
    assert bits_equal(mean, rm)
    # rstd: the add, the square root, the division: k = 3; scale = gamma * rstd: k = 4
    assert report("glue", f"bn_eval rstd C={C}", roundings_ratio(rstd, rs, 3)) <= 1.0
    assert report("glue", f"bn_eval scale C={C}", roundings_ratio(scale, g64 * rs, 4)) <= 1.0
    # shift = beta - t, t = mean * gamma * rstd carries 5 roundings, the subtraction one more on its result:
    # |err| <= 2^-24 (5 |t| + |beta - t|) <= 6 * 2^-24 (|beta| + |t|)
    t = rm.double() * g64 * rs
    assert report("glue", f"bn_eval shift C={C}", sum_ratio(shift, b64 - t, b64.abs() + t.abs(), 6)) <= 1.0


@pytest.mark.parametrize("R,C,Cd,lds", [(3, 5, 8, 5), (3, 8, 5, 8), (3, 5, 8, 7), (1, 1030, 1030, 1030), (65540, 1, 2, 1)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pad_cols(R, C, Cd, lds, dt):
    """Pad, crop, a source stride above C, a second 1024-column block, and more rows than grid.y holds."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    src = _rand(R, lds, seed=R + C)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    out = torch.full((R, Cd), 7.0, device=DEV, dtype=tdt)
    sd = src.to(DEV)
    L.call("avc_pad_cols", sd.data_ptr(), lds, out.data_ptr(), K.BF16 if dt == "bf16" else K.F32, R, C, Cd, K.stream())
    ref = torch.zeros(R, Cd)
    w = min(C, Cd)
    ref[:, :w] = src[:, :w]
    assert bits_equal(out, ref.to(tdt))


@pytest.mark.parametrize("R,C,lds", [(3, 5, 8), (1, 1030, 1032), (65540, 1, 2)])
def test_crop_add(R, C, lds):
    from autoformer_amd import kernels as K

    src, dst = _rand(R, lds, seed=R), _rand(R, C, seed=R + 1)
    got = K.crop_add(src.to(DEV), dst.to(DEV), C)
    # k = 1: one add
    assert report("glue", f"crop_add {R}x{C}", roundings_ratio(got, dst.double() + src[:, :C].double(), 1)) <= 1.0


@pytest.mark.parametrize("n", [1, 257])
def test_add(n):
    from autoformer_amd import kernels as K

    a, b = _rand(n, seed=1), _rand(n, seed=2)
    # k = 1
    assert roundings_ratio(K.add(a.to(DEV), b.to(DEV)), a.double() + b.double(), 1) <= 1.0
