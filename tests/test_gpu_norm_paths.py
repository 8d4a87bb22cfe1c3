"""GroupNorm(1, C) and LayerNorm of csrc/norm.hip over the dispatch paths the model shapes never take,
each called through autoformer_amd.kernels (or _lib.call where the wrapper hides the parameter) and
compared with float64 F.group_norm / F.layer_norm and their autograd on the CPU.

Bars: those of tests/test_gpu_metaformer.py (test_group_norm_fwd_bwd, test_layer_norm_fwd_bwd,
test_layer_norm_bf16_and_residual_forms), against float64 instead of fp32 torch:
  y, mean, rstd  rtol 1e-5 atol 1e-5      dx       rtol 1e-4 atol 1e-5
  dgamma, dbeta  rtol 1e-4 atol 1e-4      row sums rtol 1e-4 atol 1e-4      bf16 outputs rtol 1e-2 atol 1e-2

The workspace canary pins a defect of avc_group_norm_bwd: its vector path wrote nrb*C*2 + 2B + 2*B*ns
floats (nrb = ceil(B*L / 128)) into a workspace of avc_norm_ws(B*L, C) = ceil(B*L / 64)*C*2 + 1024 floats:
1224 of 1064 at (B, L, C) = (300, 1, 4), 2176 of 1280 at (512, 2, 8)."""
import pytest
import torch
import torch.nn.functional as F

from .helpers import bits_equal, close_ratio, report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(autouse=True)
def _fp32():
    import autoformer_amd as A

    A.set_compute("fp32")
    yield
    A.set_compute("fp32")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _misaligned(t):
    """A device copy of t whose base is one element past 16-byte alignment."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _check(family, what, pairs):
    for name, got, ref, rtol, atol in pairs:
        assert report(family, f"{what} {name}", close_ratio(got, ref, rtol, atol)) <= 1.0, name


# ------------------------------------------------------------------------------------- GroupNorm
def _gn_ref(x, dy, gamma, beta, B, L, C):
    """float64 GroupNorm(1, C) of frame-major (B*L, C) rows and its gradients."""
    xr = x.double().requires_grad_(True)
    g = (gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)).requires_grad_(True)
    b = (beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)).requires_grad_(True)
    y = F.group_norm(xr.view(B, L, C).transpose(1, 2), 1, g, b, EPS).transpose(1, 2).reshape(B * L, C)
    y.backward(dy.double())
    xs = x.double().view(B, -1)
    mean = xs.mean(1)
    rstd = 1 / (xs.var(1, unbiased=False) + EPS).sqrt()
    return y.detach(), mean, rstd, xr.grad, g.grad, b.grad


# (B, L, C): vector kernels with an unsplit sample; split statistics (3 chunks) with the scalar apply and
# backward; split vector kernels with an uneven last chunk (4100 + 4096); scalar with B > 1; 129 parameter
# partial rows, so pair_final_kernel's 128-row pass runs twice
GN_CASES = [(2, 8, 16), (1, 2048, 6), (1, 2049, 4), (3, 33, 5), (1, 16500, 4)]


def _gn_run(B, L, C, variant, misalign=False):
    from autoformer_amd import kernels as K

    x = _rand(B * L, C, seed=3, scale=2.0) + 0.7
    dy = _rand(B * L, C, seed=4)
    affine = variant != "noaffine"
    gamma = _rand(C, seed=1) * 0.5 + 1 if affine else None
    beta = _rand(C, seed=2) * 0.1 if affine else None
    dg0, db0 = _rand(C, seed=5), _rand(C, seed=6)
    xd = _misaligned(x) if misalign else x.to(DEV)
    gd, bd = (gamma.to(DEV), beta.to(DEV)) if affine else (None, None)
    y, mean, rstd = K.group_norm_fwd(xd, B, C, gd, bd, EPS)
    want = variant != "noparam"
    dg, db = (dg0.to(DEV), db0.to(DEV)) if want else (None, None)
    acc = variant == "accumulate"
    dx = K.group_norm_bwd(dy.to(DEV), xd, gd, mean, rstd, B, C, dg, db, accumulate=acc)
    yr, mr, rr, dxr, dgr, dbr = _gn_ref(x, dy, gamma, beta, B, L, C)
    what = f"({B},{L},{C}) {variant}{' misaligned' if misalign else ''}"
    pairs = [("y", y, yr, 1e-5, 1e-5), ("mean", mean, mr, 1e-5, 1e-5), ("rstd", rstd, rr, 1e-5, 1e-5),
             ("dx", dx, dxr, 1e-4, 1e-5)]
    if want:
        pairs += [("dgamma", dg, dgr + (dg0.double() if acc else 0), 1e-4, 1e-4),
                  ("dbeta", db, dbr + (db0.double() if acc else 0), 1e-4, 1e-4)]
    _check("groupnorm", what, pairs)


@pytest.mark.parametrize("B,L,C", GN_CASES)
@pytest.mark.parametrize("variant", ["affine", "noaffine", "noparam", "accumulate"])
def test_group_norm_paths(B, L, C, variant):
    """noaffine: gamma and beta null; noparam: dgamma / dbeta null; accumulate: onto random values."""
    _gn_run(B, L, C, variant)


@pytest.mark.parametrize("B,L,C", [(2, 8, 16), (1, 2049, 4)])
def test_group_norm_misaligned_input_falls_back(B, L, C):
    """C % 4 == 0 but x one element off 16-byte alignment: the scalar kernels must take it."""
    _gn_run(B, L, C, "affine", misalign=True)


@pytest.mark.parametrize("B,L,C", [(2, 8, 16), (1, 2049, 4)])
def test_group_norm_bf16_twin(B, L, C):
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    x = _rand(B * L, C, seed=3, scale=2.0) + 0.7
    gamma, beta = _rand(C, seed=1) * 0.5 + 1, _rand(C, seed=2) * 0.1
    A.set_compute("bf16")  # the twins exist in bf16 compute mode only
    y, _, _ = K.group_norm_fwd(x.to(DEV), B, C, gamma.to(DEV), beta.to(DEV), EPS, twin=True)
    yr = _gn_ref(x, torch.zeros_like(x), gamma, beta, B, L, C)[0]
    _check("groupnorm", f"({B},{L},{C}) twin", [("y", y, yr, 1e-5, 1e-5), ("y16", y._bf16, yr, 1e-2, 1e-2)])
    assert bits_equal(y._bf16, y.to(torch.bfloat16))


def test_group_norm_bf16_twin_refused_on_the_scalar_path():
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    A.set_compute("bf16")
    with pytest.raises(RuntimeError, match="bf16 twin"):
        K.group_norm_fwd(_rand(3 * 33, 5, seed=3).to(DEV), 3, 5, None, None, EPS, twin=True)


def test_group_norm_fwd_without_workspace():
    """avc_group_norm_fwd (no workspace, no twin): a 12288-element sample reduced by ONE block, which the
    wrapper's avc_group_norm_fwd2 call splits into three."""
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    B, L, C = 1, 2048, 6
    x = _rand(B * L, C, seed=3, scale=2.0) + 0.7
    gamma, beta = _rand(C, seed=1) * 0.5 + 1, _rand(C, seed=2) * 0.1
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y, mean, rstd = torch.empty_like(xd), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    L_.call("avc_group_norm_fwd", xd.data_ptr(), B, L * C, C, gd.data_ptr(), bd.data_ptr(), EPS, y.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), K.stream())
    yr, mr, rr = _gn_ref(x, torch.zeros_like(x), gamma, beta, B, L, C)[:3]
    _check("groupnorm", "plain entry", [("y", y, yr, 1e-5, 1e-5), ("mean", mean, mr, 1e-5, 1e-5),
                                        ("rstd", rstd, rr, 1e-5, 1e-5)])


GUARD = 8192


@pytest.mark.parametrize("B,L,C", [(300, 1, 4), (512, 2, 8)])
def test_group_norm_bwd_stays_inside_its_workspace(B, L, C):
    """The workspace is exactly avc_norm_ws(B*L, C) floats inside a buffer with 8192 sentinel floats on each
    side, so a write past it lands in the test's own memory.  Many samples of few elements: the parameter
    partials and per-sample means fit, the vector path's chunk partials did not."""
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    M = B * L
    n_ws = int(L_.lib().avc_norm_ws(M, C))
    assert n_ws == -(-M // 64) * C * 2 + 1024
    buf = torch.full((GUARD + n_ws + GUARD,), 12345.0, device=DEV)
    sentinel = buf.clone()
    x = _rand(M, C, seed=3, scale=2.0) + 0.7
    dy, gamma = _rand(M, C, seed=4), _rand(C, seed=1) * 0.5 + 1
    xd, dyd, gd = x.to(DEV), dy.to(DEV), gamma.to(DEV)
    y, mean, rstd = K.group_norm_fwd(xd, B, C, gd, None, EPS)
    dx, dg, db = torch.empty_like(xd), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    L_.call("avc_group_norm_bwd", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B,
            L * C, C, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, buf.data_ptr() + 4 * GUARD, K.stream())
    torch.cuda.synchronize()
    assert bits_equal(buf[:GUARD], sentinel[:GUARD]), "written before the workspace"
    assert bits_equal(buf[GUARD + n_ws:], sentinel[GUARD + n_ws:]), "written past the workspace"
    _, _, _, dxr, dgr, dbr = _gn_ref(x, dy, gamma, None, B, L, C)
    _check("groupnorm", f"canary ({B},{L},{C})", [("dx", dx, dxr, 1e-4, 1e-5), ("dgamma", dg, dgr, 1e-4, 1e-4),
                                                 ("dbeta", db, dbr, 1e-4, 1e-4)])


def test_group_norm_bwd_refuses_what_its_workspace_cannot_hold():
    """4000 samples of 4 elements: the per-sample means alone (8000 floats) exceed avc_norm_ws(4000, 4) = 1528."""
    from autoformer_amd import kernels as K

    B, C = 4000, 4
    x = _rand(B, C, seed=3).to(DEV)
    y, mean, rstd = K.group_norm_fwd(x, B, C, None, None, EPS)
    with pytest.raises(RuntimeError, match="workspace"):
        K.group_norm_bwd(x, x, None, mean, rstd, B, C)


# ------------------------------------------------------------------------------------- LayerNorm
def _ln_ref(x, dy, gamma, beta, res):
    R, D = x.shape
    xr = x.double().requires_grad_(True)
    g = (gamma.double() if gamma is not None else torch.ones(D, dtype=torch.float64)).requires_grad_(True)
    b = (beta.double() if beta is not None else torch.zeros(D, dtype=torch.float64)).requires_grad_(True)
    y = F.layer_norm(xr, (D,), g, b, EPS)
    y.backward(dy.double())
    dx = xr.grad + (res.double() if res is not None else 0)
    x64 = x.double()
    return y.detach(), x64.mean(1), 1 / (x64.var(1, unbiased=False) + EPS).sqrt(), dx, g.grad, b.grad


def _ln_run(R, D, variant, misalign=False):
    """plain / noaffine (gamma, beta null) / dgamma_only (dbeta null) / accumulate / fused (the residual
    gradient added, the bf16 twin and the row sums written in the same pass) / bf16_out (forward to bf16 only)."""
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    x, dy = _rand(R, D, seed=3, scale=3.0), _rand(R, D, seed=4)
    affine = variant != "noaffine"
    gamma = _rand(D, seed=1) * 0.3 + 1 if affine else None
    beta = _rand(D, seed=2) * 0.1 if affine else None
    fused = variant == "fused"
    res = _rand(R, D, seed=5) if fused else None
    dg0, db0 = _rand(D, seed=6), _rand(D, seed=7)
    if fused:
        A.set_compute("bf16")  # the bf16 twins exist in bf16 compute mode only
    xd = _misaligned(x) if misalign else x.to(DEV)
    gd, bd = (gamma.to(DEV), beta.to(DEV)) if affine else (None, None)
    y, mean, rstd = K.layer_norm_fwd(xd, gd, bd, EPS, out_bf16=variant == "bf16_out")
    dg, db = dg0.to(DEV), (None if variant == "dgamma_only" else db0.to(DEV))
    acc = variant == "accumulate"
    rsum = torch.empty(R, device=DEV) if fused else None
    dx = K.layer_norm_bwd(dy.to(DEV), xd, gd, mean, rstd, dg, db, accumulate=acc, residual=res.to(DEV) if fused else None,
                          twin=fused, row_sum=rsum)
    yr, mr, rr, dxr, dgr, dbr = _ln_ref(x, dy, gamma, beta, res)
    what = f"({R},{D}) {variant}{' misaligned' if misalign else ''}"
    if variant == "bf16_out":
        assert y.dtype == torch.bfloat16
        pairs = [("y16", y, yr, 1e-2, 1e-2)]
    else:
        pairs = [("y", y, yr, 1e-5, 1e-5)]
    pairs += [("mean", mean, mr, 1e-5, 1e-5), ("rstd", rstd, rr, 1e-5, 1e-5), ("dx", dx, dxr, 1e-4, 1e-5),
              ("dgamma", dg, dgr + (dg0.double() if acc else 0), 1e-4, 1e-4)]
    if db is not None:
        pairs.append(("dbeta", db, dbr + (db0.double() if acc else 0), 1e-4, 1e-4))
    if fused:
        pairs += [("dx16", dx._bf16, dxr, 1e-2, 1e-2), ("row_sum", rsum, dxr.sum(1), 1e-4, 1e-4)]
    _check("layernorm", what, pairs)


# vector forms (D % 4 == 0): one float4 per lane at D <= 256 (D = 4: one live lane; 256: every lane), two at
# D in (256, 512] (260: one live lane in the second; 512: every lane); R = 1, 5, 65: one live wave, a second
# block of four rows, a second block of 64 backward rows
LN_VEC = [(1, 4), (5, 256), (65, 260), (5, 512), (65, 4), (1, 512)]
# scalar form: D % 4 != 0 below and above 512
LN_SCALAR = [(5, 6), (65, 516), (1, 6)]


@pytest.mark.parametrize("R,D", LN_VEC + LN_SCALAR)
@pytest.mark.parametrize("variant", ["plain", "noaffine", "dgamma_only", "accumulate"])
def test_layer_norm_paths(R, D, variant):
    _ln_run(R, D, variant)


@pytest.mark.parametrize("R,D", LN_VEC)
@pytest.mark.parametrize("variant", ["fused", "bf16_out"])
def test_layer_norm_vector_only_forms(R, D, variant):
    _ln_run(R, D, variant)


def test_layer_norm_above_512_columns_directly():
    """D = 1024 is a multiple of 4 but too long for the register-row kernels: the scalar form."""
    _ln_run(5, 1024, "plain")


@pytest.mark.parametrize("variant", ["plain", "fused"])
def test_layer_norm_many_rows_grow_the_backward_block(variant):
    """R = 33000 > 32768: the one-pass backward takes lrb = 80 rows per block instead of 64."""
    _ln_run(33000, 8, variant)


@pytest.mark.parametrize("R,D", [(5, 256), (65, 260)])
def test_layer_norm_misaligned_input_falls_back(R, D):
    _ln_run(R, D, "plain", misalign=True)


@pytest.mark.parametrize("R,D", [(5, 256), (65, 6)])
def test_layer_norm_plain_entry_points(R, D):
    """avc_layer_norm_fwd and avc_layer_norm_bwd, the forms without the bf16 / residual arguments: the
    backward is the two-pass scalar form even where the one-pass kernel would apply."""
    from autoformer_amd import _lib as L_
    from autoformer_amd import kernels as K

    x, dy = _rand(R, D, seed=3, scale=3.0), _rand(R, D, seed=4)
    gamma, beta = _rand(D, seed=1) * 0.3 + 1, _rand(D, seed=2) * 0.1
    xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    mean, rstd, dg, db = (torch.empty(n, device=DEV) for n in (R, R, D, D))
    ws = torch.empty(int(L_.lib().avc_norm_ws(R, D)), device=DEV)
    L_.call("avc_layer_norm_fwd", xd.data_ptr(), R, D, gd.data_ptr(), bd.data_ptr(), EPS, y.data_ptr(), mean.data_ptr(),
            rstd.data_ptr(), K.stream())
    L_.call("avc_layer_norm_bwd", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, D,
            dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), K.stream())
    yr, mr, rr, dxr, dgr, dbr = _ln_ref(x, dy, gamma, beta, None)
    _check("layernorm", f"plain entries ({R},{D})", [("y", y, yr, 1e-5, 1e-5), ("mean", mean, mr, 1e-5, 1e-5),
                                                     ("rstd", rstd, rr, 1e-5, 1e-5), ("dx", dx, dxr, 1e-4, 1e-5),
                                                     ("dgamma", dg, dgr, 1e-4, 1e-4), ("dbeta", db, dbr, 1e-4, 1e-4)])
