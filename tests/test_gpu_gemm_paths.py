"""Every avc_gemm kernel family behind its one entry point, pinned and checked per element.

Each row of tests/gemm_path_cases.py is run three ways:
  1. the witness: avc_gemm_last_path() names the kernel the row was written for, so a change to a
     dispatch predicate that moves the row to another kernel fails here instead of passing unnoticed;
  2. the values, per element against the float64 meaning of the descriptor (tests/gemm_ref.py).  Test
     data holds bf16-exact values (an "fp32" operand is the same values stored as fp32), so every
     product is exact in fp32 and the only error is fp32 accumulation:
        |err| <= (K + splits + 4) * 2^-24 * S,   S = |A| |B|^T + |bias| + |row_bias| + |residual| + |C0|
     -- the any-order summation bound over the K products, one addition per split-K partial, and the
     epilogue's additions (bias, row bias, residual, prior C); fp32 compute: + 1, each product rounds
     once.  A batch summed into one C has batch * K products and batch * splits partials.
     The bf16 twin is bit-equal to the rounded fp32 C; a bf16-only C adds BF16_ULP * |ref|;
  3. the guards: C (and its twin) is a view into a larger buffer of a sentinel, with guard rows above
     and below (and between the batches) and ldc > N guard columns; every
     guard element must be bit-unchanged.  Every row has guard columns (ldc = N + 3 on the scalar-store
     kernels, N + 8 where 16-B vector stores need it) except the avc_gemm_bnb rows, whose y shares C's
     ldc and so needs ldc == N.
col_sum is compared against float64 column sums of the kernel's own C: M terms and the prior value
in any order, (M + 1) * 2^-24 * (sum |C| + |prior|).
BatchNorm statistics are compared against fp64 statistics of the kernel's own fp32 C (bars of
test_bn_stats_epilogue_and_finalize / test_gemm_bn_fused_finalize), the BatchNorm-backward epilogue
against the fp64 backward of the kernel's own C (bars of test_bn_act_forward_backward).
"""
import ctypes

import pytest
import torch

from . import gemm_ref as R
from .gemm_path_cases import CASES
from .helpers import BF16_ULP, EPS32, _ratio, bits_equal, f64, report, rinf_ratio, sum_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 4          # guard rows above, below and between batches (4: C stays 16-B aligned for the vector stores)
SENT = 7.25    # sentinel, exact in bf16
_SHARED = {}   # operand values and products shared by rows of one shape (computed once, never written)


def _ring(mode):
    from autoformer_amd import _lib

    bm, bn, nst = (128, 128, 4) if mode == 1 else (0, 0, 0)  # the forced tile of the rows with ring=1
    _lib.call("avc_gemm_set_ring", mode, bm, bn, nst, 8, 2)


@pytest.fixture(autouse=True)
def _restore_ring_and_compute():
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    was = "bf16" if K.compute() == K.BF16 else "fp32"
    yield
    _ring(-1)
    A.set_compute(was)


def _relf(a, b):
    a, b = f64(a), f64(b)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _operand(rows, Kd, o, batch, gen, values=None):
    """(gemm_ref.Op over the CPU values, device tensor, avc_operand) of an operand recipe."""
    from autoformer_amd import kernels as K

    dt = torch.bfloat16 if o["dt"] == "bf16" else torch.float32
    ks, win = o["ks"], o["win"]
    nb = batch if o["batched"] else 1
    if win is None:
        shape = (Kd, rows) if ks else (rows, Kd)
    else:
        taps, pad, t_out, t_in, chans = win
        frames = Kd if ks else rows
        assert frames % t_out == 0 and taps * chans == (rows if ks else Kd)
        shape = (frames // t_out * t_in, chans)
    if values is not None:
        v = (values.t() if ks else values).contiguous().reshape(1, *shape)
    else:
        v = torch.randn(nb, *shape, generator=gen).bfloat16().float()  # bf16-exact values
    ld = shape[1]
    stride = shape[0] * shape[1] if o["batched"] else 0
    dev = v.to(DEV).to(dt)
    return R.Op(v.reshape(-1), ld, ks, win, stride), dev, K.operand(dev, ld, kstrided=ks, window=win, batch_stride=stride)


class _Out:
    """C as a view into a sentinel-filled buffer: guard rows, guard columns, gaps between batches."""

    def __init__(self, c, dtype, prior):
        self.N, self.M, self.ldc = c.N, c.M, c.N + c.ldc_pad
        self.nb = 1 if (c.bsum or c.batch == 1) else c.batch
        self.Mp = c.M if (c.fold or self.nb == 1) else c.M + G
        rows = 2 * G + self.nb * self.Mp
        self.buf0 = torch.full((rows, self.ldc), SENT, dtype=dtype)
        if prior is not None:
            for z in range(self.nb):
                self.interior(self.buf0, z).copy_(prior[z])
        self.buf = self.buf0.to(DEV)
        self.view = self.buf[G:]                       # what the descriptor points at
        self.cbs = self.Mp * self.ldc if self.nb > 1 else 0

    def interior(self, t, z):
        return t[G + z * self.Mp:G + z * self.Mp + self.M, :self.N]

    def got(self):
        h = self.buf.cpu()
        return torch.stack([self.interior(h, z) for z in range(self.nb)])

    def guards_untouched(self):
        h = self.buf.cpu().clone()
        for z in range(self.nb):
            self.interior(h, z).copy_(self.interior(self.buf0, z))
        return bits_equal(h, self.buf0)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_gemm_path(c):
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    A.set_compute(c.comp)
    _ring(c.ring)
    gen = torch.Generator().manual_seed(sum(map(ord, c.name)))
    M, N, Kd = c.M, c.N, c.K
    sh = _SHARED.setdefault(c.shared, {}) if c.shared else None
    if sh is not None and not sh:
        sh["a"] = torch.randn(M, Kd, generator=gen).bfloat16().float()
        sh["b"] = torch.randn(N, Kd, generator=gen).bfloat16().float()
    a_ref, a_dev, a_op = _operand(M, Kd, c.a, c.batch, gen, sh["a"] if sh else None)
    b_ref, b_dev, b_op = _operand(N, Kd, c.b, c.batch, gen, sh["b"] if sh else None)
    nb = 1 if (c.bsum or c.batch == 1) else c.batch
    bias = torch.randn(N, generator=gen) + (3.0 if c.bn is not None else 0.0) if c.bias else None
    res = torch.randn(nb, M, N, generator=gen) if c.res else None
    prior = torch.randn(nb, M, N, generator=gen) if c.acc else None
    rb = None
    if c.row_bias:
        T, pad = c.row_bias
        rb = (torch.randn(M // T * (2 * pad + 1), N, generator=gen), T, pad)

    out = _Out(c, torch.bfloat16 if c.c16only else torch.float32, prior)
    twin = _Out(c, torch.bfloat16, None) if c.twin else None
    resb = _Out(c, torch.float32, res) if c.res else None
    kw = dict(ldc=out.ldc, accumulate=c.acc, split_k=c.split, batch=c.batch, c_batch_stride=out.cbs, cperm=c.cperm)
    if bias is not None:
        kw["bias"] = bias.to(DEV)
    if resb is not None:
        kw["residual"] = resb.view
    if twin is not None:
        kw["c_bf16"] = twin.view
    if rb is not None:
        kw["row_bias"] = (rb[0].to(DEV), rb[1], rb[2])
    # ---- BatchNorm forward statistics / backward reduction riders
    part = st = fin = None
    if c.bn is not None:
        part = K.bn_partial_buffer(M, N, DEV)
        kw["bn_partial"] = part
        if c.bn >= 1:
            gamma, beta = (torch.rand(N, generator=gen) + 0.5).to(DEV), torch.randn(N, generator=gen).to(DEV)
            rm0, rv0 = torch.randn(N, generator=gen).to(DEV), (torch.rand(N, generator=gen) + 0.5).to(DEV)
            rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.long, device=DEV)
            kw["bn_fin"] = fin = (gamma, beta, rm, rv, nbt, 0.1, 1e-5, c.bn)
    if c.bnb is not None:
        y = (torch.randn(M, N, generator=gen) * 1.3 + 0.2).bfloat16()
        mean = y.double().mean(0).float()
        rstd = (1.0 / (y.double().var(0, unbiased=False) + 1e-5).sqrt()).float()
        gamma, beta = torch.rand(N, generator=gen) + 0.5, torch.randn(N, generator=gen) * 0.2
        coef = torch.empty(6 * N, device=DEV)
        dgam, dbet, dbia = (torch.empty(N, device=DEV) for _ in range(3))
        yd = y.to(DEV)
        kw["bnb"] = (yd, mean.to(DEV), rstd.to(DEV), gamma.to(DEV), beta.to(DEV), c.bnb, coef, dgam, dbet, dbia, 0)

    if c.col_sum:
        cs0 = torch.randn(N, generator=gen)
        cs = cs0.to(DEV)
        kw["col_sum"] = cs

    st = K.gemm(M, N, Kd, a_op, b_op, out.view, **kw)
    path = K.gemm_last_path()
    torch.cuda.synchronize()

    # ---- 1. the witness
    assert path == c.expect, f"{c.name}: ran on path {path:#x}, the row is written for {c.expect:#x}"

    # ---- 2. the values
    prods = None
    if sh is not None:
        if "prods" not in sh:
            sh["prods"] = R.product(M, N, Kd, a_ref, b_ref)
        prods = sh["prods"]
    ref, S = R.reference(M, N, Kd, a_ref, b_ref, batch=c.batch, batch_sum=c.bsum, bias=bias, residual=res, c0=prior,
                         cperm=c.cperm, row_bias=rb, prods=prods)
    got = out.got()
    units = c.batch if c.bsum else 1
    depth = Kd * units + c.split * units + (5 if c.comp == "fp32" else 4)
    if c.c16only:
        ratio = _ratio((f64(got) - ref).abs(), depth * EPS32 * S + BF16_ULP * ref.abs())
    else:
        ratio = sum_ratio(got, ref, S, depth)
    assert report(c.family, f"{c.name} C", ratio) <= 1
    if twin is not None:
        assert bits_equal(twin.got(), got.bfloat16()), f"{c.name}: the bf16 twin is not the rounded fp32 C"

    # ---- 3. the guards
    assert out.guards_untouched(), f"{c.name}: wrote outside C"
    if twin is not None:
        assert twin.guards_untouched(), f"{c.name}: wrote outside the bf16 twin"

    # ---- riders
    if c.col_sum:
        cf = f64(got[0])
        assert report(c.family, f"{c.name} col_sum",
                      sum_ratio(cs, cf.sum(0) + cs0.double(), cf.abs().sum(0) + cs0.double().abs(), M + 1)) <= 1
    if c.bn is not None:
        cf = f64(got[0])
        m_ref, r_ref = cf.mean(0), 1 / torch.sqrt(cf.var(0, unbiased=False) + 1e-5)
        if c.bn == 0:
            mean_, rstd_, _, _ = K.bn_finalize(part, M, N, None, None, None, None, None, 0.1, 1e-5)
        else:
            mean_, rstd_ = st[0], st[1]
            rm2, rv2, n2 = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.long, device=DEV)
            for _ in range(c.bn):
                st2 = K.bn_finalize(part, M, N, fin[0], fin[1], rm2, rv2, n2, 0.1, 1e-5)
            for nm, x, y2 in zip(("mean", "rstd", "scale", "shift", "rmean", "rvar"), st + (rm, rv), st2 + (rm2, rv2)):
                assert report(c.family, f"{c.name} fused {nm}", rinf_ratio(x, f64(y2), 1e-6)) <= 1
            assert int(nbt.item()) == c.bn == int(n2.item())
        assert report(c.family, f"{c.name} bn mean", rinf_ratio(mean_, m_ref, 1e-5)) <= 1
        assert report(c.family, f"{c.name} bn rstd", rinf_ratio(rstd_, r_ref, 1e-4)) <= 1
    if c.bnb is not None:
        cdev = out.view[:M]  # ldc == N: contiguous
        dy = K.bn_bwd_apply(cdev, yd, coef, c.bnb)
        torch.cuda.synchronize()
        dy_ref, dg_ref, db_ref = R.bn_backward(got[0], y, mean, rstd, gamma, beta, c.bnb)
        assert report(c.family, f"{c.name} bnb dy", _relf(dy, dy_ref) / 1e-4) <= 1
        assert report(c.family, f"{c.name} bnb dgamma", _relf(dgam, dg_ref) / 1e-5) <= 1
        assert report(c.family, f"{c.name} bnb dbeta", _relf(dbet, db_ref) / 1e-5) <= 1
        assert report(c.family, f"{c.name} bnb dbias", float(dbia.abs().max()) / 1e-3) <= 1


# ---------------------------------------------------------------------------------- host-only refusals
def _desc(M, N, Kd, a, b, c, **fields):
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    d = L.GemmDesc()
    d.M, d.N, d.K, d.batch, d.split_k, d.ldc, d.compute = M, N, Kd, 1, 1, N, L.BF16
    d.a, d.b = K.operand(a, Kd), K.operand(b, Kd)
    if c is not None:
        d.c = c.data_ptr()
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


REFUSED = [("cperm-with-bias", dict(cperm=4, bias="f32"), "cperm"),
           ("bn-partial-with-split-k", dict(bn_partial="f32", split_k=2), "bn_partial"),
           ("bf16-only-c-with-accumulate", dict(c=None, c_bf16="bf16", accumulate=1), "bf16-only"),
           ("row-bias-on-a-k-strided-operand", dict(row_bias="f32", rb_t=8, rb_pad=1, a_kstrided=1), "row_bias"),
           ("col-sum-with-accumulate", dict(col_sum="f32", accumulate=1), "col_sum"),
           ("negative-k", dict(K=-1), "negative")]


@pytest.mark.parametrize("name,fields,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_launch_nothing(name, fields, word):
    """Each refused combination is refused on the host: the message names it, the witness reads 0 and C
    is untouched."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    M, N, Kd = 64, 64, 64
    a = torch.randn(M, Kd, device=DEV).bfloat16()
    b = torch.randn(N, Kd, device=DEV).bfloat16()
    K.gemm(M, N, Kd, K.operand(a, Kd), K.operand(b, Kd), torch.empty(M, N, device=DEV))
    assert K.gemm_last_path() != 0
    c = torch.full((M, N), SENT, device=DEV)
    bufs = {"f32": torch.zeros(M * N, device=DEV), "bf16": torch.full((M, N), SENT, device=DEV, dtype=torch.bfloat16)}
    fields = {k: bufs[v] if isinstance(v, str) else v for k, v in fields.items()}
    kstr = fields.pop("a_kstrided", 0)
    d = _desc(M, N, Kd, a, b, None if "c" in fields and fields.pop("c") is None else c, **fields)
    d.a.kstrided = kstr
    rc = L.lib().avc_gemm(ctypes.byref(d), K.stream())
    assert rc != 0 and word.encode() in L.lib().avc_last_error(), L.lib().avc_last_error()
    assert K.gemm_last_path() == 0
    torch.cuda.synchronize()
    assert bool((c == SENT).all()) and bool((bufs["bf16"] == SENT).all())


def test_empty_product_launches_nothing():
    """M == 0 (and N == 0) return success without a launch: witness 0, C untouched."""
    from autoformer_amd import kernels as K

    a = torch.randn(8, 64, device=DEV).bfloat16()
    b = torch.randn(64, 64, device=DEV).bfloat16()
    c = torch.full((8, 64), SENT, device=DEV)
    K.gemm(8, 64, 64, K.operand(a, 64), K.operand(b, 64), torch.empty(8, 64, device=DEV))
    assert K.gemm_last_path() != 0
    for M, N in ((0, 64), (8, 0)):
        K.gemm(M, N, 64, K.operand(a, 64), K.operand(b, 64), c, ldc=64)
        assert K.gemm_last_path() == 0
    torch.cuda.synchronize()
    assert bool((c == SENT).all())


def test_bnb_refusal_clears_the_witness():
    """avc_gemm_bnb's own argument check (before gemm_impl) leaves the witness 0 as well."""
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    a = torch.randn(64, 64, device=DEV).bfloat16()
    c = torch.full((64, 64), SENT, device=DEV)
    K.gemm(64, 64, 64, K.operand(a, 64), K.operand(a, 64), torch.empty(64, 64, device=DEV))
    assert K.gemm_last_path() != 0
    d = _desc(64, 64, 64, a, a, c)
    bb = L.BnbArgs()  # y / mean / rstd / coef / ws all null
    rc = L.lib().avc_gemm_bnb(ctypes.byref(d), ctypes.byref(bb), K.stream())
    assert rc != 0 and b"avc_gemm_bnb" in L.lib().avc_last_error()
    assert K.gemm_last_path() == 0
    torch.cuda.synchronize()
    assert bool((c == SENT).all())
