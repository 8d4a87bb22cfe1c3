"""The softmax cross-entropy kernels (csrc/xent.hip), the binding and the autograd op on the device.

The yardstick is fp64 F.cross_entropy(..., label_smoothing = s) with autograd on the CPU, from the same fp32
inputs; rel-inf is max |difference| over max |fp64 value|, and the bar is 1e-5 for L and for dlogits: the bar
test_gpu_ge2e.py, test_rownorm_fwd_bwd and test_vc_loss_block_matches_torch hold fp32 kernels to against fp64.
Logits are randn rows scaled per row by 0.1 .. 8 and labels are uniform, so L is O(1).

Row offsets: the offset rows are built so that the shift is exact in fp32 (the row is first rounded to the
grid of 1e4's neighbourhood), so x - max(x) has the same bits with and without the offset; what was observed on
the MI355X is stated at test_row_offsets_cost_nothing."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .helpers import bits_equal, rel_inf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5
SHAPES = [(1, 1, 1),            # L = 0 and dlogits = 0 exactly
          (1, 2, 2),
          (3, 5, 5),            # scalar form
          (4, 64, 64),
          (5, 65, 68),          # tail past a wave
          (7, 80, 96),          # ld > C, vector form
          (2, 257, 257),
          (64, 256, 256),       # the training shape
          (3, 1025, 1028),      # several elements per thread
          (2, 16384, 16384)]    # the cap
SMOOTH = [0.0, 0.1]


def rows(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * (0.1 + 7.9 * torch.rand(B, 1, generator=g))
    return x, torch.randint(0, C, (B,), generator=g)


def reference(x, labels, smooth):
    """(L, dlogits, argmax hits) in fp64 on the CPU; x fp32 (B, C), labels int64 (B,)."""
    x64 = x.double().requires_grad_(True)
    L = F.cross_entropy(x64, labels, label_smoothing=smooth)
    L.backward()
    return L.item(), x64.grad.numpy(), int((x64.detach().argmax(1) == labels).sum())


@functools.lru_cache(maxsize=None)
def case(B, C, smooth):
    """Inputs and the fp64 reference of a shape; computed once, read-only."""
    x, labels = rows(B, C, seed=100 * B + C)
    return x, labels, reference(x, labels, smooth)


def strided(x, ld):
    """(view, buffer): x (B, C) on the device as a view of a (B, ld) buffer, row stride ld, 16-byte aligned."""
    buf = torch.full((x.shape[0], ld), 777.0, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]], buf


def raw(xv, lab, smooth, B, C, ld, d=None, ldd=0, correct=None):
    """avc_xent itself: returns (rc, L tensor)."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    lib = _lib.lib()
    ws = torch.empty(int(lib.avc_xent_ws(B, C)) // 4, device=DEV)
    L = torch.full((), -5.0, device=DEV)
    rc = lib.avc_xent(xv.data_ptr(), ld, B, C, lab.data_ptr(), smooth, L.data_ptr(), d.data_ptr() if d is not None else None,
                      ldd, correct.data_ptr() if correct is not None else None, ws.data_ptr(), K.stream())
    torch.cuda.synchronize()
    return rc, L


def errs_of(got_L, got_d, ref):
    eL = abs(got_L - ref[0]) / abs(ref[0]) if ref[0] != 0.0 else abs(got_L)
    scale = np.abs(ref[1]).max()
    return eL, (rel_inf(got_d, ref[1]) if scale > 0 else float(np.abs(got_d).max()))


# ----------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("smooth", SMOOTH)
@pytest.mark.parametrize("B,C,ld", SHAPES)
def test_kernel_against_fp64(B, C, ld, smooth):
    from autoformer_amd import kernels as K

    x, labels, ref = case(B, C, smooth)
    xv, buf = strided(x, ld)
    assert xv.stride(0) == ld or B == 1
    L, d, correct = K.xent(xv, K.Labels(labels, C, DEV), smooth)
    torch.cuda.synchronize()
    eL, ed = errs_of(L.item(), d.cpu().numpy(), ref)
    print("xent (%d, %d, ld %d) s = %.1f: L %.6f, rel-inf L %.3e dlogits %.3e, correct %d"
          % (B, C, ld, smooth, L.item(), eL, ed, correct.item()))
    assert d.shape == (B, C) and correct.dtype == torch.int32
    if C == 1:
        assert L.item() == 0.0 and not d.any()                                   # exactly
    assert eL < BAR and ed < BAR, (eL, ed)
    assert correct.item() == ref[2]
    assert buf[:, C:].eq(777.0).all() and torch.equal(buf[:, :C].cpu(), x)       # the padding of logits is not touched


@pytest.mark.parametrize("C", [80, 65])
def test_row_offsets_cost_nothing(C):
    """Rows offset by +1e4 and by -1e4 against the rows without the offset.  Observed on the MI355X: the same
    dlogits bits in both forms (vector, C = 80; scalar, C = 65) and for both smoothings; asserted here as the
    bar against fp64, which is what the offset must not cost, plus the bits."""
    from autoformer_amd import kernels as K

    x, labels = rows(4, C, seed=31)
    base = (x + 1e4) - 1e4                                                        # on 1e4's grid: the shifts below are exact
    up, down = base + 1e4, base - 1e4
    assert torch.equal(up - 1e4, base) and torch.equal(down + 1e4, base)
    xs, labs = torch.cat([base, up, down]), labels.repeat(3)
    for smooth in SMOOTH:
        ref = reference(xs, labs, smooth)
        L, d, _ = K.xent(xs.to(DEV), K.Labels(labs, C, DEV), smooth)
        eL, ed = errs_of(L.item(), d.cpu().numpy(), ref)
        same = bits_equal(d[:4], d[4:8]) and bits_equal(d[:4], d[8:])
        print("xent offsets C = %d s = %.1f: rel-inf L %.3e dlogits %.3e, same bits as without the offset: %s"
              % (C, smooth, eL, ed, same))
        assert eL < BAR and ed < BAR, (eL, ed)
        assert same


@pytest.mark.parametrize("C", [600, 601])
def test_correct_count_and_ties(C):
    from autoformer_amd import kernels as K

    B = 12
    x, labels = rows(B, C, seed=41)
    top = x.argmax(1)
    x[torch.arange(B), top] += 0.01                                              # a clear winner per row
    labels[::2] = top[::2]                                                       # half the labels are the winner
    # four tie rows: two exactly equal maxima at columns 5 and 300 (different threads and waves)
    tie = x[:4].clone()
    tie[:, 5] = tie[:, 300] = tie.max() + 1.0
    x = torch.cat([x, tie])
    labels = torch.cat([labels, torch.tensor([5, 300, 5, 7])])
    t2 = x[:B].double().topk(2, dim=1).values
    assert ((t2[:, 0] - t2[:, 1]) > 1e-3).all()                                  # the fp64 argmax is not in doubt
    assert (x[B:, 5] == x[B:, 300]).all() and (x[B:].max(1).values == x[B:, 5]).all()
    want = int((x[:B].double().argmax(1) == labels[:B]).sum()) + 2               # ties: only the lower index counts
    assert 6 <= want - 2 <= B
    for smooth in SMOOTH:
        _, _, correct = K.xent(x.to(DEV), K.Labels(labels, C, DEV), smooth, grads=False)
        assert correct.item() == want, (correct.item(), want)
    for lab, hit in ((5, 1), (300, 0)):                                          # a tie row alone
        _, _, correct = K.xent(x[B:B + 1].to(DEV), K.Labels([lab], C, DEV))
        assert correct.item() == hit


def test_two_calls_are_bit_identical_and_outputs_are_optional():
    from autoformer_amd import kernels as K

    for B, C in ((64, 256), (3, 1025)):
        x, labels, ref = case(B, C, 0.1)
        xd, lab = x.to(DEV), K.Labels(labels, C, DEV)
        a, b = K.xent(xd, lab, 0.1), K.xent(xd, lab, 0.1)
        torch.cuda.synchronize()
        for p, q in zip(a, b):
            assert bits_equal(p, q)
        # dlogits = None and correct = None, each and both: L has the same bits
        d, c = torch.empty(B, C, device=DEV), torch.zeros((), device=DEV, dtype=torch.int32)
        for dd, cc in ((None, c), (d, None), (None, None)):
            rc, L = raw(xd, lab.dev, 0.1, B, C, C, d=dd, ldd=C if dd is not None else 0, correct=cc)
            assert rc == 0 and bits_equal(L, a[0])
        assert bits_equal(d, a[1]) and c.item() == a[2].item() == ref[2]
        L0, d0, c0 = K.xent(xd, lab, 0.1, grads=False)
        assert d0 is None and bits_equal(L0, a[0]) and c0.item() == ref[2]


@pytest.mark.parametrize("B,C,ldd", [(5, 65, 68), (7, 80, 96)])
def test_only_the_outputs_are_written(B, C, ldd):
    """dlogits with ldd > C, filled with a sentinel: columns C .. ldd keep it, and so do guard regions around
    dlogits, L, correct and the stated workspace."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    guard, S = 16, -768.0
    x, labels, ref = case(B, C, 0.1)
    xd, lab = x.to(DEV), K.Labels(labels, C, DEV)
    nws = int(_lib.lib().avc_xent_ws(B, C)) // 4
    sizes = {"L": 1, "d": B * ldd, "ws": nws}
    bufs = {k: torch.full((n + 2 * guard,), S, device=DEV) for k, n in sizes.items()}
    v = {k: bufs[k][guard:guard + n] for k, n in sizes.items()}
    cbuf = torch.full((2 * guard + 1,), -7, device=DEV, dtype=torch.int32)
    _lib.call("avc_xent", xd.data_ptr(), C, B, C, lab.dev.data_ptr(), 0.1, v["L"].data_ptr(), v["d"].data_ptr(), ldd,
              cbuf[guard:].data_ptr(), v["ws"].data_ptr(), K.stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert (bufs[k][:guard] == S).all() and (bufs[k][guard + n:] == S).all(), k
    assert (cbuf[:guard] == -7).all() and (cbuf[guard + 1:] == -7).all() and cbuf[guard].item() == ref[2]
    d = v["d"].view(B, ldd)
    assert (d[:, C:] == S).all() and not (d[:, :C] == S).any()
    eL, ed = errs_of(v["L"].item(), d[:, :C].cpu().numpy(), ref)
    assert eL < BAR and ed < BAR, (eL, ed)


def test_labels_outside_the_classes_are_defined_behaviour():
    """Labels -1 and C as a raw device tensor at (3, 5): the call succeeds, L is NaN, the row with a valid
    label has the reference's dlogits, and nothing around logits and dlogits is written.  This checks defined
    behaviour: the kernel compares a label with column indices and never uses it as an address."""
    B, C, guard, S = 3, 5, 64, -768.0
    x, _ = rows(B, C, seed=51)
    labels = torch.tensor([-1, 2, C])
    ref = reference(x, torch.tensor([0, 2, 0]), 0.0)
    xbuf = torch.full((B * C + 2 * guard,), S, device=DEV)
    xbuf[guard:guard + B * C] = x.reshape(-1).to(DEV)
    before = xbuf.clone()
    dbuf = torch.full((B * C + 2 * guard,), S, device=DEV)
    correct = torch.full((), -7, device=DEV, dtype=torch.int32)
    lab = labels.to(torch.int32).to(DEV)
    rc, L = raw(xbuf[guard:guard + B * C], lab, 0.0, B, C, C, d=dbuf[guard:guard + B * C], ldd=C, correct=correct)
    assert rc == 0
    assert np.isnan(L.item())
    assert bits_equal(xbuf, before)                                               # logits and their guards
    assert (dbuf[:guard] == S).all() and (dbuf[guard + B * C:] == S).all()
    d = dbuf[guard:guard + B * C].view(B, C).cpu().numpy()
    assert np.isfinite(d).all()
    assert rel_inf(d[1], ref[1][1]) < BAR
    assert correct.item() == int(x[1].argmax() == 2)                             # the rows without a class never count
    # the rows with no class: softmax / B, nothing subtracted
    soft = torch.softmax(x.double(), 1).numpy() / B
    assert rel_inf(d[[0, 2]], soft[[0, 2]]) < BAR


# ----------------------------------------------------------------------- the autograd op
def test_softmax_xent_under_autograd():
    from autoformer_amd import kernels as K
    from autoformer_amd.xent import SoftmaxXent, softmax_xent

    B, C = 7, 80
    x, labels, ref = case(B, C, 0.1)
    xd = x.to(DEV).requires_grad_(True)
    L = softmax_xent(xd, K.Labels(labels, C, DEV), 0.1)
    (2.5 * L).backward()
    torch.cuda.synchronize()
    eL, ed = errs_of(L.item(), xd.grad.cpu().numpy(), (ref[0], 2.5 * ref[1]))
    print("softmax_xent upstream 2.5: rel-inf L %.3e dlogits %.3e" % (eL, ed))
    assert eL < BAR and ed < BAR
    # the module, with labels as an int64 device tensor (the caller's promise) and without a gradient
    crit = SoftmaxXent(0.1)
    with torch.no_grad():
        L2 = crit(x.to(DEV), labels.to(DEV))
    assert L2.item() == L.item() and crit.correct.item() == ref[2] and crit.correct.is_cuda
    # a non-contiguous view is made contiguous, not misread
    L3 = softmax_xent(x.t().contiguous().to(DEV).t(), K.Labels(labels, C, DEV), 0.1)
    assert L3.item() == L.item()
    with pytest.raises(TypeError):
        softmax_xent(x.to(DEV).half(), K.Labels(labels, C, DEV))                 # fp32 only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        softmax_xent(x, K.Labels(labels, C, DEV))                                # a host tensor
    with pytest.raises(TypeError):
        softmax_xent(x.to(DEV), labels)                                          # host labels go through Labels
    with pytest.raises(ValueError):
        softmax_xent(x.to(DEV), K.Labels(labels[:3], C, DEV))
