"""Direct tests of the MetaDV kernels (metadv.hip, include/autovc_hip_dv.h) against torch indexing and
fp64, on the smallest shapes that can go wrong: E and W that are no multiple of the 64-wide tile or
of the 4-wide vectors (the single-element paths), a tile-aligned shape (the vector paths), window
starts at 0 and at T - W, overlapping windows, more than one utterance and crop."""
import numpy as np
import pytest
import torch

from .helpers import rel_inf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 5  # rows in front of and behind every output

# (B, T, E, W, S, lefts[s][b]): starts at 0 and T - W, windows of one row overlapping each other
ODD = (2, 21, 40, 16, 3, [[0, 5], [5, 2], [3, 0]])
ODD2 = (2, 40, 70, 18, 3, [[0, 22], [22, 2], [3, 0]])        # E past one tile, W no multiple of 4
ALIGNED = (2, 80, 64, 32, 3, [[0, 48], [48, 20], [10, 0]])
WIDE = (2, 150, 192, 128, 2, [[0, 22], [11, 3]])              # several tiles along E and W
SHAPES = [ODD, ODD2, ALIGNED, WIDE]


def _h(B, T, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, E, generator=g)


def _gather(h, B, T, E, W, S, lefts):
    """X[(s*B+b)*E + l][c] = h[b][left[s][b] + c][l] by indexing."""
    hb = h.view(B, T, E)
    return torch.cat([hb[b, lefts[s][b]:lefts[s][b] + W].t() for s in range(S) for b in range(B)])


def _guarded(rows, cols, dtype, fill):
    buf = torch.full((rows + 2 * GUARD, cols), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


@pytest.mark.parametrize("shape", SHAPES)
def test_crop_windows_equals_the_gather(shape):
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    B, T, E, W, S, lefts = shape
    assert 0 in sum(lefts, []) and T - W in sum(lefts, [])
    h = _h(B, T, E)
    want = _gather(h, B, T, E, W, S, lefts)
    lf = K.Lefts(lefts, S, B, DEV)
    hd = h.to(DEV)
    for src, dtype, ref in ((hd, K.F32, want), (hd, K.BF16, want.bfloat16()), (hd.bfloat16(), K.BF16, want.bfloat16())):
        got = K.crop_windows(src, lf, B, T, W, dtype=dtype)
        assert got.dtype == ref.dtype and torch.equal(got.cpu(), ref), (src.dtype, dtype)
    # guard rows around the output stay untouched (the launch writes S*B*E rows of W and nothing else)
    for tdt, dt in ((torch.float32, K.F32), (torch.bfloat16, K.BF16)):
        buf, X = _guarded(S * B * E, W, tdt, 7.0)
        L.call("avc_crop_windows", hd.data_ptr(), K.F32, lf.host, lf.dev.data_ptr(), None, B, T, E, W, S, X.data_ptr(),
               dt, K.stream())
        torch.cuda.synchronize()
        assert torch.equal(X.cpu(), want.to(tdt))
        assert (buf[:GUARD] == 7.0).all() and (buf[-GUARD:] == 7.0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_crop_windows_bwd_equals_the_scatter_sum(shape):
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    B, T, E, W, S, lefts = shape
    g = torch.Generator().manual_seed(1)
    dX = torch.randn(S * B * E, W, generator=g)
    de1 = torch.randn(B, E, generator=g)
    last = [T - 1, W - 1]
    want = torch.zeros(B, T, E, dtype=torch.float64)
    for s in range(S):
        for b in range(B):
            blk = dX[(s * B + b) * E:(s * B + b + 1) * E].double()  # (E, W)
            want[b, lefts[s][b]:lefts[s][b] + W] += blk.t()
    dXd, de1d = dX.to(DEV), de1.to(DEV)
    covered = torch.zeros(B, T, dtype=torch.bool)
    for s in range(S):
        for b in range(B):
            covered[b, lefts[s][b]:lefts[s][b] + W] = True
    for lasts in (None, last):
        ref = want.clone()
        for b in range(B):
            ref[b, (T - 1) if lasts is None else lasts[b]] += de1[b].double()
        lf = K.Lefts(lefts, S, B, DEV, last=lasts)
        buf, dh = _guarded(B * T, E, torch.float32, float("nan"))  # poisoned: every element must be written
        L.call("avc_crop_windows_bwd", dXd.data_ptr(), de1d.data_ptr(), lf.host, lf.dev.data_ptr(),
               lf.last_host, None if lf.last_dev is None else lf.last_dev.data_ptr(), B, T, E, W, S, dh.data_ptr(),
               K.stream())
        torch.cuda.synchronize()
        got = dh.cpu().view(B, T, E)
        err = rel_inf(got.numpy(), ref.numpy())
        print(f"crop_windows_bwd {shape[:5]} last={lasts}: rel-inf {err:.3e}")
        assert err <= 1e-6, err
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
        outside = ~covered
        for b in range(B):
            outside[b, (T - 1) if lasts is None else lasts[b]] = False
        assert outside.any() or shape is ODD  # ODD's windows cover all 21 frames; the others leave gaps
        assert (got[outside] == 0.0).all()  # frames outside every window: exactly zero
    # without de1 the last frame takes the windows' sum alone
    lf = K.Lefts(lefts, S, B, DEV)
    got = K.crop_windows_bwd(dXd, None, lf, B, T, E).cpu().view(B, T, E)
    assert rel_inf(got.numpy(), want.numpy()) <= 1e-6


def test_chan_mean_forward_and_backward():
    from autoformer_amd import kernels as K
    from autoformer_amd import metadv as MD

    S, B, E, O = 3, 2, 40, 5
    g = torch.Generator().manual_seed(2)
    Y = torch.randn(S * B * E, O, generator=g)
    want = Y.double().view(S, B, E, O)[..., O - 1].mean(0)
    Yd = Y.to(DEV).requires_grad_(True)
    e2 = MD.chan_mean(Yd, S, B)
    assert e2.shape == (B, E) and rel_inf(e2.detach().cpu().numpy(), want.numpy()) <= 1e-6
    gout = torch.randn(B, E, generator=g)
    e2.backward(gout.to(DEV))
    dY = Yd.grad.cpu()
    assert dY.shape == (S * B * E, O) and (dY[:, :O - 1] == 0.0).all()  # zero outside column O - 1
    ref = (gout.double() / S).repeat(S, 1).reshape(-1)
    assert rel_inf(dY[:, O - 1].numpy(), ref.numpy()) <= 1e-6
    # the raw backward writes all of a poisoned buffer's rows
    full = K.chan_mean_bwd(gout.to(DEV), S, O).cpu()
    assert torch.isfinite(full).all() and torch.equal(full, dY)


def test_metadv_head_against_fp64():
    from autoformer_amd import kernels as K

    S, O, B, E, D, C = 3, 5, 3, 40, 24, 7
    g = torch.Generator().manual_seed(3)
    e1, Y = torch.randn(B, E, generator=g), torch.randn(S * B * E, O, generator=g)
    w_dv, b_dv = torch.randn(D, 2 * E, generator=g) / 8, torch.randn(D, generator=g)
    w_out, b_out = torch.randn(C, D, generator=g) / 4, torch.randn(C, generator=g)
    e2 = Y.double().view(S, B, E, O)[..., O - 1].mean(0)
    emb = torch.cat((e1.double(), e2), 1) @ w_dv.double().t() + b_dv.double()
    dv_ref = emb / emb.norm(dim=1, keepdim=True)
    pred_ref = emb @ w_out.double().t() + b_out.double()
    dev = [t.to(DEV) for t in (e1, Y, w_dv, b_dv, w_out, b_out)]
    pred, dvec = K.metadv_head(dev[0], dev[1], S, dev[2], dev[3], dev[4], dev[5])
    errs = rel_inf(pred.cpu().numpy(), pred_ref.numpy()), rel_inf(dvec.cpu().numpy(), dv_ref.numpy())
    print("metadv_head rel-inf pred %.3e d_vec %.3e" % errs)
    assert pred.shape == (B, C) and dvec.shape == (B, D) and max(errs) <= 1e-5, errs
    np.testing.assert_allclose(dvec.cpu().norm(dim=1).numpy(), 1.0, rtol=1e-6)
    # the fused head equals chan_mean followed by itself on a single "crop" holding e2
    e2d = K.chan_mean(dev[1], S, B)
    pred0, dvec0 = K.metadv_head(dev[0], e2d.reshape(B * E, 1).contiguous(), 1, dev[2], None, dev[4], None)
    emb0 = torch.cat((e1.double(), e2), 1) @ w_dv.double().t()
    assert rel_inf(pred0.cpu().numpy(), (emb0 @ w_out.double().t()).numpy()) <= 1e-5


def test_host_refusals_launch_nothing():
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    B, T, E, W, S = 2, 21, 40, 16, 3
    h = _h(B, T, E).to(DEV)
    buf, X = _guarded(S * B * E, W, torch.float32, 7.0)
    dh = torch.full((B * T, E), 7.0, device=DEV)

    def refused(name, *args):
        assert getattr(L.lib(), name)(*args) == -1, name
        return L.lib().avc_last_error().decode()

    good = K.Lefts([[0, 5], [5, 2], [3, 0]], S, B, DEV)
    for bad in ([[0, 6], [5, 2], [3, 0]], [[0, 5], [-1, 2], [3, 0]]):  # a start out of range
        lf = K.Lefts(bad, S, B, DEV)
        assert "outside" in refused("avc_crop_windows", h.data_ptr(), K.F32, lf.host, lf.dev.data_ptr(), None, B, T, E,
                                    W, S, X.data_ptr(), K.F32, K.stream())
        assert "outside" in refused("avc_crop_windows_bwd", X.data_ptr(), None, lf.host, lf.dev.data_ptr(), None, None,
                                    B, T, E, W, S, dh.data_ptr(), K.stream())
        with pytest.raises(RuntimeError):
            K.crop_windows(h, lf, B, T, W)
    # a start inside T but past a row's own length
    lens = (L.c_int * B)(21, 20)
    assert "outside" in refused("avc_crop_windows", h.data_ptr(), K.F32, good.host, good.dev.data_ptr(), lens, B, T, E,
                                W, S, X.data_ptr(), K.F32, K.stream())
    # null pointers
    assert "null" in refused("avc_crop_windows", None, K.F32, good.host, good.dev.data_ptr(), None, B, T, E, W, S,
                             X.data_ptr(), K.F32, K.stream())
    assert "null" in refused("avc_crop_windows", h.data_ptr(), K.F32, good.host, None, None, B, T, E, W, S,
                             X.data_ptr(), K.F32, K.stream())
    assert "null" in refused("avc_crop_windows_bwd", X.data_ptr(), None, good.host, good.dev.data_ptr(), None, None, B,
                             T, E, W, S, None, K.stream())
    assert "null" in refused("avc_metadv_head", h.data_ptr(), None, S, 4, h.data_ptr(), None, h.data_ptr(), None, B, E,
                             8, 4, X.data_ptr(), dh.data_ptr(), K.stream())
    # W > T
    zero = K.Lefts([[0, 0]] * S, S, B, DEV)
    assert "longer than T" in refused("avc_crop_windows", h.data_ptr(), K.F32, zero.host, zero.dev.data_ptr(), None, B,
                                      T, E, T + 1, S, X.data_ptr(), K.F32, K.stream())
    assert "longer than T" in refused("avc_crop_windows_bwd", X.data_ptr(), None, zero.host, zero.dev.data_ptr(), None,
                                      None, B, T, E, T + 1, S, dh.data_ptr(), K.stream())
    torch.cuda.synchronize()
    assert (buf == 7.0).all() and (dh == 7.0).all()  # nothing was launched
