"""avc_bn_seg_apply (bn_seg.hip, include/autovc_hip_eval.h) against torch fp64
F.batch_norm(training=True) applied to each utterance segment alone on the CPU.

Shapes: the smallest at which the kernel can go wrong -- T = 2 (the least torch admits), an odd T, C = 80
(one full and one partial 64-channel tile), C = 512 (eight tiles), more than one segment, T = 176 (the
conversion length, LDS-resident) and one T above AVC_BN_SEG_LDS_ROWS (the re-read path).

The bar of the outputs is the one tests/test_gpu_kernels.py::test_bn_act_forward_backward holds
avc_bn_apply's forward to: rel-inf < 1e-5 against the reference; mean and rstd are held to it per
(segment, channel)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
ACTS = {0: lambda z: z, 1: torch.relu, 2: torch.tanh}   # K.ACT_NONE / RELU / TANH: what the models use


def lds_rows():
    from autoformer_amd import _lib

    return _lib.BN_SEG_LDS_ROWS


def shapes():
    return [(1, 2, 80), (3, 7, 80), (2, 64, 512), (3, 176, 80), (2, lds_rows() + 1, 80)]


def rinf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def inputs(B, T, C, ld, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B * T, ld, generator=g) * 2 + 1
    y += torch.randn(B, 1, ld, generator=g).repeat_interleave(T, dim=0).reshape(B * T, ld)  # segment means differ
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res = torch.randn(B * T, ld, generator=g)
    return y, gamma, beta, res


def reference(y, B, T, C, gamma, beta, act, res=None, eps=EPS):
    """fp64: F.batch_norm(training=True) of each segment alone, then act (+ residual); mean, rstd (B, C)."""
    yd = y[:, :C].double().reshape(B, T, C)
    outs, means, rstds = [], [], []
    for b in range(B):
        z = F.batch_norm(yd[b].t().unsqueeze(0), None, None, gamma.double(), beta.double(), True, 0.1, eps)
        outs.append(ACTS[act](z.squeeze(0).t()))
        means.append(yd[b].mean(dim=0))
        rstds.append(1.0 / torch.sqrt(yd[b].var(dim=0, unbiased=False) + eps))
    o = torch.cat(outs)
    if res is not None:
        o = o + res[:, :C].double()
    return o, torch.stack(means), torch.stack(rstds)


@pytest.fixture(autouse=True)
def _fp32():
    import autoformer_amd as A

    A.set_compute("fp32")
    yield
    A.set_compute("bf16")


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("B,T,C", shapes())
def test_against_fp64_batch_norm_per_segment(B, T, C, pad):
    """Outputs, mean and rstd per (segment, channel); pad > 0: ld > C.  Every act in one case: the
    statistics are the same, the reference is computed once per act."""
    from autoformer_amd import kernels as Kr

    ld = C + pad
    y, gamma, beta, _ = inputs(B, T, C, ld)
    yd, gd, bd = y.to(DEV), gamma.to(DEV), beta.to(DEV)
    for act in ACTS:
        want, mean, rstd = reference(y, B, T, C, gamma, beta, act)
        got, m, r = Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, C=C, want_stats=True)
        assert got.shape == (B * T, ld) and m.shape == r.shape == (B, C)
        e = (rinf(got[:, :C], want), rinf(m, mean), rinf(r, rstd))
        print(f"B={B} T={T} C={C} ld={ld} act={act}: out {e[0]:.2e} mean {e[1]:.2e} rstd {e[2]:.2e}")
        assert max(e) < 1e-5, e
        # per (segment, channel), not only in the max norm of the whole table
        assert ((m.cpu().double() - mean).abs() <= 1e-5 * mean.abs().clamp(min=1.0)).all()
        assert ((r.cpu().double() - rstd).abs() <= 1e-5 * rstd).all()


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,T,C", [(3, 7, 80), (2, lds_rows() + 1, 80)])
def test_outputs_and_residual(B, T, C, act, with_res):
    """fp32 out only, bf16 twin only, both -- with and without the residual, ld > C, on the resident and
    the re-read path.  The fp32 result meets the 1e-5 bar; the bf16 output is that result rounded once:
    bit-identical to the fp32 output's own rounding, and the same whether fp32 is also written or not."""
    import autoformer_amd as A
    from autoformer_amd import kernels as Kr

    ld = C + 3
    y, gamma, beta, res = inputs(B, T, C, ld, seed=1)
    yd, gd, bd = y.to(DEV), gamma.to(DEV), beta.to(DEV)
    rd = res.to(DEV) if with_res else None
    want, _, _ = reference(y, B, T, C, gamma, beta, act, res if with_res else None)
    o32 = Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, rd, C=C, twin16=False)         # fp32 only
    assert o32.dtype == torch.float32 and getattr(o32, "_bf16", None) is None
    assert rinf(o32[:, :C], want) < 1e-5
    o16 = Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, rd, C=C, out_bf16=True)        # bf16 only
    assert o16.dtype == torch.bfloat16 and o16.shape == (B * T, ld)
    both = Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, rd, C=C, twin16=True)         # both
    assert torch.equal(both[:, :C], o32[:, :C])
    assert torch.equal(both._bf16[:, :C], o32[:, :C].bfloat16())
    assert torch.equal(o16[:, :C], both._bf16[:, :C])
    A.set_compute("bf16")                                                             # the default twin follows the mode
    assert Kr.bn_seg_apply(yd, B, T, gd, bd, EPS, act, rd, C=C)._bf16 is not None


def test_large_mean_small_spread():
    """A segment whose channels sit at 1e3 with a spread of 1e-2: E[y^2] - E[y]^2 in fp32 would lose
    everything (1e6 against 1e-4).  No bar is fixed in advance: the error of an fp32 two-pass computation
    in torch on the CPU against fp64 is measured here, and the kernel is allowed 4x that (reduction
    order).  Both numbers are printed; profiles/eval_grid_bench.txt records a run."""
    from autoformer_amd import kernels as Kr

    B, T, C = 3, 176, 80
    g = torch.Generator().manual_seed(3)
    y = (1e3 + 1e-2 * torch.randn(B * T, C, generator=g)).float()
    gamma, beta = torch.ones(C), torch.zeros(C)
    want, mean, rstd = reference(y, B, T, C, gamma, beta, 0)
    y3 = y.reshape(B, T, C)
    m32 = y3.mean(dim=1, keepdim=True)
    v32 = ((y3 - m32) ** 2).mean(dim=1, keepdim=True)
    two_pass = ((y3 - m32) / torch.sqrt(v32 + EPS)).reshape(B * T, C)
    err_cpu = float((two_pass.double() - want).abs().max())
    got, m, r = Kr.bn_seg_apply(y.to(DEV), B, T, gamma.to(DEV), beta.to(DEV), EPS, 0, want_stats=True)
    err_gpu = float((got.cpu().double() - want).abs().max())
    print(f"large mean / small spread: fp32 two-pass on the CPU {err_cpu:.3e}, kernel {err_gpu:.3e} (max abs, "
          f"outputs of unit spread); rstd rel {rinf(r, rstd):.3e}")
    assert torch.isfinite(got).all()
    assert err_cpu > 0 and err_gpu <= 4 * err_cpu, (err_gpu, err_cpu)


@pytest.mark.parametrize("T", [7, lds_rows() + 1])
def test_segments_are_independent(T):
    """Changing segment 1's data leaves segment 0's output (and statistics) bit-identical."""
    from autoformer_amd import kernels as Kr

    B, C = 2, 80
    y, gamma, beta, _ = inputs(B, T, C, C, seed=5)
    y2 = y.clone()
    y2[T:] = y2[T:] * 3 - 7
    gd, bd = gamma.to(DEV), beta.to(DEV)
    a, ma, ra = Kr.bn_seg_apply(y.to(DEV), B, T, gd, bd, EPS, 2, want_stats=True)
    b, mb, rb = Kr.bn_seg_apply(y2.to(DEV), B, T, gd, bd, EPS, 2, want_stats=True)
    assert torch.equal(a[:T], b[:T]) and torch.equal(ma[0], mb[0]) and torch.equal(ra[0], rb[0])
    assert not torch.equal(a[T:], b[T:])
    # ... and equals the B = 1 call on segment 0 alone
    one = Kr.bn_seg_apply(y[:T].contiguous().to(DEV), 1, T, gd, bd, EPS, 2)
    assert torch.equal(one, a[:T])


@pytest.mark.parametrize("B,T,C", [(3, 7, 80), (2, lds_rows() + 1, 80), (2, 64, 512)])
def test_nothing_outside_the_tile_is_written(B, T, C):
    """Rows outside [0, B*T) and columns [C, ld) of sentinel-filled outputs (fp32 and bf16) keep the
    sentinel; so do the rows around the statistics."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    ld, guard, S = C + 7, 3, -768.0   # (exact in bf16)
    M = B * T
    y, gamma, beta, res = inputs(B, T, C, ld, seed=7)
    buf32 = torch.full((M + 2 * guard, ld), S, device=DEV)
    buf16 = torch.full((M + 2 * guard, ld), S, device=DEV, dtype=torch.bfloat16)
    stats = torch.full((2, B + 2, C), S, device=DEV)
    yd, gd, bd, rd = y.to(DEV), gamma.to(DEV), beta.to(DEV), res.to(DEV)
    o32, o16 = buf32[guard:guard + M], buf16[guard:guard + M]
    _lib.call("avc_bn_seg_apply", yd.data_ptr(), _lib.F32, ld, B, T, C, gd.data_ptr(), bd.data_ptr(), EPS, 1,
              rd.data_ptr(), o32.data_ptr(), o16.data_ptr(), stats[0, 1].data_ptr(), stats[1, 1].data_ptr(), Kr.stream())
    torch.cuda.synchronize()
    want, mean, rstd = reference(y, B, T, C, gamma, beta, 1, res)
    assert rinf(o32[:, :C], want) < 1e-5
    for buf in (buf32, buf16):
        assert (buf[:guard] == S).all() and (buf[guard + M:] == S).all() and (buf[:, C:] == S).all()
        assert not (buf[guard:guard + M, :C] == S).any()
    assert (stats[:, 0] == S).all() and (stats[:, B + 1] == S).all()
    assert rinf(stats[0, 1:B + 1], mean) < 1e-5 and rinf(stats[1, 1:B + 1], rstd) < 1e-5
