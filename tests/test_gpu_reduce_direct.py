"""The reductions outside the GEMMs and norms, called directly against float64 references computed on
the CPU from the same fp32 inputs: avc_colsum (csrc/bn.hip), and avc_moments / avc_adain_* /
avc_segsum / avc_rownorm_* (csrc/variants.hip).

Bars: an fp32 sum is held to |err| <= d * 2^-24 * sum|terms| with d the longest chain of dependent
additions a term passes through (serial loop + tree depths, read from the kernel and stated at each use);
moments / AdaIN and rownorm keep the bars of their older direct tests (tests/test_variants.py), against
float64."""
import warnings

import pytest
import torch

from .helpers import bits_equal, f64, rel_inf, report, sum_ratio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------- colsum
def _colsum_d(M, N, accumulate):
    """avc_colsum's strip sizing (bn.hip), then the chain: a thread adds every 16th row of its strip
    (rpb / 16), 16 row lanes are added through LDS, a finalize thread adds every 4th strip partial
    (ceil(nrb / 4)), 4 groups through LDS, and the accumulate."""
    ncb = _cdiv(N, 64)
    target = max(1024 // ncb, 1)
    rpb = 64 * _cdiv(_cdiv(M, 64), target)
    nrb = _cdiv(M, rpb)
    return rpb // 16 + 16 + _cdiv(nrb, 4) + 4 + (1 if accumulate else 0), rpb, nrb


# (M, N, ld, element offset of the base, with out2)
COLSUM_CASES = [
    # vector form: N % 4 == 0, ld % 4 == 0, 16-byte aligned
    (1, 4, 4, 0, False), (63, 64, 64, 0, False), (65, 68, 72, 0, True), (1000, 132, 132, 0, False),
    # scalar form: N % 4, ld % 4, or (last) a base one element off alignment
    (77, 5, 8, 0, True), (130, 70, 70, 0, False), (64, 8, 9, 0, False), (70, 8, 8, 1, False),
    # strips of 128 rows and 516 strip partials: the finalize's 128-partial pass runs five times
    (66000, 4, 4, 0, False),
]


@pytest.mark.parametrize("M,N,ld,off,with2", COLSUM_CASES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum(M, N, ld, off, with2, accumulate):
    from autoformer_amd import kernels as K

    buf = _rand(off + M * ld, seed=M + N)
    x = buf[off:].view(M, ld)
    init, init2 = _rand(N, seed=1), _rand(N, seed=2)
    xd = buf.to(DEV)[off:].view(M, ld)
    assert (xd.data_ptr() % 16 == 0) == (off == 0)
    out = init.to(DEV)
    out2 = init2.to(DEV) if with2 else None
    K.colsum(xd, M, N, ld=ld, out=out, accumulate=accumulate, out2=out2)
    d, rpb, nrb = _colsum_d(M, N, accumulate)
    if M == 66000:
        assert rpb > 64 and nrb > 128
    cols = x[:, :N].double()
    for name, got, i0 in (("out", out, init), ("out2", out2, init2)):
        if got is None:
            continue
        ref = cols.sum(0) + (i0.double() if accumulate else 0)
        sabs = cols.abs().sum(0) + (i0.double().abs() if accumulate else 0)
        what = f"{M}x{N} ld={ld} off={off} acc={accumulate} {name} d={d}"
        assert report("colsum", what, sum_ratio(got, ref, sabs, d)) <= 1.0


# ------------------------------------------------------------------------------ moments / AdaIN
def _moments_case(x_cpu, seed):
    """tests/test_variants.py test_gpu_moment_kernels_match_torch, at another input: the same loss, the
    same bars, float64 reference."""
    from autoformer_amd import variants as VV

    x = x_cpu.to(DEV).requires_grad_(True)
    mu = torch.tensor(0.3, device=DEV, requires_grad=True)
    sd = torch.tensor(1.9, device=DEV, requires_grad=True)
    w = _rand(*x_cpu.shape, seed=seed).to(DEV)
    mom = VV.moments(x)
    y = VV.adain(x, mu, sd)
    ((y * w).sum() + 0.7 * mom[0] - 1.3 * mom[1]).backward()
    xr = x_cpu.double().requires_grad_(True)
    mur, sdr = f64(mu).requires_grad_(True), f64(sd).requires_grad_(True)
    yr = (xr - xr.mean()) / xr.std() * sdr + mur
    ((yr * f64(w)).sum() + 0.7 * xr.mean() - 1.3 * xr.std()).backward()
    return {
        "y": rel_inf(f64(y), yr.detach()) / 1e-5,
        "mean": abs(mom[0].item() - xr.mean().item()) / 1e-5,
        "std": abs(mom[1].item() - xr.std().item()) / 1e-5,
        "dx": rel_inf(f64(x.grad), xr.grad) / 1e-4,
        "dmu": abs(mu.grad.item() - mur.grad.item()) / (1e-4 * abs(mur.grad.item()) + 1e-4),
        "dsigma": abs(sd.grad.item() - sdr.grad.item()) / (1e-4 * abs(sdr.grad.item()) + 1e-4),
    }


@pytest.mark.parametrize("shape", [(37, 3), (1, 2), (2, 1), (524293,)])
def test_moments_adain_tails_and_block_cap(shape):
    """n = 111, 2, 2: the n % 4 scalar tails (n = 2: no vector at all); 524293 = 512 blocks x 1024 + 5: the
    512-block cap makes the grid-stride loop run twice, with a 1-element tail."""
    r = _moments_case(_rand(*shape, seed=7, scale=1.7) - 2.5, 8)
    for k, v in r.items():
        assert report("moments", f"{shape} {k}", v) <= 1.0, k


def test_moments_adain_large_mean_small_spread():
    """mean 100, std 0.1: the double-precision sums of variants.hip keep sum x^2 - n mean^2 from cancelling
    (in fp32 the variance 0.01 would sit below the rounding of the 1e4-sized squares)."""
    r = _moments_case(_rand(37, 80, seed=9, scale=0.1) + 100.0, 10)
    for k, v in r.items():
        assert report("moments", f"mean100 {k}", v) <= 1.0, k


def test_moments_of_one_element():
    """n = 1: the mean is the element, the unbiased std is NaN as torch's is, and the backward passes (which
    divide by n - 1) refuse."""
    from autoformer_amd import variants as VV

    x = torch.tensor([1.25], device=DEV, requires_grad=True)
    mom = VV.moments(x)
    assert mom[0].item() == 1.25 and torch.isnan(mom[1]).item()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch warns about the zero degrees of freedom
        assert torch.isnan(x.detach().cpu().std()).item()
    with pytest.raises(RuntimeError, match="avc_moments_bwd"):
        mom.sum().backward()
    y = VV.adain(x, 0.3, 1.9)
    with pytest.raises(RuntimeError, match="avc_adain_bwd"):
        y.sum().backward()


# ---------------------------------------------------------------------------------------- segsum
# (B, T, C, ld, accumulate): one column; exactly one block of 256 columns; a second block; T = 1; a
# column block of wider rows; accumulate onto random values
@pytest.mark.parametrize("B,T,C,ld,accumulate", [(3, 19, 1, 1, False), (2, 7, 256, 256, False), (2, 5, 300, 300, False),
                                                 (3, 1, 70, 70, False), (3, 19, 70, 80, False), (2, 7, 300, 310, True)])
def test_segsum(B, T, C, ld, accumulate):
    from autoformer_amd import kernels as K

    x = _rand(B * T, ld, seed=B + T + C)
    c0 = ld - C  # the block's first column
    init = _rand(B, C, seed=3)
    xd = x.to(DEV)
    out = K.segsum(xd[:, c0:], B, T, C, ld=ld, out=init.to(DEV), accumulate=accumulate)
    blk = x.view(B, T, ld)[:, :, c0:].double()
    ref = blk.sum(1) + (init.double() if accumulate else 0)
    sabs = blk.abs().sum(1) + (init.double().abs() if accumulate else 0)
    # d: one serial loop over T, and the accumulate
    d = T + (1 if accumulate else 0)
    assert report("segsum", f"B={B} T={T} C={C} ld={ld} acc={accumulate}", sum_ratio(out, ref, sabs, d)) <= 1.0
    if T == 1 and not accumulate:
        assert bits_equal(out, x.view(B, T, ld)[:, 0, c0:].contiguous())


# --------------------------------------------------------------------------------------- rownorm
@pytest.mark.parametrize("R,C", [(1, 3), (5, 64), (6, 70)])
def test_rownorm_fwd_bwd(R, C):
    """C < 64: most lanes idle; C = 64: one element per lane; C = 70: a second, partial pass; R = 1, 5, 6:
    blocks of four rows with 1 and 2 live rows in the last.  Bars of test_gpu_rownorm_step_select_segsum_match_torch:
    forward 1e-6, backward 1e-5 (rel-inf), here also for the norms, against float64."""
    from autoformer_amd import kernels as K

    x, dy = _rand(R, C, seed=R), _rand(R, C, seed=R + 1)
    y, norms = K.rownorm_fwd(x.to(DEV))
    dx = K.rownorm_bwd(dy.to(DEV), y, norms)
    x64, dy64 = x.double(), dy.double()
    n64 = x64.norm(dim=-1, keepdim=True)
    y64 = x64 / n64
    dx64 = (dy64 - y64 * (y64 * dy64).sum(-1, keepdim=True)) / n64
    assert report("rownorm", f"{R}x{C} y", rel_inf(f64(y), y64) / 1e-6) <= 1.0
    assert report("rownorm", f"{R}x{C} norms", rel_inf(f64(norms), n64.squeeze(-1)) / 1e-6) <= 1.0
    assert report("rownorm", f"{R}x{C} dx", rel_inf(f64(dx), dx64) / 1e-5) <= 1.0
