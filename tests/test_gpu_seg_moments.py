"""avc_seg_moments / avc_adain_seg (seg_moments.hip, include/autovc_hip_seg.h) against torch fp64 applied
to each segment alone on the CPU.

Shapes (B, n): the smallest at which the kernels can go wrong -- one mel frame, an odd T, n % 4 != 0 (the
scalar path, with a second segment off the 16-byte grid), the conversion shape 176 x 80 (LDS-resident),
one float4 above AVC_SEG_MOMENTS_LDS_FLOATS (the global re-read path), and n = 1 (NaN std, exact mean).

The bars are those tests/test_variants.py::test_gpu_moment_kernels_match_torch holds the whole-tensor
kernels to: moments within 1e-5 absolute, AdaIN output rel-inf < 1e-5; inputs as there, randn * 1.7 - 2.5."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cap():
    from autoformer_amd import _lib

    return _lib.SEG_MOMENTS_LDS_FLOATS


def shapes():
    return [(1, 80), (3, 7 * 80), (2, 15), (2, 176 * 80), (2, cap() + 4), (1, 1)]


def rinf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


@functools.lru_cache(maxsize=None)
def case(B, n, seed=7):
    """x (B, n), mu (B,), sigma (B,) on the host, and the fp64 reference: moments (B, 2), AdaIN (B, n).
    Computed once per shape and shared; nobody writes to them."""
    g = torch.Generator().manual_seed(seed + n)
    x = torch.randn(B, n, generator=g) * 1.7 - 2.5
    mu, sigma = torch.randn(B, generator=g), torch.rand(B, generator=g) + 0.5
    return (x, mu, sigma) + reference(x, mu, sigma)


def reference(x, mu, sigma):
    xd = x.double()
    mean = xd.mean(dim=1)
    std = torch.stack([xd[b].std() for b in range(x.shape[0])])     # n = 1: NaN, as torch.std gives
    y = (xd - mean[:, None]) / std[:, None] * sigma.double()[:, None] + mu.double()[:, None]
    return torch.stack([mean, std], dim=1), y


@pytest.mark.parametrize("B,n", shapes())
def test_against_fp64_per_segment(B, n):
    """Moments within 1e-5 absolute and AdaIN rel-inf < 1e-5, per segment."""
    from autoformer_amd import kernels as Kr

    x, mu, sigma, mom, y = case(B, n)
    xd = x.to(DEV).reshape(-1)
    got = Kr.seg_moments(xd, B)
    out = Kr.adain_seg(xd, B, mu.to(DEV), sigma.to(DEV)).reshape(B, n)
    assert got.shape == (B, 2) and got.dtype == torch.float32
    if n == 1:
        assert torch.equal(got[:, 0].cpu(), x[:, 0])                # the mean of one value is that value
        assert torch.isnan(got[:, 1]).all() and torch.isnan(out).all()
        return
    err = (got.cpu().double() - mom).abs().max().item()
    rels = [rinf(out[b], y[b]) for b in range(B)]
    print(f"B={B} n={n}: moments max abs {err:.2e}, adain rel-inf per segment", " ".join(f"{r:.2e}" for r in rels))
    assert err < 1e-5
    assert max(rels) < 1e-5, rels


def test_misaligned_base_takes_the_scalar_path():
    """n % 4 == 0 but x starts one float off the 16-byte grid: the same bars."""
    from autoformer_amd import kernels as Kr

    B, n = 2, 80
    x, mu, sigma, mom, y = case(B, n)
    buf = torch.zeros(B * n + 4, device=DEV)
    xd = buf[1:1 + B * n]
    xd.copy_(x.reshape(-1))
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    got = Kr.seg_moments(xd, B)
    out = Kr.adain_seg(xd, B, mu.to(DEV), sigma.to(DEV)).reshape(B, n)
    assert (got.cpu().double() - mom).abs().max().item() < 1e-5
    assert max(rinf(out[b], y[b]) for b in range(B)) < 1e-5


@pytest.mark.parametrize("B,n", shapes())
def test_one_segment_matches_the_whole_tensor_kernels(B, n):
    """At B = 1 the per-segment kernels meet the same bars against K.moments and K.adain_fwd."""
    from autoformer_amd import kernels as Kr

    x, mu, sigma, _, _ = case(B, n)
    xd, md, sd = x[0].contiguous().to(DEV), mu[:1].contiguous().to(DEV), sigma[:1].contiguous().to(DEV)
    got = Kr.seg_moments(xd, 1)
    whole = Kr.moments(xd)
    if n == 1:
        assert torch.equal(got[0, 0], whole[0]) and torch.isnan(got[0, 1]) and torch.isnan(whole[1])
        return
    assert (got[0].double() - whole.double()).abs().max().item() < 1e-5
    assert rinf(Kr.adain_seg(xd, 1, md, sd), Kr.adain_fwd(xd, whole, md, sd)) < 1e-5


def test_large_mean_small_spread():
    """A segment at 1e3 with a spread of 1e-2 beside a unit one: E[x^2] - E[x]^2 in fp32 would lose
    everything (1e6 against 1e-4), and so would a mean rounded to fp32 before the subtraction (half an ulp
    of 1e3 is 3e-5, a third of a percent of the spread).  No bar is fixed in advance: the max abs error of
    the unit-spread output (mu = 0, sigma = 1) against fp64 is compared with torch's own fp32 result on the
    CPU for the same segment, and the kernel is allowed 4x that, the margin tests/test_gpu_bn_seg.py gives
    avc_bn_seg_apply for the same reason.  Both numbers are printed.
    Measured on the MI355X (profiles/eval_grid_families_bench.txt): torch fp32 on the CPU 1.907e-3, the
    kernel 1.765e-7 -- it keeps the mean in fp64 through the subtraction."""
    from autoformer_amd import kernels as Kr

    n = 176 * 80
    g = torch.Generator().manual_seed(3)
    x = torch.stack([1e3 + 1e-2 * torch.randn(n, generator=g), torch.randn(n, generator=g)]).float()
    mu, sigma = torch.zeros(2), torch.ones(2)
    mom, want = reference(x, mu, sigma)
    cpu32 = (x[0] - x[0].mean()) / x[0].std()
    err_cpu = float((cpu32.double() - want[0]).abs().max())
    xd = x.to(DEV).reshape(-1)
    got = Kr.adain_seg(xd, 2, mu.to(DEV), sigma.to(DEV)).reshape(2, n)
    m = Kr.seg_moments(xd, 2)
    err_gpu = float((got[0].cpu().double() - want[0]).abs().max())
    print(f"large mean / small spread: torch fp32 on the CPU {err_cpu:.3e}, kernel {err_gpu:.3e} (max abs, output "
          f"of unit spread); std rel {abs(m[0, 1].item() - mom[0, 1].item()) / mom[0, 1].item():.3e}; "
          f"unit segment rel-inf {rinf(got[1], want[1]):.3e}")
    assert torch.isfinite(got).all()
    assert err_cpu > 0 and err_gpu <= 4 * err_cpu, (err_gpu, err_cpu)
    assert rinf(got[1], want[1]) < 1e-5


@pytest.mark.parametrize("n", [15, 7 * 80, cap() + 4])
def test_segments_are_independent(n):
    """Changing segment 1's input leaves segment 0's output bits and moments unchanged, and both equal the
    B = 1 call on segment 0 alone."""
    from autoformer_amd import kernels as Kr

    x, mu, sigma, _, _ = case(2, n)
    x2 = x.clone()
    x2[1] = x2[1] * 3 - 7
    md, sd = mu.to(DEV), sigma.to(DEV)
    a, ma = Kr.adain_seg(x.to(DEV).reshape(-1), 2, md, sd).reshape(2, n), Kr.seg_moments(x.to(DEV).reshape(-1), 2)
    b, mb = Kr.adain_seg(x2.to(DEV).reshape(-1), 2, md, sd).reshape(2, n), Kr.seg_moments(x2.to(DEV).reshape(-1), 2)
    assert torch.equal(a[0], b[0]) and torch.equal(ma[0], mb[0])
    assert not torch.equal(a[1], b[1]) and not torch.equal(ma[1], mb[1])
    x0 = x[0].contiguous().to(DEV)
    assert torch.equal(Kr.adain_seg(x0, 1, md[:1].contiguous(), sd[:1].contiguous()), a[0])
    assert torch.equal(Kr.seg_moments(x0, 1)[0], ma[0])


@pytest.mark.parametrize("B,n", [(3, 7 * 80), (2, 15), (2, cap() + 4)])
def test_nothing_outside_the_outputs_is_written(B, n):
    """Guard regions around y [0, B*n) and out [0, 2B) keep their sentinel."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    guard, S = 8, -768.0
    x, mu, sigma, mom, y = case(B, n)
    xd, md, sd = x.to(DEV).reshape(-1), mu.to(DEV), sigma.to(DEV)
    ybuf = torch.full((B * n + 2 * guard,), S, device=DEV)
    obuf = torch.full((2 * B + 2 * guard,), S, device=DEV)
    yv, ov = ybuf[guard:guard + B * n], obuf[guard:guard + 2 * B]
    _lib.call("avc_adain_seg", xd.data_ptr(), B, n, md.data_ptr(), sd.data_ptr(), yv.data_ptr(), Kr.stream())
    _lib.call("avc_seg_moments", xd.data_ptr(), B, n, ov.data_ptr(), Kr.stream())
    torch.cuda.synchronize()
    for buf, m in ((ybuf, B * n), (obuf, 2 * B)):
        assert (buf[:guard] == S).all() and (buf[guard + m:] == S).all()
        assert not (buf[guard:guard + m] == S).any()
    assert max(rinf(yv.reshape(B, n)[b], y[b]) for b in range(B)) < 1e-5
    assert (ov.reshape(B, 2).cpu().double() - mom).abs().max().item() < 1e-5


def test_bad_arguments_raise():
    from autoformer_amd import kernels as Kr
    from autoformer_amd import variants as V

    x = torch.randn(3 * 80, device=DEV)
    ok = torch.ones(3, device=DEV)
    with pytest.raises(ValueError, match="B\\*n == numel"):
        Kr.seg_moments(x, 7)
    with pytest.raises(ValueError, match="B\\*n == numel"):
        Kr.adain_seg(x, 7, torch.ones(7, device=DEV), torch.ones(7, device=DEV))
    with pytest.raises(ValueError, match="B\\*n == numel"):
        Kr.seg_moments(x, 0)
    for mu, sigma in ((ok[:2].contiguous(), ok), (ok, torch.ones(4, device=DEV)), (ok.reshape(3, 1), ok),
                      (ok, ok.double())):
        with pytest.raises(ValueError, match="must be a contiguous fp32 \\(3,\\) tensor"):
            Kr.adain_seg(x, 3, mu, sigma)
    strided = torch.randn(3 * 80, 2, device=DEV)[:, 0]
    for bad in (strided, x.bfloat16()):
        with pytest.raises(TypeError, match="contiguous fp32"):
            Kr.seg_moments(bad, 3)
        with pytest.raises(TypeError, match="contiguous fp32"):
            Kr.adain_seg(bad, 3, ok, ok)
    with pytest.raises(RuntimeError, match="autoformer_amd kernels need HIP device tensors"):
        Kr.seg_moments(x.cpu(), 3)
    h = x.reshape(3 * 8, 10)
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="forward-only"):
        V.seg_moments(h, 3)
    with pytest.raises(RuntimeError, match="forward-only"):
        V.adain_seg(h, 3, ok, ok)
    with torch.no_grad():
        assert V.seg_moments(h, 3).shape == (3, 2) and V.adain_seg(h, 3, ok, ok).shape == h.shape
