"""The forward-only persistent recurrence (lstm_infer.hip, avc_lstm_infer) and the d-vector head
(variants.hip, avc_dvec_head) at kernel level, H = 768, bf16 compute, 8- and 16-row groups.

Reference for the recurrence: the CPU loop of test_gpu_kernels.py::test_lstm_persistent_forward_
matches_per_step (fp32 state, bf16-rounded W_hh, h_{t-1} rounded to bf16 before the recurrent
product) with that test's bar for this arithmetic, relf < 2e-3, on h_last (captured at step
lens[b] - 1) and on the bf16 h of every frame.  Measured: h_last 2.4e-7 (T = 1) to 1.9e-4 (T = 37);
the bf16 h 1.6e-3 to 1.7e-3 at every shape, T = 1 included -- that is the bf16 rounding of the output
itself (up to 2^-9 relative per element)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 768


@pytest.fixture(autouse=True)
def _bf16():
    import autoformer_amd as A

    A.set_compute("bf16")
    yield
    A.set_compute("bf16")


def relf(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def _case(B, T, seed=1):
    G = 4 * H
    gen = torch.Generator().manual_seed(seed)
    xproj = torch.randn(B * T, G, generator=gen) * 0.5
    whh = (torch.randn(G, H, generator=gen) * (1.0 / H ** 0.5)).bfloat16()
    return xproj, whh


def _ref(xproj, whh, B, T):
    """(B, T, H) fp32 h of every step."""
    w = whh.float()
    xp = xproj.view(B, T, 4 * H)
    h = torch.zeros(B, H)
    c = torch.zeros(B, H)
    outs = []
    for t in range(T):
        gts = xp[:, t] + h.bfloat16().float() @ w.t()
        i, f, gg, o = gts.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs, 1)


def _shapes(rows):
    # no recurrent product at all; a partial group captured at step 0, mid-sequence and the last
    # step; a second group holding one row; the persistent forward test's own T
    return [(1, 1, None), (3, 5, [5, 1, 3]), (rows + 1, 4, None), (2, 37, None)]


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("case", range(4))
def test_lstm_infer_matches_cpu_loop(rows, case):
    from autoformer_amd import kernels as Kr

    B, T, lens = _shapes(rows)[case]
    xproj, whh = _case(B, T)
    ref = _ref(xproj, whh, B, T)
    assert Kr.lstm_infer_persistent(B, H, rows)
    hb = Kr.lstm_infer_scratch(B, H, DEV, rows)
    h16, last = Kr.lstm_infer(xproj.to(DEV), whh.to(DEV), B, T, H, lens=lens, rows=rows, want_h16=True,
                              want_last=True, hbuf=hb)
    torch.cuda.synchronize()
    assert Kr.lstm_timeout_flag(hb, B, H) == 0
    Kr.check_faults()
    ref_last = torch.stack([ref[b, (lens[b] if lens else T) - 1] for b in range(B)])
    e_last, e_h16 = relf(last, ref_last), relf(h16.float().view(B, T, H), ref)
    print(f"rows={rows} B={B} T={T}: relf h_last {e_last:.3e}, h_bf16 {e_h16:.3e}")
    assert last.shape == (B, H) and h16.shape == (B * T, H) and h16.dtype == torch.bfloat16
    assert e_last < 2e-3, e_last
    assert e_h16 < 2e-3, e_h16


@pytest.mark.parametrize("rows", [8, 16])
def test_lstm_infer_single_outputs(rows):
    """h_bf16 = None and h_last = None are each a valid call; neither changes the other output."""
    from autoformer_amd import kernels as Kr

    B, T, lens = 3, 5, [5, 1, 3]
    xproj, whh = _case(B, T, seed=2)
    xd, wd = xproj.to(DEV), whh.to(DEV)
    hb = Kr.lstm_infer_scratch(B, H, DEV, rows)
    both16, both_last = Kr.lstm_infer(xd, wd, B, T, H, lens=lens, rows=rows, want_h16=True, want_last=True, hbuf=hb)
    only16, none_last = Kr.lstm_infer(xd, wd, B, T, H, lens=lens, rows=rows, want_h16=True, want_last=False, hbuf=hb)
    none16, only_last = Kr.lstm_infer(xd, wd, B, T, H, lens=lens, rows=rows, want_h16=False, want_last=True, hbuf=hb)
    torch.cuda.synchronize()
    assert Kr.lstm_timeout_flag(hb, B, H) == 0
    assert none_last is None and none16 is None
    assert torch.equal(only16, both16) and torch.equal(only_last, both_last)
    with pytest.raises(ValueError):
        Kr.lstm_infer(xd, wd, B, T, H, rows=rows, want_h16=False, want_last=False)


def test_lstm_infer_refuses_bad_lens_on_the_host():
    """A length of 0 or T + 1 is refused before any launch, by the wrapper and by the C entry."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as Kr

    B, T = 3, 5
    xproj, whh = _case(B, T, seed=3)
    xd, wd = xproj.to(DEV), whh.to(DEV)
    for bad in ([5, 0, 3], [5, T + 1, 3]):
        with pytest.raises(ValueError):
            Kr.lstm_infer(xd, wd, B, T, H, lens=bad, want_h16=False, want_last=True)
        hb = Kr.lstm_infer_scratch(B, H, DEV)
        last = torch.full((B, H), 7.0, device=DEV)
        arr = (ctypes.c_int * B)(*bad)
        rc = _lib.lib().avc_lstm_infer(xd.data_ptr(), wd.data_ptr(), arr, B, T, H, 0, None, last.data_ptr(),
                                       hb.data_ptr(), Kr.stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"lens" in _lib.lib().avc_last_error()
        assert bool((last == 7.0).all())  # nothing ran
    # both outputs null, and a shape off the persistent path, are refused as well
    assert _lib.lib().avc_lstm_infer(xd.data_ptr(), wd.data_ptr(), None, B, T, H, 0, None, None, hb.data_ptr(),
                                     Kr.stream()) != 0
    assert not Kr.lstm_infer_persistent(B, 512) and not Kr.lstm_infer_persistent(B, H, 4)


@pytest.mark.parametrize("B", [1, 5])
def test_dvec_head_matches_fp64(B):
    from autoformer_amd import kernels as Kr

    E = 256
    gen = torch.Generator().manual_seed(5 + B)
    h = torch.randn(B, H, generator=gen) * 0.3
    w = (torch.rand(E, H, generator=gen) * 2 - 1) * (6.0 / (E + H)) ** 0.5
    b = (torch.rand(E, generator=gen) * 2 - 1) / H ** 0.5
    y = h.double() @ w.double().t() + b.double()
    ref = y / y.norm(dim=-1, keepdim=True)
    got = Kr.dvec_head(h.to(DEV), w.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"dvec_head B={B}: rel-inf {err:.3e}")
    assert got.shape == (B, E)
    assert err < 1e-5, err
