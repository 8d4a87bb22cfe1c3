"""The GE2E loss kernels (csrc/ge2e.hip), the autograd op, EmbedderStep, verification_eer and the trainer's
command line on the device.

The yardstick of the kernels is `restatement` below -- the plain-torch text of the loss -- evaluated in fp64
with autograd on the CPU; rel-inf is max |difference| over max |fp64 value|, and the bar is 1e-5 for each of
L, de and dw: the bar test_vc_loss_block_matches_torch, test_rownorm_fwd_bwd and
test_dvec_head_matches_fp64 hold fp32 kernels to against fp64.  The same restatement in fp32 on the CPU sits
at or below 5.4e-7 on the shapes here, so the bar is about 18 x what fp32 arithmetic alone costs.

The yardstick of the model tests is a plain-torch twin on the CPU (nn.LSTM + Linear + normalise + the
restatement) with the same state_dict, at the bars of test_gpu_lstmdv.py::
test_fp32_training_step_matches_fixture."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .conftest import ROOT
from .helpers import grad_mismatches, rel_inf
from .test_ge2e import _tree
from .test_lstmdv import RefDV

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5
SHAPES = [(2, 2, 256),    # smallest legal; M - 1 = 1
          (3, 2, 8),      # D below a wave; odd N
          (5, 3, 100),    # D a multiple of 4 but not of 64
          (4, 5, 257),    # scalar path; tail
          (65, 2, 256),   # N past one wave of columns
          (64, 10, 256)]  # the training shape; still tiny


@pytest.fixture(autouse=True)
def _restore_modes():
    import autoformer_amd as A
    from autoformer_amd import kernels as K
    from autoformer_amd.layers import set_grad_sink

    yield
    A.set_compute("bf16")
    K.set_deterministic(False)
    set_grad_sink(False)


def similarities(e):
    """S (N, M, N) of the definition: e (N, M, D), any dtype."""
    N, M, _ = e.shape
    c = e.mean(1)
    c_ex = (e.sum(1, keepdim=True) - e) / (M - 1)
    S = F.cosine_similarity(e[:, :, None, :], c[None, None, :, :], dim=-1, eps=1e-8)       # (N, M, N)
    own = F.cosine_similarity(e, c_ex, dim=-1, eps=1e-8)                                    # (N, M)
    eye = torch.eye(N, dtype=torch.bool)[:, None, :].expand(N, M, N)
    return torch.where(eye, own[:, :, None].expand(N, M, N), S)


def restatement(e, w):
    """The definition: e (N, M, D), w a scalar tensor, any dtype."""
    N, M, _ = e.shape
    return F.cross_entropy((w * similarities(e)).reshape(N * M, N), torch.arange(N).repeat_interleave(M))


def reference(e, w):
    """(L, de, dw) of the restatement in fp64 with autograd; e (N, M, D) fp32 on the host."""
    e64 = e.double().requires_grad_(True)
    w64 = torch.tensor(float(w), dtype=torch.float64, requires_grad=True)
    L = restatement(e64, w64)
    L.backward()
    return L.item(), e64.grad.numpy(), w64.grad.item()


def rows(N, M, D, seed):
    """randn rows scaled per row by 0.1 .. 3, so the norms differ."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, M, D, generator=g) * (0.1 + 2.9 * torch.rand(N, M, 1, generator=g))


@functools.lru_cache(maxsize=None)
def case(N, M, D):
    """e and the fp64 reference of a shape; computed once, read-only."""
    e = rows(N, M, D, seed=1000 * N + 10 * M + D)
    return e, 10.0, reference(e, 10.0)


def device_run(e, w, scale=None):
    """(L, de, dw) of the op on the device through autograd; e a device tensor (any alignment)."""
    from autoformer_amd.ge2e import ge2e_loss

    ed = e.detach().requires_grad_(True)
    wd = torch.tensor(float(w), device=DEV, requires_grad=True)
    L = ge2e_loss(ed, e.shape[0], e.shape[1], wd)
    (L if scale is None else scale * L).backward()
    torch.cuda.synchronize()
    return L.item(), ed.grad.cpu().numpy(), wd.grad.item()


def errors(got, ref):
    return (abs(got[0] - ref[0]) / abs(ref[0]), rel_inf(got[1], ref[1]), abs(got[2] - ref[2]) / abs(ref[2]))


# ----------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("N,M,D", SHAPES)
def test_kernel_against_fp64(N, M, D):
    e, w, ref = case(N, M, D)
    got = device_run(e.to(DEV), w)
    errs = errors(got, ref)
    print("ge2e (%d, %d, %d): L %.6f, rel-inf L %.3e de %.3e dw %.3e" % ((N, M, D, got[0]) + errs))
    assert max(errs) < BAR, errs
    # (N*M, D) rows are the same problem
    from autoformer_amd.ge2e import ge2e_loss

    L2 = ge2e_loss(e.reshape(N * M, D).to(DEV), N, M, torch.tensor(w, device=DEV))
    assert L2.item() == got[0]


def test_forward_only_matches_and_keeps_no_gradient():
    from autoformer_amd import kernels as K

    e, w, ref = case(5, 3, 100)
    ed, wd = e.to(DEV), torch.tensor([w], device=DEV)
    L0, de0, dw0 = K.ge2e(ed, 5, 3, wd, grads=False)
    L1, de1, dw1 = K.ge2e(ed, 5, 3, wd, grads=True)
    assert de0 is None and dw0 is None and de1.shape == (15, 100)
    assert L0.item() == L1.item() and abs(L0.item() - ref[0]) / abs(ref[0]) < BAR


def test_upstream_gradient_is_honoured():
    e, w, ref = case(5, 3, 100)
    got = device_run(e.to(DEV), w, scale=3.0)
    errs = errors(got, (ref[0], 3.0 * ref[1], 3.0 * ref[2]))
    print("ge2e upstream 3.0: rel-inf L %.3e de %.3e dw %.3e" % errs)
    assert max(errs) < BAR, errs


def test_misaligned_e_gives_the_same_numbers():
    """A view at a 4-byte offset into a larger buffer: D % 4 == 0, but the base is not 16-byte aligned."""
    e, w, ref = case(5, 3, 100)
    buf = torch.zeros(e.numel() + 1, device=DEV)
    view = buf[1:].view(5, 3, 100)
    view.copy_(e)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = device_run(view, w)
    aligned = device_run(e.to(DEV), w)
    errs = errors(got, ref)
    print("ge2e misaligned: rel-inf L %.3e de %.3e dw %.3e; vs aligned de %.3e" % (errs + (rel_inf(got[1], aligned[1]),)))
    assert max(errs) < BAR, errs
    assert max(errors(got, aligned)) < BAR


def test_two_calls_are_bit_identical():
    from autoformer_amd import kernels as K

    for N, M, D in ((64, 10, 256), (4, 5, 257)):
        e, w, _ = case(N, M, D)
        ed, wd = e.to(DEV), torch.tensor([w], device=DEV)
        a = K.ge2e(ed, N, M, wd)
        b = K.ge2e(ed, N, M, wd)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("N,M,D", [(5, 3, 100), (4, 5, 257)])
def test_nothing_outside_the_outputs_is_written(N, M, D):
    """Guard regions around L, de, dw and the stated workspace keep their sentinel."""
    from autoformer_amd import _lib
    from autoformer_amd import kernels as K

    guard, S = 8, -768.0
    e, w, ref = case(N, M, D)
    ed, wd = e.to(DEV), torch.tensor([w], device=DEV)
    nws = int(_lib.lib().avc_ge2e_ws(N, M, D)) // 4
    sizes = {"L": 1, "de": N * M * D, "dw": 1, "ws": nws}
    bufs = {k: torch.full((n + 2 * guard,), S, device=DEV) for k, n in sizes.items()}
    v = {k: bufs[k][guard:guard + n] for k, n in sizes.items()}
    _lib.call("avc_ge2e", ed.data_ptr(), N, M, D, wd.data_ptr(), v["L"].data_ptr(), v["de"].data_ptr(),
              v["dw"].data_ptr(), v["ws"].data_ptr(), K.stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert (bufs[k][:guard] == S).all() and (bufs[k][guard + n:] == S).all(), k
    assert not (v["de"] == S).any()
    got = (v["L"].item(), v["de"].reshape(N, M, D).cpu().numpy(), v["dw"].item())
    assert max(errors(got, ref)) < BAR
    # the forward-only form: de and dw stay untouched
    for b in bufs.values():
        b.fill_(S)
    _lib.call("avc_ge2e", ed.data_ptr(), N, M, D, wd.data_ptr(), v["L"].data_ptr(), None, None, v["ws"].data_ptr(),
              K.stream())
    torch.cuda.synchronize()
    assert (bufs["de"] == S).all() and (bufs["dw"] == S).all()
    assert (bufs["ws"][:guard] == S).all() and (bufs["ws"][guard + nws:] == S).all()
    assert (bufs["L"][:guard] == S).all() and (bufs["L"][guard + 1:] == S).all() and v["L"].item() == got[0]


def test_scale_invariance():
    """Scaling every row by 7 leaves L unchanged (1e-6, relative) and divides de by 7 (1e-5, rel-inf)."""
    e, w, _ = case(64, 10, 256)
    a = device_run(e.to(DEV), w)
    b = device_run((7.0 * e).to(DEV), w)
    dL, dde = abs(a[0] - b[0]) / abs(a[0]), rel_inf(7.0 * b[1], a[1])
    print("ge2e rows x 7: L %.7f vs %.7f (rel %.3e), 7 de vs de rel-inf %.3e" % (a[0], b[0], dL, dde))
    assert dL < 1e-6 and dde < BAR


def test_identical_rows_of_one_speaker():
    e = rows(4, 3, 64, seed=7).clone()
    e[1] = e[1, 0]
    ref = reference(e, 10.0)
    got = device_run(e.to(DEV), 10.0)
    errs = errors(got, ref)
    print("ge2e identical rows: rel-inf L %.3e de %.3e dw %.3e" % errs)
    assert np.isfinite(got[1]).all() and max(errs) < BAR, errs


def test_a_zero_row_stays_finite():
    e = rows(3, 2, 40, seed=8).clone()
    e[2, 1] = 0.0
    L, de, dw = device_run(e.to(DEV), 10.0)
    assert np.isfinite(L) and np.isfinite(de).all() and np.isfinite(dw)


def test_wrapper_refusals():
    from autoformer_amd.ge2e import ge2e_loss

    w = torch.tensor(10.0, device=DEV)
    with pytest.raises(ValueError):
        ge2e_loss(torch.randn(6, 8, device=DEV), 4, 2, w)              # 6 rows are not 4 x 2
    with pytest.raises(ValueError):
        ge2e_loss(torch.randn(3, 8, device=DEV), 3, 1, w)              # M = 1
    with pytest.raises(TypeError):
        ge2e_loss(torch.randn(6, 8, device=DEV).bfloat16(), 3, 2, w)   # fp32 only


# ----------------------------------------------------------------------- the model under the loss
N_, M_, T_ = 3, 2, 24


@functools.lru_cache(maxsize=None)
def twin_state():
    """The twin's initial weights (nn.LSTM's own initialisation under a fixed seed); read-only."""
    torch.manual_seed(11)
    return {k: v.detach().clone() for k, v in RefDV().state_dict().items()}


@functools.lru_cache(maxsize=None)
def batches():
    g = torch.Generator().manual_seed(12)
    return tuple(torch.randn(N_ * M_, T_, 80, generator=g) for _ in range(3))


def twin(dtype=torch.float32):
    m = RefDV()
    m.load_state_dict(twin_state())
    return m.to(dtype), torch.nn.Parameter(torch.tensor(10.0, dtype=dtype))


def device_pair(comp):
    import autoformer_amd as A
    from autoformer_amd.factory.LstmDV import LstmDV
    from autoformer_amd.ge2e import GE2ELoss

    A.set_compute(comp)
    m = LstmDV()
    m.load_state_dict(twin_state())
    return m.to(DEV).train(), GE2ELoss().to(DEV)


def golden_of(named):
    """The dict grad_mismatches reads, from the twin's gradients."""
    g = {}
    for name, p in named:
        g["gnorm/" + name] = p.grad.detach().double().norm().item()
        g["ghead/" + name] = p.grad.detach().double().reshape(-1)[:64].numpy()
    return g


class _Named:
    def __init__(self, items):
        self.items = items

    def named_parameters(self):
        return self.items


@functools.lru_cache(maxsize=None)
def twin_step0():
    """loss, embeddings and the gradients of every parameter, of w and of x, of the twin's first step."""
    m, w = twin()
    x = batches()[0].clone().requires_grad_(True)
    emb = m(x)
    loss = restatement(emb.reshape(N_, M_, -1), w)
    loss.backward()
    return loss.item(), emb.detach().numpy(), golden_of(list(m.named_parameters()) + [("w", w), ("dx", x)])


def test_fp32_step_matches_the_twin():
    m, crit = device_pair("fp32")
    loss_ref, emb_ref, g = twin_step0()
    x = batches()[0].to(DEV).requires_grad_(True)
    emb = m(x)
    loss = crit(emb, N_, M_)
    loss.backward()
    torch.cuda.synchronize()
    print("fp32 step: loss %.6f vs twin %.6f, emb rel-inf %.3e" % (loss.item(), loss_ref,
                                                                 rel_inf(emb.detach().cpu().numpy(), emb_ref)))
    np.testing.assert_allclose(loss.item(), loss_ref, rtol=1e-4)
    named = list(m.named_parameters()) + [("w", crit.w), ("dx", x)]
    bad = grad_mismatches(_Named(named), g, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
    assert not bad, bad


def _twin_run(dtype):
    """Three steps of the twin with EmbedderStep's recipe on the CPU: losses, and step 0's gradients as
    the optimiser saw them (scaled and clipped)."""
    m, w = twin(dtype)
    params = list(m.parameters()) + [w]
    opt = torch.optim.Adam(params, lr=1e-4)
    losses, g0 = [], None
    for k, x in enumerate(batches()):
        loss = restatement(m(x.to(dtype)).reshape(N_, M_, -1), w)
        opt.zero_grad()
        loss.backward()
        w.grad.mul_(0.01)
        m.embedding.weight.grad.mul_(0.5)
        m.embedding.bias.grad.mul_(0.5)
        torch.nn.utils.clip_grad_norm_(params, 3.0)
        if k == 0:
            g0 = golden_of(list(m.named_parameters()) + [("w", w)])
        opt.step()
        with torch.no_grad():
            w.clamp_(min=1e-6)
        losses.append(loss.item())
    return losses, g0


@functools.lru_cache(maxsize=None)
def twin_runs():
    return _twin_run(torch.float32), _twin_run(torch.float64)


def test_three_embedder_steps_follow_the_twin():
    """Step 0 at the one-step bars; steps 1 and 2 within 10 x the twin's own fp32-to-fp64 difference, never
    below 1e-4 (Adam's first update is +-lr per element, so gradients near zero may flip sign: there is no
    derived bar for the later steps).  Measured on the MI355X: see DESIGN section 7."""
    from autoformer_amd.train_embedder import EmbedderStep

    (l32, g0), (l64, _) = twin_runs()
    m, crit = device_pair("fp32")
    step = EmbedderStep(m, crit)
    got = []
    for k, x in enumerate(batches()):
        got.append(step.step(x.to(DEV), N_, M_).item())
        if k == 0:
            torch.cuda.synchronize()
            named = list(m.named_parameters()) + [("w", crit.w)]
            bad = grad_mismatches(_Named(named), g0, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
            assert not bad, bad
    step.check()
    print("EmbedderStep path: %s" % step.path)
    for k in range(3):
        print("step %d: device %.7f twin fp32 %.7f fp64 %.7f |dev - fp32| %.3e |fp32 - fp64| %.3e"
              % (k, got[k], l32[k], l64[k], abs(got[k] - l32[k]), abs(l32[k] - l64[k])))
    np.testing.assert_allclose(got[0], l32[0], rtol=1e-4)
    for k in (1, 2):
        assert abs(got[k] - l32[k]) <= max(10 * abs(l32[k] - l64[k]), 1e-4), (k, got[k], l32[k], l64[k])
    assert crit.w.item() != 10.0 and crit.w.item() >= 1e-6


def test_sub_batches_give_the_one_pass_step():
    """The path the default shape takes (N = 64, M = 10 goes through the model as 8 passes of 80 rows): with
    the rows per pass forced to 2 for B = 6, one step's loss and every gradient the optimiser sees (scaled,
    clipped, accumulated over the three passes in sink mode) against the one-pass step of the same weights.
    fp32 with the deterministic kernels: rows are independent, so the passes differ from the one pass only
    in the order of the weight gradients' sums over the B T = 144 rows (three partial sums added up, and
    GEMMs of another height).  Bar: rel-inf 1e-4 per tensor -- 144 terms x 2^-24 is 8.6e-6 of the terms'
    magnitudes, with a factor of about 10 for sums that cancel; a pass left out or counted twice moves a
    gradient by about a third."""
    from autoformer_amd import kernels as K
    from autoformer_amd.train_embedder import EmbedderStep

    K.set_deterministic(True)
    x = batches()[0].to(DEV)
    runs = []
    for cap in (None, 2):
        m, crit = device_pair("fp32")
        step = EmbedderStep(m, crit)
        if cap is not None:
            step._cap[(N_ * M_, K.compute())] = cap
        loss = step.step(x, N_, M_).item()
        step.check()
        runs.append((loss, step.path, {n: p.grad.detach().cpu().numpy().copy()
                                       for n, p in list(m.named_parameters()) + [("w", crit.w)]},
                     step.flat.detach().cpu().numpy().copy()))
    (l1, p1, g1, f1), (l2, p2, g2, f2) = runs
    assert p1 == "one pass (B = 6)" and p2 == "3 sub-batches of at most 2 rows (B = 6)", (p1, p2)
    errs = {n: rel_inf(g2[n], g1[n]) for n in g1}
    worst = max(errs, key=errs.get)
    print("sub-batches: loss %.7f vs %.7f, worst gradient %s rel-inf %.3e, weights after the step rel-inf %.3e"
          % (l2, l1, worst, errs[worst], rel_inf(f2, f1)))
    assert abs(l2 - l1) <= 1e-6 * abs(l1)
    assert errs[worst] < 1e-4, errs


def test_bf16_mode():
    """Embeddings at the project's bf16 bar against the fp32 twin, finite gradients, and the kernel apart from
    the LSTM's rounding: the fp64 restatement of the device's own embeddings reproduces the device loss and de
    to 1e-5.  dw is held to the same 1e-5, of sum |dz S| -- the magnitudes of the terms it is the sum of, dz
    the gradient at the logits: these embeddings have not separated (every S is within 1e-2 of 1) and the dz
    of a row sum to zero, so dw is the small remainder of cancelling terms and its own magnitude says nothing
    about the error the fp32 rounding of S allows (measured: |dw| = 2.2e-4 beside sum |dz S| = 1.33; the
    error is 9.3e-5 of the former, 1.6e-8 of the latter)."""
    m, crit = device_pair("bf16")
    _, emb_ref, _ = twin_step0()
    x = batches()[0].to(DEV).requires_grad_(True)
    emb = m(x)
    emb.retain_grad()
    loss = crit(emb, N_, M_)
    loss.backward()
    torch.cuda.synchronize()
    err = rel_inf(emb.detach().cpu().numpy(), emb_ref)
    for name, p in list(m.named_parameters()) + [("w", crit.w), ("dx", x)]:
        assert torch.isfinite(p.grad).all(), name
    # the kernel apart from the LSTM's rounding: the device's own embeddings through the fp64 restatement
    ref = reference(emb.detach().cpu().reshape(N_, M_, -1), crit.w.item())
    got = (loss.item(), emb.grad.cpu().numpy().reshape(N_, M_, -1), crit.w.grad.item())
    errs = errors(got, ref)
    S = similarities(emb.detach().cpu().double().reshape(N_, M_, -1)).reshape(N_ * M_, N_)
    dz = (torch.softmax(crit.w.item() * S, 1) - F.one_hot(torch.arange(N_).repeat_interleave(M_), N_)) / (N_ * M_)
    dw_terms = (dz * S).abs().sum().item()
    print("bf16 step: emb rel-inf vs fp32 twin %.3e; kernel on its own embeddings: L %.3e de %.3e dw %.3e of |dw| = "
          "%.3e, %.3e of sum |dz S| = %.3e" % ((err,) + errs + (abs(ref[2]), abs(got[2] - ref[2]) / dw_terms, dw_terms)))
    assert err < 5e-2, err
    assert max(errs[:2]) < BAR, errs
    assert abs(got[2] - ref[2]) < BAR * dw_terms


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
def test_learning(comp):
    """6 speakers, speaker s a fixed envelope v_s ~ N(0, I_80), every frame v_s + 0.5 N(0, I); N = 4 of the 6
    per step, M = 3, T = 32, lr 1e-4, 10 steps: the last loss is below half the first (plain torch on the
    CPU goes from about 1.05 to at most 0.005)."""
    import autoformer_amd as A
    from autoformer_amd.factory.LstmDV import LstmDV
    from autoformer_amd.ge2e import GE2ELoss
    from autoformer_amd.train_embedder import EmbedderStep

    A.set_compute(comp)
    torch.manual_seed(3)
    m, crit = LstmDV().to(DEV).train(), GE2ELoss().to(DEV)
    step = EmbedderStep(m, crit, lr=1e-4)
    g = torch.Generator().manual_seed(4)
    env = torch.randn(6, 80, generator=g)
    losses = []
    for _ in range(10):
        spk = torch.randperm(6, generator=g)[:4]
        x = env[spk].repeat_interleave(3, 0)[:, None, :] + 0.5 * torch.randn(12, 32, 80, generator=g)
        losses.append(step.step(x.to(DEV), 4, 3).item())
    step.check()
    print("learning %s: %s (%s)" % (comp, " ".join("%.4f" % v for v in losses), step.path))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses


# ----------------------------------------------------------------------- bookkeeping
@pytest.fixture(scope="module")
def spmel(tmp_path_factory):
    return _tree(str(tmp_path_factory.mktemp("spmel")), {f"s{k}": [40 + k + u for u in range(7)] for k in range(4)})


def test_verification_eer_by_hand(spmel):
    from autoformer_amd.embed import cos_scores, embed_utterances
    from autoformer_amd.train_embedder import eer, verification_eer

    m, _ = device_pair("bf16")
    m.eval()
    got = verification_eer(m, spmel, enrol=5, len_crop=48)
    tg, nt, enrolled, trials = [], [], [], []
    for spk in sorted(os.listdir(spmel)):
        files = sorted(os.listdir(os.path.join(spmel, spk)))
        mels = [np.load(os.path.join(spmel, spk, f)) for f in files]
        enrolled.append(embed_utterances(m, mels[:5], 48).mean(0))
        trials.append(embed_utterances(m, mels[5:], 48))
    for k, tr in enumerate(trials):
        sc = cos_scores(tr, np.stack(enrolled))
        for row in sc:
            tg.append(row[k])
            nt += [v for j, v in enumerate(row) if j != k]
    assert got[1:] == (8, 24) and len(tg) == 8 and len(nt) == 24
    assert got[0] == eer(tg, nt)


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "autoformer_amd.train_embedder", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_checkpoint_loads_everywhere(spmel, tmp_path):
    from autoformer_amd.embed import build_metadata
    from autoformer_amd.factory.LstmDV import LstmDV

    out = str(tmp_path / "dv.ckpt")
    log = _cli("--spmel", spmel, "--out", out, "--speakers", "4", "--utterances", "2", "--partial", "24", "32",
               "--num_iters", "3", "--log_every", "1", "--eval_spmel", spmel, "--eval_every", "3")
    assert "[3/3] ge2e" in log and "EER" in log and os.path.exists(out + ".state")
    m = LstmDV()
    m.load_state_dict(torch.load(out, map_location="cpu", weights_only=True))   # as embed / evaluate / convert load it
    meta = build_metadata(spmel, m.to(DEV).eval(), num_uttrs=4, len_crop=48)
    assert len(meta) == 4 and all(np.isfinite(s[1]).all() and s[1].shape == (256,) for s in meta)


def test_cli_resume_continues_the_run(spmel, tmp_path):
    """4 iterations straight against 2 plus --resume for 2, fp32 with the deterministic kernels."""
    common = ["--spmel", spmel, "--speakers", "4", "--utterances", "2", "--partial", "24", "32", "--dtype", "fp32",
              "--deterministic", "--seed", "5"]
    a, b = str(tmp_path / "straight.ckpt"), str(tmp_path / "resumed.ckpt")
    _cli(*common, "--out", a, "--num_iters", "4")
    _cli(*common, "--out", b, "--num_iters", "2")
    log = _cli(*common, "--out", b, "--num_iters", "4", "--resume", b)
    assert "resumed" in log and "at iteration 2" in log
    sa = torch.load(a, map_location="cpu", weights_only=True)
    sb = torch.load(b, map_location="cpu", weights_only=True)
    worst = max(rel_inf(sb[k].numpy(), sa[k].numpy()) for k in sa)
    bitwise = all(torch.equal(sa[k], sb[k]) for k in sa)
    ta = torch.load(a + ".state", map_location="cpu", weights_only=True)
    tb = torch.load(b + ".state", map_location="cpu", weights_only=True)
    print("resume: worst rel-inf %.3e, bitwise %s, w %.7f vs %.7f" % (worst, bitwise, ta["w"].item(), tb["w"].item()))
    assert worst <= 1e-6
    assert ta["iteration"] == tb["iteration"] == 4 and ta["sampler"] == tb["sampler"]
    assert abs(ta["w"].item() - tb["w"].item()) <= 1e-6 * abs(ta["w"].item())
