"""CriticStep, GanVer1Solver and the GAN trainer's command line on the device.

Everything at B = 2, T = 176, freq 22 with closed-form (detinit) weights, fp32 unless said.  Two yardsticks:

* tests/golden/gan_ver1_step.npz (and gan_ver1_step_adain.npz): made once on the CPU from the reference's own
  modules (factory/AutoVC.py or AutoVC2.py, MetaDV.py with its random.randint replaced by the fixed window
  starts, Discriminator.py, three torch.optim.Adam) and the step expression of train_with_gan_ver1.py:116-176,
  run as vc_step, critic_step, vc_step, critic_step (n_critic = 2, pretrained_step = 0) on detinit.det_inputs
  batches seed 1234, 1235, ...: the five losses of every iteration, the norm of every parameter's gradient at
  the first critic step, the BatchNorm running means after it, the norms of the three optimizers' updates.
* a plain-torch twin built here from oracle.autovc_cpu / oracle.variants_cpu, oracle.discriminator_cpu and
  tests/metadv_torch.py with torch.optim.Adam.  The fixture pins the twin (on the CPU, no GPU needed); the
  twin pins the step element by element on the device, where the reference does not exist.

Bars: a loss of a step taken from the same state as the twin's to rtol 1e-4 (test_gpu_disc.py's bar for the same
quantities); gradients inside helpers.grad_mismatches' bars (norm 1e-2, head 1e-2 of the tensor's scale), the
discriminator's conv1 head at test_gpu_disc.py's 5e-2 (it reads the converted mel through a LeakyReLU whose slope
flips where a pre-activation crosses zero).

One departure from "every gradient inside grad_mismatches' bars": a conv bias that feeds a training-mode
BatchNorm has an analytically zero gradient, and what any implementation holds there is the rounding of
sum_{b,t} dA, proportional to sum |dA|.  helpers.grad_mismatches gives such biases an absolute floor
(1e-6 + 1e-2 max |head|) sized for the plain VC step; with the critic's terms flowing back through the decoder the
reference's own value there is far above it (decoder.convolutions.0: norm 7.1e-5 in the fixture), and one
rounding noise cannot be compared with another element by element.  These biases are therefore taken out of the
helper's check and compared by size: the device's norm is at most ZERO_GRAD_FACTOR = 4 times the twin's (+ 1e-6).
That is looser than the helper's bar for them; less noise than the twin always passes, and the factor allows
for another summation order.

Losses after Adam updates (vc, critic, vc, critic run freely on the device against the twin run freely on the
CPU) are held to 1e-4 + SEQ_FACTOR x the twin's own drift when every VC gradient of the twin is perturbed, before
each Adam step, by Gaussian noise of SEQ_SIGMA = 1e-2 of the tensor's rms -- the distance the gradient bars above
allow between the device's gradients and the twin's (the worse of two noise seeds, times 2).  The bar is not a
constant because the sensitivity is not: Adam's early updates are lr * sign(g)-like, and d_loss at the fourth
iteration moves by several per cent under such noise while l_id moves by 1e-5.  The source of the distance is the
VC model's fp32-mode gradients, which differ from the twin's by about 1e-3 (relative Frobenius norm) already in a
plain vc_step, while the classifier's and the discriminator's are within 1e-5; the twin's own VC gradient is
well-conditioned (fp32 against fp64: 5e-6).  The update norms of the three optimizers are compared with the twin's
as well (2e-2), and what must not move is compared bit by bit.
"""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import metadv_torch as MT
from .conftest import GOLDEN, ROOT
from .helpers import bits_equal, grad_mismatches

gpu = pytest.mark.gpu

DEV = "cuda:0"
B_, T_, C_, LR = 2, 176, 5, 1e-4
LCD, LCLS, LDIS = 1.0, 0.1, 1.0
LEFTS = [[0, 16, 32, 48], [48, 5, 23, 11]]
ZERO_GRAD_FACTOR = 4.0   # zero-gradient biases: noise compared by size (module docstring: a stated departure)
SEQ_SIGMA, SEQ_FACTOR = 1e-2, 2.0


def zero_grad_bias(name):
    """A conv bias followed by a training-mode BatchNorm (every ConvNorm + BatchNorm1d pair of the VC families;
    the AdaIN postnet's feature_last_combine convs have no BatchNorm behind them)."""
    return "conv.bias" in name and "feature_last_combine" not in name


def _norm_close(tag, k, got, ref):
    if tag == "vc" and zero_grad_bias(k):
        assert got <= ZERO_GRAD_FACTOR * ref + 1e-6 and ref <= ZERO_GRAD_FACTOR * got + 1e-6, (tag, k, got, ref)
    else:
        assert abs(got - ref) <= 1e-3 * ref + 1e-6, (tag, k, got, ref)


@functools.lru_cache(maxsize=None)
def batch(k):
    from autoformer_amd.detinit import det_inputs

    x, e = det_inputs(B_, T_, seed=1234 + k)
    return torch.from_numpy(x), torch.from_numpy(e)


@pytest.fixture(autouse=True)
def _restore_modes():
    import autoformer_amd as A
    from autoformer_amd import kernels as K
    from autoformer_amd.layers import set_grad_sink

    yield
    A.set_compute("bf16")
    K.set_deterministic(False)
    set_grad_sink(False)


# ----------------------------------------------------------------------- the twin
def _c_state():
    import factory.MetaDV as M
    from autoformer_amd.detinit import det_init_

    m = M.MetaDV(C_)
    det_init_(m)
    return {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}


class Twin:
    """train_with_gan_ver1.py:116-176 in plain torch on the CPU over functional state_dicts."""

    def __init__(self, adain=False, bf16=False, noise=None):
        from oracle import autovc_cpu as A
        from oracle import discriminator_cpu as Dc
        from oracle import variants_cpu as V

        self.adain, self.bf16, self.A, self.Dc, self.V = adain, bf16, A, Dc, V
        self.vc = A.make_state(V.autovc2_spec() if adain else A.autovc_spec())
        self.c = _c_state()
        self.d = A.make_state(Dc.disc_spec())
        self.opts = [torch.optim.Adam(A.params_of(self.vc), LR), torch.optim.Adam(list(self.c.values()), LR),
                     torch.optim.Adam(A.params_of(self.d), LR)]
        # noise = (sigma, seed): every VC gradient gets sigma * rms * N(0, 1) added before each Adam step
        self.noise = None if noise is None else (noise[0], torch.Generator().manual_seed(noise[1]))

    def VC(self, x, c_org, c_trg, tf=None):
        if self.adain:
            return self.V.adain_forward("AutoVC2", self.vc, x, c_org, c_trg, tf)
        return self.A.autovc_forward(self.vc, x, c_org, c_trg)

    def params(self):
        return [self.A.params_of(self.vc), list(self.c.values()), self.A.params_of(self.d)]

    def _cast(self):
        # the bf16 compute mode's rounding points, emulated: autocast for VC and D, metadv_torch's `r` for C
        return torch.autocast("cpu", dtype=torch.bfloat16) if self.bf16 else contextlib.nullcontext()

    def step(self, x, e, target=None, lefts=None):
        """One iteration; with target = (x_target, target_style) the critic iteration.  Returns the five losses,
        the gradients by module (name -> tensor or None) and the update norms of the three optimizers."""
        with self._cast():
            x_id, x_psnt, code_real = self.VC(x, e, e)
            code_re = self.VC(x_psnt, e, None)
            if self.adain:
                code_re = code_re[0]
        l_id, l_psnt = F.mse_loss(x, x_id.squeeze(1).float()), F.mse_loss(x, x_psnt.squeeze(1).float())
        l_cd = F.l1_loss(code_real.float(), code_re.float())
        total = l_id + l_psnt + LCD * l_cd
        c_loss = d_loss = torch.zeros(())
        self.aux = {"x_id": x_id, "x_psnt": x_psnt, "code_real": code_real, "code_re": code_re}
        if target is not None:
            xt, et = target
            with self._cast():
                if self.adain:
                    _, tf = self.VC(x_psnt, et, None)
                    _, x_conv, _ = self.VC(x, e, et, tf)
                else:
                    _, x_conv, _ = self.VC(x, e, et)
            x_conv = x_conv.squeeze(1).float()
            _, trans = MT.forward(self.c, x_conv, lefts, r=MT.bf16_round if self.bf16 else MT._ident)
            with self._cast():
                real, fake = self.Dc.disc_forward(self.d, xt), self.Dc.disc_forward(self.d, x_conv)
            c_loss = F.cosine_embedding_loss(trans, et, torch.ones(x.shape[0]))
            d_loss = self.Dc.discriminator_loss(real.float(), fake.float())
            total = total + LCLS * c_loss + LDIS * d_loss
            self.aux.update(trans=trans, real=real, fake=fake)
        self.aux = {k: v.detach().float() for k, v in self.aux.items()}
        before = [torch.cat([p.detach().reshape(-1) for p in ps]) for ps in self.params()]
        for o in self.opts:
            o.zero_grad()
        total.backward()
        grads = [{k: (None if v.grad is None else v.grad.detach().clone()) for k, v in sd.items() if v.requires_grad}
                 for sd in (self.vc, self.c, self.d)]
        if self.noise is not None:
            sigma, gen = self.noise
            for p in self.params()[0]:
                p.grad.add_(sigma * p.grad.norm() / np.sqrt(p.numel()) * torch.randn(p.shape, generator=gen))
        for o in self.opts[:3 if target is not None else 1]:
            o.step()
        upd = [(torch.cat([p.detach().reshape(-1) for p in ps]) - b).double().norm().item()
               for ps, b in zip(self.params(), before)]
        return [v.item() for v in (l_id, l_psnt, l_cd, c_loss, d_loss)], grads, upd


def _gdict(grads, like):
    """A module's twin gradients in the form helpers.grad_mismatches reads (a missing gradient is zero)."""
    g = {}
    for k, v in grads.items():
        v = torch.zeros_like(like[k]) if v is None else v
        g["gnorm/" + k] = v.double().norm().item()
        g["ghead/" + k] = v.double().reshape(-1)[:64].numpy()
    return g


@functools.lru_cache(maxsize=None)
def twin_sequence(noise=None):
    """vc_step, critic_step, vc_step, critic_step as the fixture ran them; the first critic step's gradients and
    the BatchNorm buffers after it.  noise: Twin's."""
    tw = Twin(noise=noise)
    rows, upds, nb = [], [], 0
    for i in range(4):
        x, e = batch(nb)
        nb += 1
        if i % 2:
            rows_, grads, upd = tw.step(x, e, batch(nb), LEFTS[i // 2])
            nb += 1
            if i == 1:
                g1 = grads
                bn = [{k: v.detach().clone() for k, v in sd.items() if "running" in k or "num_batches" in k}
                      for sd in (tw.vc, tw.d)]
        else:
            rows_, _, upd = tw.step(x, e)
        rows.append(rows_)
        upds.append(upd)
    return np.array(rows), np.array(upds), g1, bn


@functools.lru_cache(maxsize=None)
def twin_fresh_critic(adain=False, bf16=False):
    """A critic step as the very first iteration: batch 0 the source, batch 1 the target."""
    tw = Twin(adain, bf16)
    x, e = batch(0)
    rows, grads, upd = tw.step(x, e, batch(1), LEFTS[0])
    bn = [{k: v.detach().clone() for k, v in sd.items() if "running" in k or "num_batches" in k} for sd in (tw.vc, tw.d)]
    return rows, grads, bn, tw.aux


def test_the_fixture_pins_the_twin():
    """On the CPU: the twin reproduces what the reference's modules gave.  (Update norms to 1e-2: Adam's first
    update of an element whose gradient is rounding noise is up to lr either way.)"""
    g = dict(np.load(os.path.join(GOLDEN, "gan_ver1_step.npz")))
    rows, upds, g1, bn = twin_sequence()
    print("twin losses\n", rows, "\nfixture\n", g["losses"])
    np.testing.assert_allclose(rows, g["losses"], rtol=1e-4)
    np.testing.assert_allclose(upds, g["updates"], rtol=1e-2)
    assert (upds[0::2, 1:] == 0).all() and (g["updates"][0::2, 1:] == 0).all()     # a vc_step moves VC alone
    assert g["lefts"].tolist() == LEFTS
    worst = 0.0
    for tag, grads in zip(("vc", "c", "d"), g1):
        for k, v in grads.items():
            ref = float(g[f"gnorm/{tag}/{k}"])
            got = 0.0 if v is None else v.double().norm().item()
            if not (tag == "vc" and zero_grad_bias(k)):
                worst = max(worst, abs(got - ref) / max(ref, 1e-6))
            _norm_close(tag, k, got, ref)
    print("worst gradient-norm deviation of the twin from the fixture: %.2e" % worst)
    assert float(g["gnorm/c/metablock.output.weight"]) == 0.0                      # linear2 gets no gradient
    for tag, sd in zip(("vc", "d"), bn):
        keys = [k for k in sd if "running_mean" in k or "num_batches" in k]
        assert keys
        for k in keys:
            # these calls came after an Adam update, whose lr * sign(g) steps follow the rounding of small
            # gradients, so the statistics differ from one CPU's arithmetic to another's by some 1e-5 of the
            # vector's scale, while a missing or reordered call moves a running mean by a tenth of a batch
            # mean.  Hence rel-inf 1e-3.
            ref = g[f"bn/{tag}/{k}"]
            np.testing.assert_allclose(sd[k].numpy(), ref, rtol=1e-4, atol=1e-6 + 1e-3 * np.abs(ref).max(), err_msg=k)
    # identity pass, encoder re-pass, conversion: the encoder's BatchNorms saw 3 calls, the decoder's 2, D's 2
    assert int(g["bn/vc/encoder.convolutions.0.1.num_batches_tracked"]) == 2 + 3
    assert int(g["bn/vc/decoder.convolutions.0.1.num_batches_tracked"]) == 1 + 2
    assert int(g["bn/d/bn1.num_batches_tracked"]) == 2


def test_the_adain_fixture_pins_the_twin():
    g = dict(np.load(os.path.join(GOLDEN, "gan_ver1_step_adain.npz")))
    tw = Twin(adain=True)
    rows0, _, _ = tw.step(*batch(0))
    rows1, grads, _ = tw.step(*batch(1), batch(2), LEFTS[0])
    np.testing.assert_allclose([rows0, rows1], g["losses"], rtol=1e-4)
    for tag, gr in zip(("vc", "c", "d"), grads):
        for k, v in gr.items():
            ref = float(g[f"gnorm/{tag}/{k}"])
            got = 0.0 if v is None else v.double().norm().item()
            _norm_close(tag, k, got, ref)
    # the AdaIN critic step runs the encoder a fourth time (the target's feature pass)
    assert int(g["bn/vc/encoder.convolutions.0.1.num_batches_tracked"]) == 2 + 4


# ----------------------------------------------------------------------- the step on the device
def _modules(comp="fp32", adain=False):
    import autoformer_amd as A
    from autoformer_amd.detinit import det_init_
    from factory.AutoVC import AutoVC
    from factory.AutoVC2 import AutoVC2
    from factory.Discriminator import Discriminator
    from factory.MetaDV import MetaDV

    A.set_compute(comp)
    mods = ((AutoVC2 if adain else AutoVC)(44, 256, 512, 22), MetaDV(C_), Discriminator())
    for m in mods:
        det_init_(m)
    return [m.to(DEV).train() for m in mods]


def _step(comp="fp32", adain=False, lr=LR):
    from autoformer_amd.train_gan import CriticStep

    VC, C, Dm = _modules(comp, adain)
    return CriticStep(VC, C, Dm, lr=lr, lambda_cd=LCD, lambda_cls=LCLS, lambda_dis=LDIS, use_adain=adain)


def _dev(k):
    return [v.to(DEV) for v in batch(k)]


def _grad_check(step, grads):
    """helpers.grad_mismatches' bars for every parameter but the zero-gradient biases (module docstring)."""
    bad = {}
    for tag, m, gr in zip(("vc", "c", "d"), (step.VC, step.C, step.D), grads):
        like = dict(m.named_parameters())
        g = _gdict(gr, {k: like[k].detach().cpu() for k in gr})
        b = grad_mismatches(m, g, bn_fed_bias=lambda n: False)
        if tag == "vc":
            for k in [k for k in like if zero_grad_bias(k)]:
                b.pop(k, None)
                got, ref = like[k].grad.double().norm().item(), g["gnorm/" + k]
                if got > ZERO_GRAD_FACTOR * ref + 1e-6:
                    b[k] = (got, ref, "zero-gradient bias: noise above %g x the twin's" % ZERO_GRAD_FACTOR)
        if tag == "d":
            b = {k: v for k, v in b.items() if not (k.startswith("conv1") and abs(v[0] - v[1]) <= 1e-2 * v[1] + 1e-6
                 and v[2] <= 5e-2 * max(np.abs(g["ghead/" + k]).max(), v[1] / np.sqrt(like[k].numel()), 1e-6))}
        bad.update({f"{tag}/{k}": v for k, v in b.items()})
    return bad


@gpu
def test_fresh_critic_step_matches_the_twin():
    rows, grads, bn, _ = twin_fresh_critic()
    step = _step()
    c_before = {k: v.detach().clone() for k, v in step.C.state_dict().items()}
    got = step.critic_step(*_dev(0), *_dev(1), LEFTS[0])
    step.check()                                                                    # the fault word is clean
    got = [v.item() for v in got]
    print("critic step losses %s\n             twin %s" % (got, rows))
    np.testing.assert_allclose(got, rows, rtol=1e-4)
    bad = _grad_check(step, grads)
    print("outside the gradient bars:", bad)
    assert not bad, bad
    # the running statistics of every BatchNorm: a missing or reordered forward call shows here
    for m, sd in zip((step.VC, step.D), bn):
        have = m.state_dict()
        assert sd
        for k, v in sd.items():
            np.testing.assert_allclose(have[k].detach().cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
    assert step.VC._decoder_bwd_done is None
    # what this loss gives no gradient does not move: linear2, and rows 0..86 of the mixer's output conv
    after = step.C.state_dict()
    for k in ("metablock.output.weight", "metablock.output.bias"):
        assert bits_equal(after[k], c_before[k]), k
    assert bits_equal(after["metablock.mlp.3.weight"][:87].contiguous(), c_before["metablock.mlp.3.weight"][:87].contiguous())
    assert not bits_equal(after["metablock.mlp.3.weight"][87:].contiguous(),
                          c_before["metablock.mlp.3.weight"][87:].contiguous())
    assert not bits_equal(after["metablock.dv.weight"], c_before["metablock.dv.weight"])


def sequence_bars():
    """Per iteration and loss: 1e-4 + SEQ_FACTOR x the twin's relative drift under gradient noise (module
    docstring), the worse of two seeds; the first iteration precedes every update, so its bar is 1e-4."""
    rows = twin_sequence()[0]
    drift = np.zeros_like(rows)
    for seed in (0, 1):
        noisy = twin_sequence(noise=(SEQ_SIGMA, seed))[0]
        drift = np.maximum(drift, np.abs(noisy - rows) / np.maximum(np.abs(rows), 1e-30))
    return 1e-4 + SEQ_FACTOR * drift


@gpu
def test_sequence_matches_the_twin_and_a_vc_step_leaves_the_critics_alone():
    """vc, critic, vc, critic as the fixture ran them, run freely: every iteration's five losses inside
    sequence_bars(), every iteration's update norms against the twin's (module docstring); a vc_step leaves C, D
    and their Adam state bit-equal."""
    rows, upds, _, _ = twin_sequence()
    bars = sequence_bars()
    step = _step()
    flats = (step.vc_flat, step.c_flat, step.d_flat)
    got, moved, nb = [], [], 0
    for i in range(4):
        x, e = _dev(nb)
        nb += 1
        before = [f.clone() for f in flats]
        if i % 2:
            got.append([v.item() for v in step.critic_step(x, e, *_dev(nb), LEFTS[i // 2])])
            nb += 1
        else:
            state = [t.clone() for o in (step.c_opt, step.d_opt) for t in (o.flat, o.m, o.v, o.state)]
            parts = step.vc_step(x, e)
            torch.cuda.synchronize()
            now = [t for o in (step.c_opt, step.d_opt) for t in (o.flat, o.m, o.v, o.state)]
            assert all(bits_equal(a, b) for a, b in zip(state, now)), i             # C, D and their Adam state
            got.append([v.item() for v in parts] + [0.0, 0.0])
        moved.append([(f - b).double().norm().item() for f, b in zip(flats, before)])
    step.check()
    got, moved = np.array(got), np.array(moved)
    dev = np.abs(got - rows) / np.maximum(np.abs(rows), 1e-30)
    print("sequence losses\n", got, "\ntwin\n", rows, "\nrelative deviation\n", dev, "\nbars\n", bars)
    print("update norms\n", moved, "\ntwin\n", upds)
    assert np.isfinite(got).all()
    assert (bars[0] == 1e-4).all()
    assert (dev <= bars).all(), (dev, bars)
    np.testing.assert_allclose(moved, upds, rtol=2e-2)
    assert (moved[0::2, 1:] == 0).all() and (moved[1::2] > 0).all()


@gpu
def test_decoder_gradients_are_the_sum_of_both_passes():
    """lr = 0, so the weights stay: (a) the VC loss alone, (b) the critic tail alone through the conversion pass,
    (c) the whole critic step.  Every decoder and postnet gradient of (c) is (a) + (b), to 1e-3 of the tensor's
    scale (fp32 sums in another order), and neither part is zero."""
    from autoformer_amd.critic import critic_loss_block
    from autoformer_amd.layers import join_side

    step = _step(lr=0.0)
    (x, e), (xt, et) = _dev(0), _dev(1)
    names = [n for n, _ in step.VC.named_parameters() if n.startswith(("decoder.", "postnet."))]
    params = dict(step.VC.named_parameters())

    def snap():
        torch.cuda.synchronize()
        return {n: params[n].grad.detach().clone() for n in names}

    step.vc_step(x, e)
    a = snap()
    step._zero()
    _, x_conv, _ = step.VC(x, e, et)
    x_conv = x_conv.squeeze(1)
    _, trans = step.C(x_conv, lefts=LEFTS[0])
    total, _, _ = critic_loss_block(trans, et, step.D(xt), step.D(x_conv), LCLS, LDIS)
    total.backward()
    join_side()
    b = snap()
    step.critic_step(x, e, xt, et, LEFTS[0])
    c = snap()
    step.check()
    worst = ("", 0.0)
    for n in names:
        scale = max(float(c[n].abs().max()), float(c[n].norm()) / np.sqrt(c[n].numel()), 1e-12)
        err = float((c[n] - (a[n] + b[n])).abs().max()) / scale
        worst = max(worst, (n, err), key=lambda v: v[1])
        assert err <= 1e-3, (n, err)
        if "conv.bias" not in n:                                                    # (a bias feeding a BatchNorm: zero)
            assert float(a[n].norm()) > 0 and float(b[n].norm()) > 0, n
    print("decoder/postnet: worst |c - (a + b)| %.2e of scale (%s)" % (worst[1], worst[0]))


@gpu
def test_adain_critic_step_matches_the_twin():
    rows, grads, _, _ = twin_fresh_critic(adain=True)
    step = _step(adain=True)
    got = [v.item() for v in step.critic_step(*_dev(0), *_dev(1), LEFTS[0])]
    step.check()
    print("AdaIN critic step losses %s\n                   twin %s" % (got, rows))
    np.testing.assert_allclose(got, rows, rtol=1e-4)
    bad = _grad_check(step, grads)
    print("outside the gradient bars:", bad)
    assert not bad, bad


def _bf16_bars(f, m, rows_f):
    """Twice what the emulation's drift can change each loss by, with the drift measured in a norm that does not
    cancel (as the MetaDV tests measure theirs): for y -> y + D,
      mse(x, y):  |change| <= 2 sqrt(mse) rms(D) + rms(D)^2                               (Cauchy-Schwarz)
      l1(a, b):   |change| <= mean |D_a| + mean |D_b|
      c_loss:     |change| <= mean_b || D of the unit-norm style ||                       (the target has unit norm)
      d_loss:     |change| <= mean |D log p_real| + mean |D log(1 - p_fake)|
    f, m: the tensors behind the fp32 twin's and the emulation's losses."""
    def rms(k):
        return float((m[k] - f[k]).pow(2).mean().sqrt())

    def unit(v):
        return v / v.norm(dim=1, keepdim=True)

    bars = [2 * np.sqrt(rows_f[0]) * rms("x_id") + rms("x_id") ** 2, 2 * np.sqrt(rows_f[1]) * rms("x_psnt") + rms("x_psnt") ** 2,
            float((m["code_real"] - f["code_real"]).abs().mean() + (m["code_re"] - f["code_re"]).abs().mean()),
            float((unit(m["trans"]) - unit(f["trans"])).norm(dim=1).mean()),
            float((m["real"].log() - f["real"].log()).abs().mean()
                  + (torch.log1p(-m["fake"]) - torch.log1p(-f["fake"])).abs().mean())]
    return [2 * b for b in bars]


@gpu
def test_bf16_steps():
    """One critic_step and one vc_step in the bf16 compute mode: finite losses, a clean fault word, and each loss
    of the critic step within twice the CPU emulation of the mode's rounding points (the twin under bf16 autocast,
    MetaDV with metadv_torch's rounding) -- test_gpu_disc.py's bf16 step test sets no bar of its own.  The
    emulation's drift is measured on the tensors behind each loss (_bf16_bars), as the MetaDV tests measure
    theirs on the output vectors, not on the scalar loss: a mean's signed drift cancels by chance (the emulation
    moves l_id by 7.7e-5 and l_id_psnt, the same tensor plus the postnet, by 3.8e-5), so twice one sample of it is
    no envelope for another implementation's rounding.  The bound is looser than the scalar one; DESIGN section 7
    lists the resulting bars beside the deviations."""
    rows_f, _, _, aux_f = twin_fresh_critic()
    rows_m, _, _, aux_m = twin_fresh_critic(bf16=True)
    bars = _bf16_bars(aux_f, aux_m, rows_f)
    step = _step("bf16")
    got = [v.item() for v in step.critic_step(*_dev(0), *_dev(1), LEFTS[0])]
    parts = [v.item() for v in step.vc_step(*_dev(2))]
    step.check()
    assert np.isfinite(got).all() and np.isfinite(parts).all()
    names = ("l_id", "l_id_psnt", "l_cd", "c_loss", "d_loss")
    for name, g, f, m, bar in zip(names, got, rows_f, rows_m, bars):
        print("bf16 %s: device %.6f, fp32 twin %.6f, emulation %.6f: deviation %.3e against bar %.3e"
              % (name, g, f, m, abs(g - f), bar))
    for name, g, f, bar in zip(names, got, rows_f, bars):
        assert abs(g - f) <= bar, (name, g, f, bar)


# ----------------------------------------------------------------------- CLI
def _run(module, *args, limit=240):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", module, *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=limit)
    assert r.returncode == 0, r.stdout + r.stderr                                  # stop at the first failure
    return r.stdout


@gpu
def test_cli_trains_from_a_classifier_checkpoint(tmp_path):
    """train_classifier for 2 iterations on a generated 4-speaker tree, then train_gan on its checkpoint: the
    three saved files load into fresh modules, VC's keys are the reference layout's, and C/loss_trans is logged
    nonzero from iteration 2 on."""
    import re

    import factory.AutoVC as FA
    import factory.Discriminator as FD
    import factory.MetaDV as FM
    from oracle.autovc_cpu import autovc_spec

    from .test_gpu_train_classifier import _speaker_tree

    spmel = _speaker_tree(str(tmp_path / "spmel"))
    ckpt, name = str(tmp_path / "c.ckpt"), str(tmp_path / "gan")
    _run("autoformer_amd.train_classifier", "--spmel", spmel, "--out", ckpt, "--batch", "4", "--num_iters", "2",
         "--dtype", "fp32", "--det_init")
    log = _run("autoformer_amd.train_gan", "--synthetic", "--det_init", "--num_iters", "4", "--n_critic", "2",
               "--pretrained_step", "0", "--log_step", "1", "--classifier_ckpt", ckpt, "--save_model_name", name)
    lines = [ln for ln in log.splitlines() if "Iteration [" in ln]
    assert len(lines) == 4, log
    trans = [float(re.search(r"C/loss_trans: ([-0-9.]+)", ln).group(1)) for ln in lines]
    dl = [float(re.search(r"D/loss: ([-0-9.]+)", ln).group(1)) for ln in lines]
    assert trans[0] == 0.0 and dl[0] == 0.0 and all(v > 0 for v in trans[1:]) and all(v > 0 for v in dl[1:]), log
    assert trans[2] == trans[1]                                                     # the latest critic iteration's
    for key in ("VC/loss_id", "VC/loss_id_psnt", "VC/loss_cd"):
        assert all(key in ln for ln in lines)
    vc_sd = torch.load(name + ".pt", map_location="cpu", weights_only=True)
    assert list(vc_sd) == list(autovc_spec())                                       # the reference layout's keys
    FA.AutoVC(44, 256, 512, 22).load_state_dict(vc_sd)
    c_sd = torch.load(name + ".C.pt", map_location="cpu", weights_only=True)
    assert c_sd["metablock.output.weight"].shape[0] == 4                            # the checkpoint's class count
    FM.MetaDV(4).load_state_dict(c_sd)
    FD.Discriminator().load_state_dict(torch.load(name + ".D.pt", map_location="cpu", weights_only=True))
    assert all(torch.isfinite(v).all() for sd in (vc_sd, c_sd) for v in sd.values() if v.is_floating_point())
