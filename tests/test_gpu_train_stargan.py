"""CycleStep, StarGanSolver and the StarGAN trainer's command line on the device.

Everything as tests/test_gpu_train_gan.py: B = 2, T = 176, freq 22, closed-form (detinit) weights, fp32 unless said,
and the same two yardsticks:

* tests/golden/stargan_step.npz (and stargan_step_adain.npz): made once on the CPU from the reference's own
  modules (factory/AutoVC.py or AutoVC2.py, MetaDV.py with its random.randint replaced by the fixed window starts
  -- one set for the converted mel, one for the reconstruction --, Discriminator.py, three torch.optim.Adam) and the
  step expression of train_with_stargan.py:118-198, run as vc, cycle, vc, cycle (n_critic = 2, pretrained_step =
  0; AdaIN: vc, cycle) on detinit.det_inputs batches seed 1234, 1235, ...: the seven losses of every iteration, the
  norm of every parameter's gradient at the first cycle step, the BatchNorm running means after it, the norms of
  the three optimizers' updates.
* a plain-torch twin: test_gpu_train_gan.Twin with the cycle iteration added.  The fixture pins the twin (on the
  CPU: tests/test_cycle.py); the twin pins the step on the device.

Bars are that file's and for its reasons: a loss of a step from the twin's state to rtol 1e-4; gradients inside
helpers.grad_mismatches' bars, the zero-gradient conv biases by size (factor 4), D's conv1 head at 5e-2; the
free-running sequence to 1e-4 + 2 x the twin's own drift under 1e-2 rms gradient noise, computed here; update
norms to 2e-2; bf16 to twice the emulation's drift on the tensors behind each loss (c_reconst as c_loss, the cycle
MSE as the other two MSEs).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import metadv_torch as MT
from . import test_gpu_train_gan as G
from .conftest import GOLDEN
from .helpers import bits_equal

gpu = pytest.mark.gpu

DEV = G.DEV
LCYC = 1.0
LEFTS_TRANS = G.LEFTS
LEFTS_RECONST = [[7, 40, 19, 2], [33, 48, 0, 27]]
NAMES = ("l_id", "l_id_psnt", "l_cd", "c_trans", "c_reconst", "d_loss", "cycle")


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
class Twin(G.Twin):
    """train_with_stargan.py:118-198 in plain torch on the CPU: test_gpu_train_gan.Twin's state, optimizers, noise
    and bf16 emulation; step() with a target is the cycle iteration, lefts = (for the conversion, for the
    reconstruction).  Returns seven losses."""

    def step(self, x, e, target=None, lefts=None):
        if target is None:
            rows, grads, upd = super().step(x, e)
            return rows[:3] + [0.0] * 4, grads, upd
        xt, et = target
        rnd = MT.bf16_round if self.bf16 else MT._ident
        with self._cast():
            x_id, x_psnt, code_real = self.VC(x, e, e)
            code_re = self.VC(x_psnt, e, None)
            if self.adain:
                code_re = code_re[0]
        l_id, l_psnt = F.mse_loss(x, x_id.squeeze(1).float()), F.mse_loss(x, x_psnt.squeeze(1).float())
        l_cd = F.l1_loss(code_real.float(), code_re.float())
        with self._cast():
            if self.adain:
                _, tf = self.VC(x_psnt, et, None)
                _, x_conv, _ = self.VC(x, e, et, tf)
                x_conv = x_conv.squeeze(1).float()
                _, sf = self.VC(x, e, None)
                _, x_rec, _ = self.VC(x_conv, et, e, sf)
            else:
                _, x_conv, _ = self.VC(x, e, et)
                x_conv = x_conv.squeeze(1).float()
                _, x_rec, _ = self.VC(x_conv, et, e)
        x_rec = x_rec.squeeze(1).float()
        _, trans = MT.forward(self.c, x_conv, lefts[0], r=rnd)
        _, rec_style = MT.forward(self.c, x_rec, lefts[1], r=rnd)
        with self._cast():
            real, fake = self.Dc.disc_forward(self.d, xt), self.Dc.disc_forward(self.d, x_conv)
        ones = torch.ones(x.shape[0])
        c_trans, c_reconst = F.cosine_embedding_loss(trans, et, ones), F.cosine_embedding_loss(rec_style, e, ones)
        d_loss = self.Dc.discriminator_loss(real.float(), fake.float())
        cycle = F.mse_loss(x, x_rec)
        total = (l_id + l_psnt + G.LCD * l_cd + G.LCLS * (c_trans + c_reconst) + G.LDIS * d_loss + LCYC * cycle)
        aux = {"x_id": x_id, "x_psnt": x_psnt, "code_real": code_real, "code_re": code_re, "trans": trans,
               "rec_style": rec_style, "real": real, "fake": fake, "x_rec": x_rec}
        self.aux = {k: v.detach().float() for k, v in aux.items()}
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
        for o in self.opts:
            o.step()
        upd = [(torch.cat([p.detach().reshape(-1) for p in ps]) - b).double().norm().item()
               for ps, b in zip(self.params(), before)]
        return [v.item() for v in (l_id, l_psnt, l_cd, c_trans, c_reconst, d_loss, cycle)], grads, upd


def _bn_of(tw):
    return [{k: v.detach().clone() for k, v in sd.items() if "running" in k or "num_batches" in k}
            for sd in (tw.vc, tw.d)]


@functools.lru_cache(maxsize=None)
def twin_sequence(noise=None):
    """vc, cycle, vc, cycle as the fixture ran them; the first cycle step's gradients and the BatchNorm buffers
    after it.  noise: test_gpu_train_gan.Twin's."""
    tw = Twin(noise=noise)
    rows, upds, nb = [], [], 0
    for i in range(4):
        x, e = G.batch(nb)
        nb += 1
        if i % 2:
            rows_, grads, upd = tw.step(x, e, G.batch(nb), (LEFTS_TRANS[i // 2], LEFTS_RECONST[i // 2]))
            nb += 1
            if i == 1:
                g1, bn = grads, _bn_of(tw)
        else:
            rows_, _, upd = tw.step(x, e)
        rows.append(rows_)
        upds.append(upd)
    return np.array(rows), np.array(upds), g1, bn


@functools.lru_cache(maxsize=None)
def twin_fresh_cycle(adain=False, bf16=False):
    """A cycle step as the very first iteration: batch 0 the source, batch 1 the target."""
    tw = Twin(adain, bf16)
    rows, grads, _ = tw.step(*G.batch(0), G.batch(1), (LEFTS_TRANS[0], LEFTS_RECONST[0]))
    return rows, grads, _bn_of(tw), tw.aux


def bias_flip(g, tag, k):
    """How far a running mean recorded after the first cycle step may differ between two correct evaluations because
    of the conv bias in front of its BatchNorm.  That bias has an analytically zero gradient (a training-mode
    BatchNorm removes it), so what any arithmetic holds there is rounding noise of either sign, and Adam's first
    step of an element is -lr * sign(g) whatever the gradient's size: after the vc iteration's update two
    evaluations can hold biases 2 lr apart.  Nothing downstream sees that, but the BatchNorm's own batch mean moves
    with the bias, and the running mean (momentum 0.1) has taken (1 - 0.9^n) of it after the n forward calls that
    follow the update: n = the fixture's call count less the vc iteration's (two encoder calls, one of the decoder
    and postnet).  D's biases have not been updated when its statistics are recorded: 0."""
    if tag != "vc" or "running_mean" not in k:
        return 0.0
    calls = int(g[f"bn/{tag}/{k.replace('running_mean', 'num_batches_tracked')}"])
    n = calls - (2 if k.startswith("encoder.") else 1)
    return 2 * G.LR * (1 - 0.9 ** n)


def _bn_close(sd, g, tag, drift):
    """Running means and call counts of sd, recorded after the first cycle step, against the fixture's.  The bar of
    a running mean is test_gpu_train_gan's for the twin against its fixture (rel-inf 1e-3, and its reason) + what
    the zero-gradient bias in front of it can differ by (bias_flip) + SEQ_FACTOR x drift[k], the twin's own drift of
    that buffer under the gradient noise that stands for the distance between the two sides (bn_drift).  Call
    counts are exact."""
    keys = [k for k in sd if "running_mean" in k or "num_batches" in k]
    assert keys
    for k in keys:
        ref = g[f"bn/{tag}/{k}"]
        have = sd[k].detach().cpu().numpy()
        if "num_batches" in k:
            assert int(have) == int(ref), (k, have, ref)
            continue
        atol = 1e-6 + 1e-3 * np.abs(ref).max() + bias_flip(g, tag, k) + G.SEQ_FACTOR * drift[f"{tag}/{k}"]
        worst = float(np.abs(have - ref).max())
        print("bn %s/%s: off by %.3e, max |ref| %.3e, bar %.3e" % (tag, k, worst, np.abs(ref).max(), atol))
        np.testing.assert_allclose(have, ref, rtol=1e-4, atol=atol, err_msg=k)


def bn_drift(sigma):
    """Per BatchNorm buffer: how far the twin's value after the first cycle step (which follows one Adam update)
    moves when every VC gradient is perturbed before each Adam step by Gaussian noise of sigma x the tensor's rms,
    the worse of two seeds, max over the vector.  sigma = SEQ_SIGMA: the distance the gradient bars allow between
    the device's VC gradients and the twin's; FIX_SIGMA: between two CPUs' (fixture_bars)."""
    clean = twin_sequence()[3]
    out = {}
    for seed in (0, 1):
        noisy = twin_sequence(noise=(sigma, seed))[3]
        for tag, c, n in zip(("vc", "d"), clean, noisy):
            for k in c:
                d = float((n[k].double() - c[k].double()).abs().max())
                out[f"{tag}/{k}"] = max(out.get(f"{tag}/{k}", 0.0), d)
    return out


FIX_SIGMA = 1e-5


def fixture_bars():
    """The bar of every loss of the fixture against the twin: 1e-4, test_gpu_train_gan's bar for a step from the
    same state, + 2 x the twin's own relative drift when every VC gradient is perturbed before each Adam step by
    Gaussian noise of FIX_SIGMA = 1e-5 of the tensor's rms (the worse of two seeds).  The first iteration precedes
    every update and the second follows one, so their bars stay at about 1e-4; later ones do not.  Reason: the
    fixture was computed by one CPU's fp32 arithmetic and the twin runs on another's; the twin's VC gradient in fp32
    is 5e-6 (relative Frobenius norm) from its fp64 value, so two fp32 evaluations differ by up to about twice
    that, and Adam's early updates are lr * sign(g)-like, which turns a rounding-sized difference in a small
    gradient into a full step: under this noise d_loss at the fourth iteration moves by 2e-3 and c_reconst by
    2e-4, while the first two iterations move by under 1e-4."""
    rows = twin_sequence()[0]
    drift = np.zeros_like(rows)
    for seed in (0, 1):
        noisy = twin_sequence(noise=(FIX_SIGMA, seed))[0]
        drift = np.maximum(drift, np.abs(noisy - rows) / np.maximum(np.abs(rows), 1e-30))
    return 1e-4 + 2.0 * drift


def check_fixture_pins_the_twin():
    """On the CPU (called from tests/test_cycle.py): the twin reproduces what the reference's modules gave, every
    loss inside fixture_bars(), every running mean after the first cycle step inside _bn_close's bar for the same
    noise (two CPUs differ there as the device and the twin do, only by less)."""
    g = dict(np.load(os.path.join(GOLDEN, "stargan_step.npz")))
    rows, upds, g1, bn = twin_sequence()
    bars = fixture_bars()
    dev = np.abs(rows - g["losses"]) / np.maximum(np.abs(g["losses"]), 1e-30)
    print("twin losses\n", rows, "\nfixture\n", g["losses"], "\nrelative deviation\n", dev, "\nbars\n", bars)
    assert (bars[0] == 1e-4).all()
    assert (dev <= bars).all(), (dev, bars)
    np.testing.assert_allclose(upds, g["updates"], rtol=1e-2)
    assert (upds[0::2, 1:] == 0).all() and (g["updates"][0::2, 1:] == 0).all()     # a vc_step moves VC alone
    assert (g["losses"][0::2, 3:] == 0).all() and (g["losses"][1::2, 3:] > 0).all()
    assert g["lefts_trans"].tolist() == LEFTS_TRANS and g["lefts_reconst"].tolist() == LEFTS_RECONST
    worst = 0.0
    for tag, grads in zip(("vc", "c", "d"), g1):
        for k, v in grads.items():
            ref = float(g[f"gnorm/{tag}/{k}"])
            got = 0.0 if v is None else v.double().norm().item()
            if not (tag == "vc" and G.zero_grad_bias(k)):
                worst = max(worst, abs(got - ref) / max(ref, 1e-6))
            G._norm_close(tag, k, got, ref)
    print("worst gradient-norm deviation of the twin from the fixture: %.2e" % worst)
    assert float(g["gnorm/c/metablock.output.weight"]) == 0.0                      # linear2 gets no gradient
    drift = bn_drift(FIX_SIGMA)
    for tag, sd in zip(("vc", "d"), bn):
        _bn_close(sd, g, tag, drift)
    # a vc iteration (identity, re-pass), then identity, re-pass, conversion, cycle pass: the encoder's BatchNorms
    # saw 2 + 4 calls, the decoder's 1 + 3, D's 2
    assert int(g["bn/vc/encoder.convolutions.0.1.num_batches_tracked"]) == 2 + 4
    assert int(g["bn/vc/decoder.convolutions.0.1.num_batches_tracked"]) == 1 + 3
    assert int(g["bn/d/bn1.num_batches_tracked"]) == 2


def check_adain_fixture_pins_the_twin():
    g = dict(np.load(os.path.join(GOLDEN, "stargan_step_adain.npz")))
    tw = Twin(adain=True)
    rows0, _, _ = tw.step(*G.batch(0))
    rows1, grads, _ = tw.step(*G.batch(1), G.batch(2), (LEFTS_TRANS[0], LEFTS_RECONST[0]))
    np.testing.assert_allclose([rows0, rows1], g["losses"], rtol=1e-4)
    for tag, gr in zip(("vc", "c", "d"), grads):
        for k, v in gr.items():
            ref = float(g[f"gnorm/{tag}/{k}"])
            got = 0.0 if v is None else v.double().norm().item()
            G._norm_close(tag, k, got, ref)
    # the AdaIN cycle step runs the encoder twice more (the target's and the source's feature passes)
    assert int(g["bn/vc/encoder.convolutions.0.1.num_batches_tracked"]) == 2 + 6


# ----------------------------------------------------------------------- the step on the device
def _step(comp="fp32", adain=False, lr=G.LR):
    from autoformer_amd.train_stargan import CycleStep

    VC, C, Dm = G._modules(comp, adain)
    return CycleStep(VC, C, Dm, lr=lr, lambda_cd=G.LCD, lambda_cls=G.LCLS, lambda_dis=G.LDIS, lambda_cycle=LCYC,
                     use_adain=adain)


def _fresh(step):
    return [v.item() for v in step.cycle_step(*G._dev(0), *G._dev(1), LEFTS_TRANS[0], LEFTS_RECONST[0])]


def _report(what, got, rows):
    for name, a, b in zip(NAMES, got, rows):
        print("%s %s: device %.7f, twin %.7f, rel %.2e" % (what, name, a, b, abs(a - b) / max(abs(b), 1e-30)))


@gpu
def test_fresh_cycle_step_matches_the_twin():
    rows, grads, bn, _ = twin_fresh_cycle()
    step = _step()
    c_before = {k: v.detach().clone() for k, v in step.C.state_dict().items()}
    got = _fresh(step)
    step.check()                                                                    # the fault word is clean
    _report("cycle step", got, rows)
    np.testing.assert_allclose(got, rows, rtol=1e-4)
    bad = G._grad_check(step, grads)
    print("outside the gradient bars:", bad)
    assert not bad, bad
    # the running statistics of every BatchNorm: a missing or reordered forward call shows here
    for m, sd in zip((step.VC, step.D), bn):
        have = m.state_dict()
        assert sd
        for k, v in sd.items():
            np.testing.assert_allclose(have[k].detach().cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
    assert int(step.VC.state_dict()["encoder.convolutions.0.1.num_batches_tracked"]) == 4
    assert int(step.VC.state_dict()["decoder.convolutions.0.1.num_batches_tracked"]) == 3
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
    """Per iteration and loss: 1e-4 + SEQ_FACTOR x the twin's relative drift under gradient noise (the worse of two
    seeds), as test_gpu_train_gan.sequence_bars; the first iteration precedes every update, so its bar is 1e-4."""
    rows = twin_sequence()[0]
    drift = np.zeros_like(rows)
    for seed in (0, 1):
        noisy = twin_sequence(noise=(G.SEQ_SIGMA, seed))[0]
        drift = np.maximum(drift, np.abs(noisy - rows) / np.maximum(np.abs(rows), 1e-30))
    return 1e-4 + G.SEQ_FACTOR * drift


@gpu
def test_sequence_matches_the_twin_and_a_vc_step_leaves_the_critics_alone():
    """vc, cycle, vc, cycle as the fixture ran them, run freely: every iteration's seven losses inside
    sequence_bars(), every iteration's update norms against the twin's; a vc_step leaves C, D and their Adam state
    bit-equal; the BatchNorm running means after the first cycle step match the fixture inside _bn_close's bar.
    That step follows an Adam update, so the means carry the sign of the zero-gradient biases' rounding noise
    (bias_flip) and the distance between the device's VC gradients and the twin's (bn_drift(SEQ_SIGMA), the same
    noise as the losses').  Measured: decoder.convolutions.0.1.running_mean, whose entries are at most 0.031, is
    5.0e-5 off -- the size bias_flip gives, 5.4e-5 -- against a bar of 1.3e-4; the largest bar, the postnet's, is
    4.9e-2 of the largest entry, while a missing or reordered forward call moves a running mean by about a tenth
    of a batch mean."""
    g = dict(np.load(os.path.join(GOLDEN, "stargan_step.npz")))
    rows, upds, _, _ = twin_sequence()
    bars, drift = sequence_bars(), bn_drift(G.SEQ_SIGMA)
    step = _step()
    flats = (step.vc_flat, step.c_flat, step.d_flat)
    got, moved, nb = [], [], 0
    for i in range(4):
        x, e = G._dev(nb)
        nb += 1
        before = [f.clone() for f in flats]
        if i % 2:
            got.append([v.item() for v in step.cycle_step(x, e, *G._dev(nb), LEFTS_TRANS[i // 2], LEFTS_RECONST[i // 2])])
            nb += 1
            if i == 1:
                for tag, m in zip(("vc", "d"), (step.VC, step.D)):
                    _bn_close(m.state_dict(), g, tag, drift)
        else:
            state = [t.clone() for o in (step.c_opt, step.d_opt) for t in (o.flat, o.m, o.v, o.state)]
            parts = step.vc_step(x, e)
            torch.cuda.synchronize()
            now = [t for o in (step.c_opt, step.d_opt) for t in (o.flat, o.m, o.v, o.state)]
            assert all(bits_equal(a, b) for a, b in zip(state, now)), i             # C, D and their Adam state
            got.append([v.item() for v in parts] + [0.0] * 4)
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
def test_gradients_are_the_sum_of_the_parts():
    """lr = 0, so the weights stay: (a) the VC loss alone, (b) the conversion's terms alone (c_trans and d_loss
    through x_conv), (c) the cycle's terms alone (c_reconst and the cycle MSE through x_rec, which reaches back
    through the cycle pass's encoder into the conversion), (d) the whole cycle step.  Every encoder, decoder and
    postnet gradient of (d) is (a) + (b) + (c), and every gradient of C is (b)'s + (c)'s -- its two passes --, to
    1e-3 of the tensor's scale (fp32 sums in another order); no part is zero."""
    from autoformer_amd.critic import critic_loss_block
    from autoformer_amd.cycle import cycle_loss_block
    from autoformer_amd.layers import join_side

    step = _step(lr=0.0)
    (x, e), (xt, et) = G._dev(0), G._dev(1)
    vc_params, c_params = dict(step.VC.named_parameters()), dict(step.C.named_parameters())
    names = [n for n in vc_params if n.startswith(("encoder.", "decoder.", "postnet."))]
    assert len(names) == len(vc_params)

    def snap():
        join_side()
        torch.cuda.synchronize()
        return ({n: vc_params[n].grad.detach().clone() for n in names},
                {n: p.grad.detach().clone() for n, p in c_params.items()})

    step.vc_step(x, e)
    a, _ = snap()
    step._zero()
    _, x_conv, _ = step.VC(x, e, et)
    x_conv = x_conv.squeeze(1)
    _, trans = step.C(x_conv, lefts=LEFTS_TRANS[0])
    total, _, _ = critic_loss_block(trans, et, step.D(xt), step.D(x_conv), G.LCLS, G.LDIS)
    total.backward()
    b, cb = snap()
    step._zero()
    _, x_conv, _ = step.VC(x, e, et)
    x_conv = x_conv.squeeze(1)
    _, x_rec, _ = step.VC(x_conv, et, e)
    x_rec = x_rec.squeeze(1)
    _, rec_style = step.C(x_rec, lefts=LEFTS_RECONST[0])
    half = torch.full((2, 1), 0.5, device=DEV)
    _, _, c_reconst, _, cycle = cycle_loss_block(trans.detach(), et, rec_style, e, half, half, x, x_rec, G.LCLS,
                                                 G.LDIS, LCYC)
    (G.LCLS * c_reconst + LCYC * cycle).backward()
    c, cc = snap()
    step.cycle_step(x, e, xt, et, LEFTS_TRANS[0], LEFTS_RECONST[0])
    d, cd = snap()
    step.check()
    worst = ("", 0.0)
    for whole, parts in ((d, (a, b, c)), (cd, (cb, cc))):
        for n in whole:
            scale = max(float(whole[n].abs().max()), float(whole[n].norm()) / np.sqrt(whole[n].numel()), 1e-12)
            err = float((whole[n] - sum(p[n] for p in parts)).abs().max()) / scale
            worst = max(worst, (n, err), key=lambda v: v[1])
            assert err <= 1e-3, (n, err)
    # no part is zero: the decoder and postnet take all three, the encoder too; C's trained tensors both passes
    for n in names:
        if "conv.bias" not in n:                                                    # (a bias feeding a BatchNorm: zero)
            assert all(float(p[n].norm()) > 0 for p in (a, b, c)), n
    for n in ("metablock.dv.weight", "metablock.token_mixer.weight_ih_l0"):
        assert float(cb[n].norm()) > 0 and float(cc[n].norm()) > 0, n
    print("worst |whole - sum of parts| %.2e of scale (%s)" % (worst[1], worst[0]))


@gpu
def test_adain_cycle_step_matches_the_twin():
    rows, grads, _, _ = twin_fresh_cycle(adain=True)
    step = _step(adain=True)
    got = _fresh(step)
    step.check()
    _report("AdaIN cycle step", got, rows)
    np.testing.assert_allclose(got, rows, rtol=1e-4)
    bad = G._grad_check(step, grads)
    print("outside the gradient bars:", bad)
    assert not bad, bad
    assert int(step.VC.state_dict()["encoder.convolutions.0.1.num_batches_tracked"]) == 6


def _bf16_bars(f, m, rows_f):
    """test_gpu_train_gan._bf16_bars for the seven losses: its five (l_id, l_id_psnt, l_cd, c_loss as c_trans,
    d_loss), c_reconst by c_loss's bound on the reconstruction's style, and the cycle MSE by the MSE bound on x_rec:
    for y -> y + D, |change of mse(x, y)| <= 2 sqrt(mse) rms(D) + rms(D)^2.  Twice each."""
    five = G._bf16_bars(f, m, [rows_f[0], rows_f[1], rows_f[2], rows_f[3], rows_f[5]])

    def unit(v):
        return v / v.norm(dim=1, keepdim=True)

    rms = float((m["x_rec"] - f["x_rec"]).pow(2).mean().sqrt())
    c_reconst = 2 * float((unit(m["rec_style"]) - unit(f["rec_style"])).norm(dim=1).mean())
    cycle = 2 * (2 * np.sqrt(rows_f[6]) * rms + rms ** 2)
    return five[:4] + [c_reconst, five[4], cycle]


@gpu
def test_bf16_steps():
    """One cycle_step and one vc_step in the bf16 compute mode: finite losses, a clean fault word, and each loss of
    the cycle step within twice the CPU emulation's drift on the tensors behind it (_bf16_bars)."""
    rows_f, _, _, aux_f = twin_fresh_cycle()
    rows_m, _, _, aux_m = twin_fresh_cycle(bf16=True)
    bars = _bf16_bars(aux_f, aux_m, rows_f)
    step = _step("bf16")
    got = _fresh(step)
    parts = [v.item() for v in step.vc_step(*G._dev(2))]
    step.check()
    assert np.isfinite(got).all() and np.isfinite(parts).all()
    for name, g, f, m, bar in zip(NAMES, got, rows_f, rows_m, bars):
        print("bf16 %s: device %.6f, fp32 twin %.6f, emulation %.6f: deviation %.3e against bar %.3e"
              % (name, g, f, m, abs(g - f), bar))
    for name, g, f, bar in zip(NAMES, got, rows_f, bars):
        assert abs(g - f) <= bar, (name, g, f, bar)


# ----------------------------------------------------------------------- CLI
@gpu
def test_cli_trains_and_writes_the_three_files(tmp_path):
    """--synthetic --det_init --num_iters 4 --n_critic 2 in a child process: the seven keys in the reference's
    order, the cycle-only values 0.0 before the first cycle iteration and the latest one's after it, and three
    files that load into fresh modules."""
    import re

    import factory.AutoVC as FA
    import factory.Discriminator as FD
    import factory.MetaDV as FM

    name = str(tmp_path / "stargan")
    log = G._run("autoformer_amd.train_stargan", "--synthetic", "--det_init", "--num_iters", "4", "--n_critic", "2",
                 "--pretrained_step", "0", "--log_step", "1", "--num_speaker", "5", "--save_model_name", name)
    lines = [ln for ln in log.splitlines() if "Iteration [" in ln]
    assert len(lines) == 4, log
    keys = ["VC/loss_id", "VC/loss_id_psnt", "VC/loss_cd", "C/loss_trans", "C/loss_reconst", "D/loss", "Cycle/loss"]
    vals = []
    for ln in lines:
        assert re.findall(r"([A-Za-z]+/[a-z_]+):", ln) == keys, ln
        vals.append([float(v) for v in re.findall(r": ([-0-9.]+)", ln)])
    vals = np.array(vals)
    assert (vals[0, 3:] == 0).all() and (vals[1:, 3:] > 0).all() and (vals[:, :3] > 0).all(), log
    assert (vals[2, 3:] == vals[1, 3:]).all()                                       # the latest cycle iteration's
    assert " Lambda cycle --- 1" in log
    vc_sd = torch.load(name + ".pt", map_location="cpu", weights_only=True)
    FA.AutoVC(44, 256, 512, 22).load_state_dict(vc_sd)
    c_sd = torch.load(name + ".C.pt", map_location="cpu", weights_only=True)
    FM.MetaDV(5).load_state_dict(c_sd)
    FD.Discriminator().load_state_dict(torch.load(name + ".D.pt", map_location="cpu", weights_only=True))
    assert all(torch.isfinite(v).all() for sd in (vc_sd, c_sd) for v in sd.values() if v.is_floating_point())
