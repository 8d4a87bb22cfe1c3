"""ClassifierStep, validate and the classifier trainer's command line on the device.

The yardstick of the fp32 step is the plain-torch twin of tests/metadv_torch.py on the CPU with the same
closed-form weights, F.cross_entropy, torch's clip_grad_norm_ and torch.optim.Adam, at the bars of
test_gpu_metadv.py::test_fp32_training_step_matches_fixture: the loss to rtol 1e-5, every gradient's norm to
1e-2 and its first 64 elements to 1e-2 of the tensor's scale (helpers.grad_mismatches).

The parameters after the step: Adam's first update is -lr g / (|g| + eps), so an element moves by lr in the
direction of its gradient's sign, and an element whose gradient is rounding noise may move either way.  The
update u = p_after - p_before is therefore compared where the twin's gradient is at least a tenth of the
tensor's scale (the scale grad_mismatches uses: max(max |head|, norm / sqrt(numel))): a gradient inside the
1e-2 bar is then within 10 % of the twin's, cannot change sign, and moves u by at most lr * 0.1 / 4 (the
derivative of g / (|g| + eps) is eps / (|g| + eps)^2 <= 1 / (4 |g|)); with the rounding of the two parameters
(2^-24 of values below 1, 6e-4 lr each) the bar is 0.03 lr.  Everywhere, |u| <= lr (1 + 1e-3)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import metadv_torch as MT
from .conftest import ROOT
from .helpers import grad_mismatches, rel_inf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B_, T_, C_, LR, CLIP = 2, 128, 5, 1e-4, 3.0
LEFTS = [0, 0, 0, 0]  # T = crop_len: the only windows there are
LABELS = [1, 3]


@pytest.fixture(autouse=True)
def _restore_modes():
    import autoformer_amd as A
    from autoformer_amd import kernels as K
    from autoformer_amd.layers import set_grad_sink

    yield
    A.set_compute("bf16")
    K.set_deterministic(False)
    set_grad_sink(False)


def _model(C=C_):
    import factory.MetaDV as M
    from autoformer_amd.detinit import det_init_

    m = M.MetaDV(C)
    det_init_(m)
    return m


@functools.lru_cache(maxsize=None)
def _x():
    from autoformer_amd.detinit import det_inputs

    return torch.from_numpy(det_inputs(B_, T_)[0])


@functools.lru_cache(maxsize=None)
def twin_step():
    """One step of the twin on the CPU: loss, the clipped gradients, the parameters before and after."""
    sd = {k: v.detach().clone() for k, v in _model().state_dict().items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pred, _ = MT.forward(leaves, _x(), LEFTS)
    loss = F.cross_entropy(pred, torch.tensor(LABELS))
    loss.backward()
    params = list(leaves.values())
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    grads = {k: v.grad.detach().clone() for k, v in leaves.items()}
    g = {}
    for k, v in grads.items():
        g["gnorm/" + k] = v.double().norm().item()
        g["ghead/" + k] = v.double().reshape(-1)[:64].numpy()
    torch.optim.Adam(params, lr=LR).step()
    return loss.item(), g, grads, sd, {k: v.detach().clone() for k, v in leaves.items()}


def test_fp32_step_matches_the_twin():
    import autoformer_amd as A
    from autoformer_amd import kernels as K
    from autoformer_amd.train_classifier import ClassifierStep
    from autoformer_amd.xent import SoftmaxXent

    A.set_compute("fp32")
    loss_ref, g, grads_ref, before, after_ref = twin_step()
    m = _model().to(DEV).train()
    step = ClassifierStep(m, SoftmaxXent(), lr=LR, clip=CLIP)
    loss, correct = step.step(_x().to(DEV), K.Labels(LABELS, C_, DEV), LEFTS)
    step.check()
    print("fp32 classifier step: loss %.7f vs twin %.7f, correct %d" % (loss.item(), loss_ref, correct.item()))
    assert loss.is_cuda and correct.is_cuda and 0 <= correct.item() <= B_
    np.testing.assert_allclose(loss.item(), loss_ref, rtol=1e-5)
    bad = grad_mismatches(m, g, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)   # the clipped gradients
    assert not bad, bad
    worst, least = ("", 0.0), ("", 1.0)
    for name, p in m.named_parameters():
        u = p.detach().cpu() - before[name]
        u_ref = after_ref[name] - before[name]
        assert float(u.abs().max()) <= LR * (1 + 1e-3), name
        gr = grads_ref[name]
        scale = max(float(gr.reshape(-1)[:64].abs().max()), float(gr.double().norm()) / np.sqrt(gr.numel()), 1e-6)
        mask = gr.abs() >= 0.1 * scale
        if mask.any():
            err = float((u - u_ref)[mask].abs().max()) / LR
            worst = max(worst, (name, err), key=lambda v: v[1])
            assert err <= 0.03, (name, err)
        least = min(least, (name, float(mask.float().mean())), key=lambda v: v[1])
    print("fp32 classifier step: worst update error %.3e lr (%s); smallest compared share %.3f (%s)" % (worst[1], worst[0],
                                                                                                    least[1], least[0]))
    # only output channel 87 of the mixer's last conv is consumed: its other channels do not move
    assert float((m.metablock.mlp[3].weight.detach().cpu() - before["metablock.mlp.3.weight"])[:87].abs().max()) == 0.0


def _speaker_tree(root, speakers=4, utterances=6, frames=200, seed=0):
    """<root>/s<k>/u<i>.npy: speaker k a fixed envelope v_k ~ N(0, I_80), every frame v_k + 0.5 N(0, I)."""
    g = torch.Generator().manual_seed(seed)
    env = torch.randn(speakers, 80, generator=g)
    for k in range(speakers):
        os.makedirs(os.path.join(root, f"s{k}"))
        for u in range(utterances):
            mel = env[k][None, :] + 0.5 * torch.randn(frames, 80, generator=g)
            np.save(os.path.join(root, f"s{k}", f"u{u:02d}.npy"), mel.numpy().astype(np.float32))
    return root


@pytest.fixture(scope="module")
def spmel(tmp_path_factory):
    return _speaker_tree(str(tmp_path_factory.mktemp("spmel")))


def test_bf16_steps_and_learning(spmel):
    """Three steps run with a finite loss and a clean fault probe; then, to 30 steps in all on the 4-speaker
    tree (B = 4, T = 128, lr 1e-4; one fixed seed, 3, for the weights and the sampler: a smoke check, not a
    measurement), the last loss is below the first."""
    import autoformer_amd as A
    import factory.MetaDV as M
    from autoformer_amd.train_classifier import ClassifierStep, UtteranceBatches
    from autoformer_amd.xent import SoftmaxXent

    A.set_compute("bf16")
    torch.manual_seed(3)
    m = M.MetaDV(4).to(DEV).train()
    batches = UtteranceBatches(spmel, 4, 128, val_every=3, seed=3)
    step = ClassifierStep(m, SoftmaxXent(), lr=1e-4)
    losses = []
    for k in range(30):
        x, labels, lefts = next(batches)
        loss, correct = step.step(torch.from_numpy(x).to(DEV), labels, lefts)
        losses.append(loss)
        if k == 2:
            step.check()
            assert all(np.isfinite(v.item()) for v in losses)
    step.check()
    losses = [v.item() for v in losses]
    print("bf16 classifier: %s" % " ".join("%.4f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    for name, p in m.named_parameters():
        assert torch.isfinite(p).all(), name


def test_validate_is_the_row_by_row_loop(spmel):
    import autoformer_amd as A
    from autoformer_amd.train_classifier import UtteranceBatches, centre_crop, even_lefts, validate

    A.set_compute("fp32")
    m = _model(4).to(DEV).eval()
    batches = UtteranceBatches(spmel, 4, 176, val_every=3, seed=0)
    assert len(batches.val) == 8
    top1, loss, n = validate(m, batches, max_batch=3)                            # batches of 3, 3 and 2
    lefts = even_lefts(176, 128, 4)
    assert lefts == [0, 16, 32, 48]
    hits, total = 0, 0.0
    with torch.no_grad():
        for label, f in batches.val:
            x = torch.from_numpy(np.ascontiguousarray(centre_crop(np.load(f), 176)))[None].to(DEV)
            pred, _ = m(x, lefts=lefts)
            hits += int(pred[0].argmax().item() == label)
            total += F.cross_entropy(pred.double().cpu(), torch.tensor([label])).item()
    print("validate: top-1 %.3f (loop %.3f), loss %.6f (loop %.6f), n %d" % (top1, hits / 8, loss, total / 8, n))
    assert n == 8 and top1 == hits / 8
    np.testing.assert_allclose(loss, total / 8, rtol=1e-4)
    empty = UtteranceBatches(spmel, 4, 176, val_every=10, seed=0)                # six utterances: nothing held out
    assert validate(m, empty)[2] == 0


def _run(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", module, *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_checkpoint_loads_and_resume_is_bit_identical(spmel, tmp_path):
    """Fresh child processes: 4 iterations straight; the checkpoint loads into MetaDV(4) and into `embed
    --embedder MetaDV`; 2 iterations plus --resume to 4 write the same bits (fp32, deterministic kernels)."""
    import json
    import pickle

    import factory.MetaDV as M

    common = ["--spmel", spmel, "--batch", "4", "--det_init", "--deterministic", "--dtype", "fp32", "--save_every", "2",
              "--log_every", "1"]
    a, b = str(tmp_path / "straight.ckpt"), str(tmp_path / "resumed.ckpt")
    log = _run("autoformer_amd.train_classifier", *common, "--out", a, "--num_iters", "4")
    assert "[4/4] xent" in log and os.path.exists(a + ".state")
    assert json.load(open(a + ".speakers.json")) == ["s0", "s1", "s2", "s3"]
    sa = torch.load(a, map_location="cpu", weights_only=True)
    m = M.MetaDV(4)
    m.load_state_dict(sa)                                                         # as the GAN trainers would load C
    assert all(torch.isfinite(v).all() for v in sa.values())
    pkl = str(tmp_path / "train.pkl")
    _run("autoformer_amd.embed", "--spmel", spmel, "--embedder", "MetaDV", "--num_classes", "4", "--ckpt", a,
         "--num_uttrs", "6", "--out", pkl)
    meta = pickle.load(open(pkl, "rb"))
    assert len(meta) == 4 and all(np.isfinite(s[1]).all() and s[1].shape == (256,) for s in meta)

    _run("autoformer_amd.train_classifier", *common, "--out", b, "--num_iters", "2")
    log = _run("autoformer_amd.train_classifier", *common, "--out", b, "--num_iters", "4", "--resume", b)
    assert "resumed" in log and "at iteration 2" in log
    sb = torch.load(b, map_location="cpu", weights_only=True)
    worst = max(rel_inf(sb[k].numpy(), sa[k].numpy()) for k in sa)
    bitwise = all(torch.equal(sa[k], sb[k]) for k in sa)
    ta = torch.load(a + ".state", map_location="cpu", weights_only=True)
    tb = torch.load(b + ".state", map_location="cpu", weights_only=True)
    print("resume: worst rel-inf %.3e, bitwise %s" % (worst, bitwise))
    assert ta["iteration"] == tb["iteration"] == 4 and ta["sampler"] == tb["sampler"]
    assert bitwise, worst
    assert torch.equal(ta["adam_m"], tb["adam_m"]) and torch.equal(ta["adam_v"], tb["adam_v"])
