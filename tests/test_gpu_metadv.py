"""The MetaDV speaker classifier on the device against the reference fixture (tests/golden/metadv.npz),
at the full MetaDV dimensions and B = 2 or 3: the training composition in fp32 parity mode (outputs,
per-length rows, one training step's gradients), the seeded window draw, the forward-only bf16 path,
its agreement with the training composition, the bf16 training step, and embed_utterances.

The bf16 bar is not a constant: it is 2 x d_emu, where d_emu is the rel-inf distance from the same
fixture of a CPU emulation of the bf16 path's rounding points (tests/metadv_torch.py::emulate_bf16:
bf16 weights, bf16 h, bf16 conv and mixer operands, fp32 head), computed when the test runs -- the
construction of tests/test_gpu_lstmdv.py.  The factor 2 covers what the emulation leaves out: the
v_exp / v_rcp forms of the activations and the GEMMs' accumulation order.  A window one frame off
moves d_vec by more than 1e-2 of its largest entry even in fp32 (tests/test_metadv.py asserts it).
Measured on an MI355X (cases 176 / 128 / lens): forward-only d_vec rel-inf 4.6e-3 / 7.1e-3 / 5.5e-3 with
d_emu 5.0e-3 / 6.9e-3 / 6.4e-3; fp32 mode 1.0e-6 / 1.8e-6 / 2.1e-6."""
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import metadv_torch as MT
from .helpers import grad_mismatches, rel_inf
from .test_metadv import golden, ref_state, x200

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def _model():
    import factory.MetaDV as M
    from autoformer_amd.detinit import det_init_

    m = M.MetaDV(256)
    det_init_(m)
    return m.to(DEV).train()


def _cases():
    """name -> (x, lens, lefts, pred, dvec) of the fixture."""
    g = golden()
    return {"176": (g["x176"], None, [int(v) for v in g["lefts176"]], g["pred176"], g["dvec176"]),
            "128": (g["x176"][:, :128].copy(), None, [0, 0, 0, 0], g["pred128"], g["dvec128"]),
            "lens": (x200(), [int(v) for v in g["lens200"]], g["lefts200"].tolist(), g["pred200"], g["dvec200"])}


@functools.lru_cache(maxsize=None)
def _d_emu(case):
    """rel-inf drift (pred, d_vec) of the bf16 emulation from the fixture."""
    x, lens, lefts, pred, dvec = _cases()[case]
    p, d = MT.emulate_bf16(ref_state(), torch.from_numpy(x), lefts, lens)
    return rel_inf(p.numpy(), pred), rel_inf(d.numpy(), dvec)


def _run(m, case):
    x, lens, lefts, _, _ = _cases()[case]
    with torch.no_grad():
        pred, dvec = m(torch.from_numpy(x).to(DEV), lens, lefts=lefts)
    return pred.cpu().numpy(), dvec.cpu().numpy()


def test_fp32_outputs_match_fixture():
    import autoformer_amd as A

    A.set_compute("fp32")
    m = _model()
    for case, (_, _, _, pred, dvec) in _cases().items():
        p, d = _run(m, case)
        errs = rel_inf(p, pred), rel_inf(d, dvec)
        print("fp32 %s: rel-inf pred %.3e d_vec %.3e" % ((case,) + errs))
        assert max(errs) < 1e-3, (case, errs)
    # the result does not depend on how many crops go through the conv and the mixer at a time
    whole = _run(m, "176")
    for n in (1, 2):
        m.metablock.crop_chunk = n
        part = _run(m, "176")
        assert rel_inf(part[1], whole[1]) < 1e-5 and rel_inf(part[0], whole[0]) < 1e-5, n


def _step(m, g, lefts=None):
    x = torch.from_numpy(g["x176"]).to(DEV).requires_grad_(True)
    pred, dvec = m(x, lefts=lefts)
    loss = (F.cosine_embedding_loss(dvec, torch.from_numpy(g["e176"]).to(DEV), torch.ones(2, device=DEV))
            + F.cross_entropy(pred, torch.from_numpy(g["step_labels"]).to(DEV)))
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    return x, pred, dvec, loss


def test_fp32_training_step_matches_fixture():
    import autoformer_amd as A

    A.set_compute("fp32")
    g = golden()
    m = _model()
    with pytest.raises(ValueError):
        m(torch.from_numpy(g["x176"]).to(DEV), [176, 150])  # lens is an inference argument
    x, pred, dvec, loss = _step(m, g, [int(v) for v in g["lefts176"]])
    assert rel_inf(dvec.detach().cpu().numpy(), g["dvec176"]) < 1e-3
    print(f"fp32 step loss {loss.item():.7f} vs {float(g['step_loss']):.7f}")
    np.testing.assert_allclose(loss.item(), float(g["step_loss"]), rtol=1e-5)
    step = {k[5:]: g[k] for k in g.files if k.startswith("step_g")}
    bad = grad_mismatches(m, step, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
    assert not bad, bad

    class _DX:  # dx through the same check
        def named_parameters(self):
            return [("dx", x)]
    bad = grad_mismatches(_DX(), step, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
    assert not bad, bad
    # only output channel 87 of the mixer's last conv is consumed
    assert float(m.metablock.mlp[3].weight.grad[:87].abs().max()) == 0.0
    assert float(m.metablock.mlp[3].weight.grad[87].abs().max()) > 0.0


def test_seeded_draw_reproduces_the_fixture():
    import autoformer_amd as A

    A.set_compute("fp32")
    g = golden()
    m = _model()
    random.seed(7)
    with torch.no_grad():
        _, dvec = m(torch.from_numpy(g["x176"]).to(DEV))
    assert rel_inf(dvec.cpu().numpy(), g["dvec176"]) < 1e-3
    random.seed(9)
    with torch.no_grad():
        _, dvec = m(torch.from_numpy(x200()).to(DEV), [int(v) for v in g["lens200"]])
    assert rel_inf(dvec.cpu().numpy(), g["dvec200"]) < 1e-3


def test_bf16_forward_only_path_matches_fixture_and_training_composition():
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    A.set_compute("bf16")
    m = _model()
    assert K.lstm_infer_persistent(3, 768) and 3 <= m.max_infer_batch() <= 64
    for case, (_, _, _, pred, dvec) in _cases().items():
        dp, dd = _d_emu(case)
        checks0 = K.ordering_stats()["checks"]
        m.metablock.infer_path = True
        p, d = _run(m, case)
        assert K.ordering_stats()["checks"] == checks0 + 1  # the forward-only recurrence ran
        m.metablock.infer_path = False
        pt, dt = _run(m, case)
        K.check_faults()
        errs = rel_inf(p, pred), rel_inf(d, dvec)
        print("bf16 %s: forward-only rel-inf pred %.3e d_vec %.3e; d_emu pred %.3e d_vec %.3e; "
              "training composition rel-inf d_vec %.3e; between the paths %.3e"
              % ((case,) + errs + (dp, dd, rel_inf(dt, dvec), rel_inf(d, dt))))
        assert errs[0] < 2 * dp and errs[1] < 2 * dd, (case, errs, dp, dd)
        assert rel_inf(p, pt) < 2 * dp and rel_inf(d, dt) < 2 * dd, case  # path equivalence, the same bar
        np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, rtol=1e-5)


def test_bf16_training_step():
    """Gradient norms within the project's bf16 bar (5e-2, what the LstmDV bf16 step
    uses) of the fp32 fixture; every parameter and x receive a finite gradient."""
    import autoformer_amd as A

    A.set_compute("bf16")
    g = golden()
    m = _model()
    x, pred, dvec, loss = _step(m, g, [int(v) for v in g["lefts176"]])
    err = rel_inf(dvec.detach().cpu().numpy(), g["dvec176"])
    print(f"bf16 training form 176: d_vec rel-inf {err:.3e}, loss {loss.item():.6f} vs {float(g['step_loss']):.6f}")
    assert err < 5e-2, err
    worst = ("", 0.0)
    for name, p in list(m.named_parameters()) + [("dx", x)]:
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        ref_n = float(g["step_gnorm/" + name])
        rel = abs(p.grad.norm().item() - ref_n) / ref_n
        worst = max(worst, (name, rel), key=lambda v: v[1])
        assert rel < 5e-2, (name, rel)
    print(f"bf16 training step: worst gradient-norm error {worst[1]:.3e} ({worst[0]})")
    assert float(m.metablock.mlp[3].weight.grad[:87].abs().max()) == 0.0


def test_embed_utterances_with_metadv():
    import autoformer_amd as A
    from autoformer_amd.detinit import det_inputs
    from autoformer_amd.embed import embed_utterances

    A.set_compute("bf16")
    m = _model()
    lengths = [230, 130, 176, 200, 150]
    mels = [det_inputs(1, n, seed=300 + i)[0][0] for i, n in enumerate(lengths)]
    rng = random.Random(5)
    lefts = [[rng.randint(0, max(n, 176) - 128) for _ in range(4)] for n in lengths]
    alone = []
    with torch.no_grad():
        for mel, lf in zip(mels, lefts):  # one at a time, short ones zero-padded to len_crop
            x = np.zeros((max(len(mel), 176), 80), np.float32)
            x[:len(mel)] = mel
            alone.append(m(torch.from_numpy(x[None]).to(DEV), lefts=lf)[1].cpu().numpy()[0])
    alone = np.stack(alone)
    bar = 2 * _d_emu("176")[1]
    for cap in (None, 2):
        got = embed_utterances(m, mels, len_crop=176, max_batch=cap, lefts=lefts)
        err = rel_inf(got, alone)
        print(f"embed_utterances(MetaDV) max_batch={cap}: rel-inf vs one at a time {err:.3e} (bar {bar:.3e})")
        assert got.shape == (5, 256) and err < bar, (cap, err, bar)
    drawn = embed_utterances(m, mels[:2], len_crop=176)  # windows drawn by the module
    assert drawn.shape == (2, 256) and np.isfinite(drawn).all()
    with pytest.raises(ValueError, match="crop_len"):
        embed_utterances(m, mels, len_crop=64)


def test_converter_takes_a_metadv_embedder():
    import autoformer_amd as A
    from autoformer_amd.convert import Converter
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.embed import speaker_dvector
    from autoformer_amd.factory.AutoVC import AutoVC

    A.set_compute("bf16")
    T, freq = 128, 16
    vc = AutoVC(44, 256, 512, freq)
    det_init_(vc)
    dv = _model()
    conv = Converter(vc.to(DEV).train(), T, embedder=dv)
    src = det_inputs(1, T - 10, seed=31)[0][0]
    mels = [det_inputs(1, 128, seed=40 + i)[0][0] for i in range(2)]  # T = crop_len: every window starts at 0
    got = conv.convert_between(src, mels[:1], mels[1:])
    want = conv.convert(src, speaker_dvector(dv, mels[:1], T), speaker_dvector(dv, mels[1:], T))
    assert got.shape == (T - 10, 80) and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
def test_mlp_mixer_patch32_padded_patches(comp):
    """The mixer at patch 32 with a patch count that is zero-padded (image 96 -> 9 patches, padded to
    16), a shape no model exercised before MetaDV (patch 32, 576 patches), against plain torch."""
    import autoformer_amd as A
    from autoformer_amd import metaformer as MF
    from autoformer_amd.factory.MLPMixer import MLPMixer

    A.set_compute(comp)
    torch.manual_seed(0)
    B, L, ps, out = 2, 96, 32, 88
    mix = MLPMixer(image_size=L, channels=1, patch_size=ps, kernel_size=3, padding=1, dim=L, depth=1, out_dim=out)
    sd = {MT.PRE + "mlp." + k: v.detach().clone().requires_grad_(True) for k, v in mix.state_dict().items()}
    mix = mix.to(DEV)
    g = torch.Generator().manual_seed(12)
    x, dy = torch.randn(B * L, L, generator=g), torch.randn(B * L, out, generator=g)
    xd = x.to(DEV).requires_grad_()
    y = MF.mlp_mixer(xd, mix, B, L)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_()
    yr = MT.mixer(sd, xr.view(B, L, L).transpose(1, 2), ps).transpose(1, 2).reshape(B * L, out)
    yr.backward(dy)

    def rel(a, b):
        return ((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()

    bars = (1e-4, 1e-4, 1e-4) if comp == "fp32" else (2e-2, 3e-2, 5e-2)  # test_mlp_mixer_general_dim's
    errs = {"y": rel(y.detach(), yr.detach()), "dx": rel(xd.grad, xr.grad)}
    assert errs["y"] < bars[0] and errs["dx"] < bars[1], errs
    for n, p in mix.named_parameters():
        e = rel(p.grad, sd[MT.PRE + "mlp." + n].grad)
        assert e < bars[2], (n, e)
