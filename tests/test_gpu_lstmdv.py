"""The LstmDV speaker embedder on the device against the reference fixture (tests/golden/lstmdv.npz):
the training composition in fp32 parity mode (embeddings, per-length capture, one training step's
gradients), the forward-only bf16 inference path, and the user interface built on it
(embed_utterances, Converter.convert_between).

The bf16 bar is not a constant: it is 2 x d_emu, where d_emu is the rel-inf distance from the same
fixture of a CPU emulation of the bf16 rounding points (tests/test_lstmdv.py::emulate_bf16: bf16
weights, input and inter-layer h, h_{t-1} rounded before the recurrent product, fp32 head), computed
when the test runs.  The factor 2 covers what the emulation leaves out -- the v_exp / v_rcp forms of
the activations and the GEMMs' accumulation order.  On the fixture a wrong row or a wrong capture
step moves an embedding by more than 0.1 of its largest entry (test_lstmdv.py asserts it), far
outside the bar."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .helpers import grad_mismatches, rel_inf
from .test_lstmdv import emulate_bf16, golden, ref_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def _model():
    import factory.LstmDV as M
    from autoformer_amd.detinit import det_init_

    m = M.LstmDV()
    det_init_(m)
    return m.to(DEV).train()


@functools.lru_cache(maxsize=None)
def _ref_state():
    return {k: v.detach() for k, v in ref_model().state_dict().items()}


@functools.lru_cache(maxsize=None)
def _d_emu(case):
    """rel-inf drift of the bf16 emulation from the fixture: 'full24', 'lens24' or '176'."""
    g = golden()
    sd = _ref_state()
    if case == "176":
        return rel_inf(emulate_bf16(sd, torch.from_numpy(g["x176"])).numpy(), g["emb176"])
    lens = [int(v) for v in g["lens24"]] if case == "lens24" else None
    return rel_inf(emulate_bf16(sd, torch.from_numpy(g["x24"]), lens).numpy(),
                   g["emb24_lens" if case == "lens24" else "emb24_full"])


def test_fp32_embeddings_match_fixture():
    import autoformer_amd as A

    A.set_compute("fp32")
    g = golden()
    m = _model()
    x24 = torch.from_numpy(g["x24"]).to(DEV)
    with torch.no_grad():
        full = m(x24).cpu().numpy()
        part = m(x24, [int(v) for v in g["lens24"]]).cpu().numpy()
        e176 = m(torch.from_numpy(g["x176"]).to(DEV)).cpu().numpy()
    errs = rel_inf(full, g["emb24_full"]), rel_inf(part, g["emb24_lens"]), rel_inf(e176, g["emb176"])
    print("fp32 rel-inf full24 %.3e lens24 %.3e 176 %.3e" % errs)
    assert max(errs) < 1e-3, errs


def test_fp32_training_step_matches_fixture():
    import autoformer_amd as A

    A.set_compute("fp32")
    g = golden()
    m = _model()
    x = torch.from_numpy(g["x176"]).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError):
        m(x, [176, 100])  # lens is an inference argument
    emb = m(x)
    loss = F.cosine_embedding_loss(emb, torch.from_numpy(g["e176"]).to(DEV), torch.ones(2, device=DEV))
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    assert rel_inf(emb.detach().cpu().numpy(), g["emb176"]) < 1e-3
    np.testing.assert_allclose(loss.item(), float(g["step_loss"]), rtol=1e-4)
    step = {k[5:]: g[k] for k in g.files if k.startswith("step_g")}
    bad = grad_mismatches(m, step, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
    assert not bad, bad

    class _DX:  # dx through the same check
        def named_parameters(self):
            return [("dx", x)]
    bad = grad_mismatches(_DX(), step, tol=1e-2, head_tol=1e-2, bn_fed_bias=lambda n: False)
    assert not bad, bad


def test_bf16_training_step_takes_the_80_wide_input():
    """bf16 compute sends the layer-0 products (xproj K = 80, dW_ih N = 80, dx N = 80) to the bf16
    GEMM kernels, whose K blocks are 32 wide: the step's embedding (rel-inf) and every gradient norm
    are held to the project's bf16 bar (5e-2) against the fp32 fixture."""
    import autoformer_amd as A

    A.set_compute("bf16")
    g = golden()
    m = _model()
    x = torch.from_numpy(g["x176"]).to(DEV).requires_grad_(True)
    emb = m(x)
    loss = F.cosine_embedding_loss(emb, torch.from_numpy(g["e176"]).to(DEV), torch.ones(2, device=DEV))
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    err = rel_inf(emb.detach().cpu().numpy(), g["emb176"])
    print(f"bf16 training form 176: rel-inf {err:.3e}")
    assert err < 5e-2, err
    worst = ("", 0.0)
    for name, p in list(m.named_parameters()) + [("dx", x)]:
        ref_n = float(g["step_gnorm/" + name])
        rel = abs(p.grad.norm().item() - ref_n) / ref_n
        worst = max(worst, (name, rel), key=lambda v: v[1])
        assert torch.isfinite(p.grad).all() and rel < 5e-2, (name, rel)
    print(f"bf16 training step: worst gradient-norm error {worst[1]:.3e} ({worst[0]})")


@pytest.mark.parametrize("rows", [0, 8, 16])
def test_bf16_inference_matches_fixture(rows):
    import autoformer_amd as A
    from autoformer_amd import kernels as K

    A.set_compute("bf16")
    g = golden()
    m = _model()
    m.infer_rows = rows
    assert K.lstm_infer_persistent(3, 768, rows) and m.max_infer_batch() >= 64
    x24 = torch.from_numpy(g["x24"]).to(DEV)
    checks0 = K.ordering_stats()["checks"]
    with torch.no_grad():
        full = m(x24).cpu().numpy()
        part = m(x24, [int(v) for v in g["lens24"]]).cpu().numpy()
        e176 = m(torch.from_numpy(g["x176"]).to(DEV)).cpu().numpy()
    K.check_faults()
    assert K.ordering_stats()["checks"] == checks0 + 9  # three forward-only recurrences per call
    for name, got, ref, case in (("full24", full, g["emb24_full"], "full24"), ("lens24", part, g["emb24_lens"], "lens24"),
                                 ("176", e176, g["emb176"], "176")):
        err, d = rel_inf(got, ref), _d_emu(case)
        print(f"bf16 rows={rows} {name}: rel-inf {err:.3e}, d_emu {d:.3e}")
        assert err < 2 * d, (name, err, d)
    np.testing.assert_allclose(np.linalg.norm(full, axis=1), 1.0, rtol=1e-5)


def _five_mels():
    from autoformer_amd.detinit import det_inputs

    lengths = [3, 176, 176, 200, 41]
    return [det_inputs(1, n, seed=300 + i)[0][0] for i, n in enumerate(lengths)]


def test_embed_utterances_equals_one_at_a_time():
    import autoformer_amd as A
    from autoformer_amd.embed import embed_utterances

    A.set_compute("bf16")
    m = _model()
    mels = _five_mels()
    alone = []
    with torch.no_grad():
        for mel in mels:  # the reference's way: B = 1, short ones zero-padded to len_crop
            x = np.zeros((max(len(mel), 176), 80), np.float32)
            x[:len(mel)] = mel
            alone.append(m(torch.from_numpy(x[None]).to(DEV)).cpu().numpy()[0])
    alone = np.stack(alone)
    bar = 2 * _d_emu("176")
    for cap in (None, 2):
        got = embed_utterances(m, mels, len_crop=176, max_batch=cap)
        err = rel_inf(got, alone)
        print(f"embed_utterances max_batch={cap}: rel-inf vs one at a time {err:.3e} (bar {bar:.3e})")
        assert got.shape == (5, 256) and err < bar, (cap, err, bar)


def test_convert_between_equals_convert_with_dvectors():
    import autoformer_amd as A
    from autoformer_amd.convert import Converter
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.embed import speaker_dvector
    from autoformer_amd.factory.AutoVC import AutoVC

    A.set_compute("bf16")
    T, freq = 64, 16
    vc = AutoVC(44, 256, 512, freq)
    det_init_(vc)
    dv = _model()
    conv = Converter(vc.to(DEV).train(), T, embedder=dv)
    src = det_inputs(1, T - 10, seed=31)[0][0]
    src_mels = [det_inputs(1, n, seed=40 + i)[0][0] for i, n in enumerate((30, 64, 70))]
    trg_mels = [det_inputs(1, n, seed=50 + i)[0][0] for i, n in enumerate((64, 12))]
    got = conv.convert_between(src, src_mels, trg_mels)
    e_org, e_trg = speaker_dvector(dv, src_mels, T), speaker_dvector(dv, trg_mels, T)
    assert e_org.shape == (256,) and np.linalg.norm(e_org) < 1.0 + 1e-5  # a mean of unit vectors
    want = conv.convert(src, e_org, e_trg)
    assert got.shape == (T - 10, 80) and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
