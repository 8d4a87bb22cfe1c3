"""The LSTM recurrences that avc_lstm_fwd / avc_lstm_bwd dispatch to outside the benchmark's shapes,
each called directly through kernels.lstm_fwd / kernels.lstm_bwd and compared with a float64 loop
(tests/helpers.py ref_fwd / ref_bwd) on the same inputs.

1. The bf16 per-step kernels of csrc/lstm.hip (one launch per time step), taken in bf16 compute when
   the layer is bidirectional at H > 64, when H is not 512 / 768 / 1024, or when the persistent grid
   ceil(B/8) * H/32 exceeds the CU count.  The reference keeps the kernels' rounding points: bf16
   weights, and h_{t-1} (forward) / the previous backward step's dG (backward) rounded to bf16 before
   the recurrent product; everything else float64.  Bar: 2e-3 in rel-Frobenius and in max-abs error
   over max-abs reference, the bar of the persistent kernels against the same kind of reference
   (test_gpu_kernels.py test_lstm_persistent_forward_matches_per_step / _persistent_backward_case).
   Every case first asserts that the persistent path is NOT taken.

2. The default small-H kernels lstm_small_fwd / lstm_small_bwd (csrc/lstm_small.hip, the production
   encoder BiLSTM; the MFMA form stays off) over their branch lattice: both edges of every register
   bucket HM in {16, 32, 48, 64}, H % 4 in {0, 1, 2, 3} (vector / scalar flush), T below / at the
   4-step input ring, one below / at / one above the 16-step output chunk and a ragged multi-chunk T,
   both directions, FAST activations off (fp32 compute) and on (bf16 compute).  Weights and state are
   fp32 in both modes, so the reference is the unrounded float64 recurrence; the backward reference
   runs from the GPU forward's own c / gates.

   Bars (rel-Frobenius and max-abs error over max-abs reference, per output h, c, gates, dG):
     fp32 compute: 1e-4, the project's bar for fp32 recurrences.
     bf16 compute (v_exp_f32 / v_rcp_f32 activations): 4x the worst error measured over the whole
     lattice on the MI355X, rounded up to one significant digit, capped at 1e-2:
       worst rel-Frobenius  1.98e-7 (h at H = 17, T = 17, dirs = 2)  -> bar 8e-7
       worst max-abs ratio  4.07e-7 (h at H = 33, T = 17, dirs = 1)  -> bar 2e-6
     (the fp32-compute worsts over the same lattice: 9.0e-8 and 1.6e-7)."""
import functools

import pytest
import torch

from .helpers import ref_bwd, ref_fwd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

STEP_BAR = 2e-3
FP32_BAR = 1e-4
# measured on the MI355X over SMALL_CASES in bf16 compute (worst output of the worst case), and the
# bars derived from them: 4x, rounded up to one significant digit
FAST_WORST_RELF, FAST_BAR_RELF = 1.98e-7, 8e-7
FAST_WORST_RINF, FAST_BAR_RINF = 4.07e-7, 2e-6


@pytest.fixture(autouse=True)
def _restore_fp32():
    import autoformer_amd as A

    yield
    A.set_compute("fp32")


def relf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def rinf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def _errors(got, ref):
    """{name: (rel-Frobenius, max-abs ratio)}; the reference (B, T, .) against the kernels' (B*T, .)."""
    return {k: (relf(got[k], ref[k].reshape(got[k].shape)), rinf(got[k], ref[k].reshape(got[k].shape))) for k in got}


def _misses(errs, bar_f, bar_i):
    return {k: v for k, v in errs.items() if not (v[0] < bar_f and v[1] < bar_i)}


# ------------------------------------------------------------------ 1. bf16 per-step recurrences
# (B, T, H, dirs): forward kernel, backward kernel.  T >= 3: step 0, both ping-pong parities and the
# s > 0 recurrent product all run.
STEP_CASES = {
    (3, 6, 512, 2): ("lstm_step_fwd_bf<512,1>", "lstm_step_bwd_bf<512>"),
    (5, 5, 1024, 2): ("lstm_step_fwd_bf<1024,1>", "lstm_step_bwd_bf<1024>"),
    # B > 16 at H = 1024 takes the 32-row tile: rows 20..31 are masked
    (20, 5, 1024, 2): ("lstm_step_fwd_bf<1024,2>", "lstm_step_bwd_bf<1024>"),
    # 9 groups x 32 = 288 workgroups: residency refuses the persistent path (AutoVC at batch 72)
    (72, 4, 1024, 1): ("lstm_step_fwd_bf<1024,2>", "lstm_step_bwd_bf<1024>"),
    # 18 groups x 16 = 288 workgroups; a tail of 9 rows in the last 16-row tile
    (137, 3, 512, 1): ("lstm_step_fwd_bf<512,1>", "lstm_step_bwd_bf<512>"),
    (3, 7, 128, 2): ("lstm_step_fwd<true,1>", "lstm_step_bwd<true,1>"),
    # a second 16-row tile with 2 live rows
    (18, 5, 256, 1): ("lstm_step_fwd<true,1>", "lstm_step_bwd<true,1>"),
    (20, 4, 1152, 1): ("lstm_step_fwd<true,2>", "lstm_step_bwd<true,1>"),
}
_STEP_IDS = [f"B{b}-T{t}-H{h}-d{d}" for (b, t, h, d) in STEP_CASES]


def _step_setup(B, T, H, dirs):
    """bf16 compute, and the proof that this shape is on the per-step path in both passes."""
    import autoformer_amd as A
    from autoformer_amd import kernels as Kr

    A.set_compute("bf16")
    assert not Kr.lstm_persistent_fwd(B, H, dirs)
    assert not Kr.lstm_persistent_bwd(B, H, dirs)
    return Kr


def _step_weights(gen, H, dirs):
    """W_hh stacked as LSTMLayerCore.packs does: [dirs*4H][H] for the forward, per-direction transposes
    [dirs*H][4H] for the backward; bf16."""
    G = 4 * H
    whh = (torch.randn(dirs * G, H, generator=gen) * (1.0 / H ** 0.5)).bfloat16()
    whh_t = torch.cat([whh[d * G:(d + 1) * G].t() for d in range(dirs)], 0).contiguous()
    return whh, whh_t


@pytest.mark.parametrize("B,T,H,dirs", list(STEP_CASES), ids=_STEP_IDS)
def test_lstm_per_step_forward_bf16(B, T, H, dirs):
    """avc_lstm_fwd's bf16 per-step kernels -- lstm_step_fwd_bf<1024|512, 1|2> and the generic
    lstm_step_fwd<true, 1|2>, the instantiation of each shape named in STEP_CASES -- against the float64
    recurrence with bf16 weights and bf16-rounded h_{t-1}: h, c and the activated gates."""
    Kr = _step_setup(B, T, H, dirs)
    gen = torch.Generator().manual_seed(1000 * B + 10 * T + H + dirs)
    G = 4 * H
    xp = torch.randn(B, T, dirs * G, generator=gen) * 0.5
    whh, _ = _step_weights(gen, H, dirs)
    hbuf = Kr.lstm_scratch(B, H, dirs, DEV)
    h, c, g = Kr.lstm_fwd(xp.reshape(B * T, -1).to(DEV), whh.to(DEV), B, T, H, dirs, hbuf)
    torch.cuda.synchronize()
    hr, cr, gr = ref_fwd(xp.double(), whh.double(), B, T, H, dirs, round_rec=True)
    errs = _errors({"h": h, "c": c, "gates": g}, {"h": hr, "c": cr, "gates": gr})
    print(STEP_CASES[(B, T, H, dirs)][0], errs)
    assert not _misses(errs, STEP_BAR, STEP_BAR), errs


@pytest.mark.parametrize("B,T,H,dirs", list(STEP_CASES), ids=_STEP_IDS)
def test_lstm_per_step_backward_bf16(B, T, H, dirs):
    """avc_lstm_bwd's bf16 per-step kernels -- lstm_step_bwd_bf<1024|512> and the generic
    lstm_step_bwd<true, 1>, the instantiation of each shape named in STEP_CASES -- from synthetic c and
    gates, against the float64 backward with bf16 weights and the previous step's dG rounded to bf16: dG."""
    Kr = _step_setup(B, T, H, dirs)
    gen = torch.Generator().manual_seed(2000 * B + 10 * T + H + dirs)
    G = 4 * H
    dh = torch.randn(B, T, dirs * H, generator=gen) * 0.1
    c = torch.randn(B, T, dirs * H, generator=gen) * 0.7
    gates = torch.rand(B, T, dirs, 4, H, generator=gen) * 0.9 + 0.05
    gates[:, :, :, 2] = gates[:, :, :, 2] * 2 - 1  # g gate in (-1, 1)
    gates = gates.reshape(B, T, dirs * G)
    whh, whh_t = _step_weights(gen, H, dirs)
    gbuf = Kr.lstm_bwd_scratch(B, H, dirs, DEV)
    dhd = dh.reshape(B * T, -1).to(DEV)
    dg = Kr.lstm_bwd(dhd, dhd, c.reshape(B * T, -1).to(DEV), gates.reshape(B * T, -1).to(DEV), None, whh_t.to(DEV),
                     B, T, H, dirs, gbuf=gbuf)
    torch.cuda.synchronize()
    dgr = ref_bwd(dh.double(), c.double(), gates.double(), whh.double(), B, T, H, dirs, round_rec=True)
    errs = _errors({"dG": dg}, {"dG": dgr})
    print(STEP_CASES[(B, T, H, dirs)][1], errs)
    assert not _misses(errs, STEP_BAR, STEP_BAR), errs


# ------------------------------------------------------------------ 2. default small-H kernels
SMALL_B = 3
SMALL_CASES = sorted({(H, 17, 2) for H in (3, 10, 16, 17, 32, 33, 44, 48, 49, 64)}
                     | {(H, T, 2) for H in (44, 33) for T in (1, 3, 4, 15, 16, 17, 33)}
                     | {(33, 17, 1)})


@functools.lru_cache(maxsize=None)
def _small_inputs(H, T, dirs):
    """Inputs and the float64 forward of a lattice point, shared by both compute modes; read-only."""
    B, G = SMALL_B, 4 * H
    gen = torch.Generator().manual_seed(10000 * dirs + 100 * T + H)
    xp = torch.randn(B, T, dirs * G, generator=gen) * 0.8
    w = (torch.rand(dirs * G, H, generator=gen) * 2 - 1) / H ** 0.5
    dh = torch.randn(B, T, dirs * H, generator=gen)
    return xp, w, dh, ref_fwd(xp.double(), w.double(), B, T, H, dirs)


def _small_run(H, T, dirs, comp):
    """The GPU outputs of a lattice point: {"h", "c", "gates", "dG"}, each (B*T, .) with its bf16 twin."""
    import autoformer_amd as A
    from autoformer_amd import _lib as L
    from autoformer_amd import kernels as K

    A.set_compute(comp)
    assert L.lib().avc_lstm_small_mfma(H, K.BF16) == 0  # the default packed-FMA kernels
    B = SMALL_B
    xp, w, dh, _ = _small_inputs(H, T, dirs)
    wd = w.to(DEV)
    h, c, g = K.lstm_fwd(xp.reshape(B * T, -1).to(DEV), wd, B, T, H, dirs)
    dg = K.lstm_bwd(dh.reshape(B * T, -1).to(DEV), h, c, g, wd, None, B, T, H, dirs)
    torch.cuda.synchronize()
    return {"h": h, "c": c, "gates": g, "dG": dg}


def _small_errors(H, T, dirs, comp):
    B = SMALL_B
    _, w, dh, (hr, cr, gr) = _small_inputs(H, T, dirs)
    got = _small_run(H, T, dirs, comp)
    # the reference backward runs from the GPU forward's own c / gates (isolates the backward)
    dgr = ref_bwd(dh.double(), got["c"].cpu().double().reshape(B, T, -1), got["gates"].cpu().double().reshape(B, T, -1),
                  w.double(), B, T, H, dirs)
    return got, _errors(got, {"h": hr, "c": cr, "gates": gr, "dG": dgr})


def _small_bars(comp):
    return (FP32_BAR, FP32_BAR) if comp == "fp32" else (FAST_BAR_RELF, FAST_BAR_RINF)


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
@pytest.mark.parametrize("H,T,dirs", SMALL_CASES)
def test_lstm_small_matches_fp64(H, T, dirs, comp):
    """lstm_small_fwd / lstm_small_bwd<HM, FAST> at one point of their branch lattice against float64."""
    got, errs = _small_errors(H, T, dirs, comp)
    print(comp, (H, T, dirs), errs)
    bar_f, bar_i = _small_bars(comp)
    assert bar_f <= 1e-2 and bar_i <= 1e-2
    assert not _misses(errs, bar_f, bar_i), errs
    if comp == "bf16":
        assert torch.equal(got["h"]._bf16, got["h"].bfloat16()), "bf16 twin of h"
        assert torch.equal(got["dG"]._bf16, got["dG"].bfloat16()), "bf16 twin of dG"


def _wrong_fwd(xp, w, B, T, H, dirs):
    """ref_fwd with direction 1 run in forward time order."""
    G = 4 * H
    parts = [ref_fwd(xp[:, :, d * G:(d + 1) * G], w[d * G:(d + 1) * G], B, T, H, 1) for d in range(dirs)]
    return [torch.cat([p[k] for p in parts], 2) for k in range(3)]


def _wrong_bwd(dh, c, g, w, B, T, H, dirs):
    """ref_bwd without the zeroing of c_prev at the forward's first step: it takes the clamped
    neighbour that the kernel's input ring has loaded there, c of that step itself."""
    first = torch.cat([c[:, T - 1 if d else 0, d * H:(d + 1) * H] for d in range(dirs)], 1)
    return ref_bwd(dh, c, g, w, B, T, H, dirs, c0=first)


@pytest.mark.parametrize("comp", ["fp32", "bf16"])
def test_lstm_small_bars_discriminate(comp):
    """The bars separate a one-step indexing error from rounding: the same GPU outputs (H = 33, T = 17,
    both directions) miss them by at least 10x against a reference that runs direction 1 in forward time
    order (h, c, gates) and against one that does not zero c_prev at the first step (dG)."""
    H, T, dirs, B = 33, 17, 2, SMALL_B
    xp, w, dh, _ = _small_inputs(H, T, dirs)
    got, errs = _small_errors(H, T, dirs, comp)
    bar_f, bar_i = _small_bars(comp)
    assert not _misses(errs, bar_f, bar_i), errs
    hw, cw, gw = _wrong_fwd(xp.double(), w.double(), B, T, H, dirs)
    wrong = _errors({k: got[k] for k in ("h", "c", "gates")}, {"h": hw, "c": cw, "gates": gw})
    dgw = _wrong_bwd(dh.double(), got["c"].cpu().double().reshape(B, T, -1),
                     got["gates"].cpu().double().reshape(B, T, -1), w.double(), B, T, H, dirs)
    wrong.update(_errors({"dG": got["dG"]}, {"dG": dgw}))
    print(comp, wrong)
    for k, (ef, ei) in wrong.items():
        assert ef >= 10 * bar_f and ei >= 10 * bar_i, (k, ef, ei)
