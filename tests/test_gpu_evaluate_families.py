"""convert_grid(..., batch_families=True) on the GPU for the families the default leaves pair by pair
(autoformer_amd/evaluate.py): MetaConv / MetaPool and the AdaIN variants under per-utterance BatchNorm and
per-segment AdaIN, against the CPU oracles run at B = 1 per pair as the reference converts (train mode).

Set-ups, closed-form weights (det_init_), fp32 compute unless a test says bf16:
  Meta    (44, 256, 512, 22), len_crop 176, two sources (one 16 frames short), four pairs
  AutoVC2 (44, 256, 512, 16), len_crop 64, three sources (one 10 frames short), nine pairs, isAdain
  MetaConv2 (44, 256, 512, 22), len_crop 176, two sources, four pairs, isAdain
The bar of every parity check is rel-inf < 1e-3 per pair, the one tests/test_gpu_evaluate.py and
tests/test_convert.py hold the conversion to.  On these inputs the CPU oracle run as ONE batch (batch-wide
statistics and moments) sits 0.30 .. 0.43 (MetaConv, MetaPool, MetaConv2) and 1.2 .. 1.5 (AutoVC2) rel-inf
from its own B = 1 result, so the bar separates the two functions by two orders of magnitude and more."""
import functools
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SETUP = {   # name: (len_crop, freq, sources, frames the second source is short, det_inputs seed)
    "MetaConv": (176, 22, 2, 16, 35), "MetaPool": (176, 22, 2, 16, 35),
    "AutoVC2": (64, 16, 3, 10, 31), "MetaConv2": (176, 22, 2, 16, 37),
    "AutoVC_Adjust": (64, 16, 2, 10, 39),
}
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


@pytest.fixture(autouse=True)
def _restore_compute():
    import autoformer_amd as A

    yield
    A.set_compute("bf16")


def rel_inf(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _sources(name, extra=0):
    """The family's sources and embeddings; extra > 0: every source but the short one is that much longer
    than len_crop (so the grid draws crop offsets)."""
    from autoformer_amd.detinit import det_inputs

    T, _, n, short, seed = SETUP[name]
    x, e = det_inputs(n, T + extra, seed=seed)
    return [x[i][:T - short] if i == 1 else x[i][:T + (extra if i == 0 else extra // 2)] for i in range(n)], e


def _padded(name):
    T = SETUP[name][0]
    srcs, e = _sources(name)
    x = np.zeros((len(srcs), T, 80), np.float32)
    for s, m in enumerate(srcs):
        x[s, :m.shape[0]] = m
    return x, e


def _model(name, comp="fp32", train=True):
    import autoformer_amd as A
    from autoformer_amd.detinit import det_init_

    A.set_compute(comp)
    cls = getattr(importlib.import_module(f"autoformer_amd.factory.{name}"), name)
    m = cls(44, 256, 512, SETUP[name][1])
    det_init_(m)
    m = m.to(DEV)
    return m.train() if train else m.eval()


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    """mel_postnet (len_crop, 80) of every pair, source-major, from the CPU oracle at B = 1 in train mode on
    the padded source, called as the reference calls the model (util/evaluate.py:80-84: for AdaIN once with
    c_trg = None for the features of the source, once with them as target_feature).  Computed once per
    family, never modified."""
    from oracle import autovc_cpu as O
    from oracle import metaformer_cpu as M
    from oracle import variants_cpu as V

    T, freq, n, _, _ = SETUP[name]
    x, e = _padded(name)
    out = []
    with torch.no_grad():
        if name in ("MetaConv", "MetaPool"):
            spec, fwd = ((M.metaconv_spec, M.metaconv_forward) if name == "MetaConv"
                         else (M.metapool_spec, M.metapool_forward))
            sd = O.make_state(spec())

            def one(xs, es, et):
                return fwd(sd, xs, es, et, freq=freq, training=True)[1]
        else:
            sd = O.make_state(V.SPECS[name]())

            def one(xs, es, et):
                _, feats = V.adain_forward(name, sd, xs, es, None, freq=freq, training=True)
                return V.adain_forward(name, sd, xs, es, et, target_feature=feats, freq=freq, training=True)[1]
        for s in range(n):
            for t in range(n):
                o = one(torch.from_numpy(x[s:s + 1]), torch.from_numpy(e[s:s + 1]), torch.from_numpy(e[t:t + 1]))
                a = o.squeeze(1)[0].numpy().copy()
                a.setflags(write=False)
                out.append(a)
    return tuple(out)


def _grid(m, name, **kw):
    from autoformer_amd.evaluate import convert_grid

    T, _, n, short, _ = SETUP[name]
    srcs, e = _sources(name)
    kw.setdefault("batch_families", True)
    mels, pads = convert_grid(m, srcs, e, len_crop=T, isAdain=name.endswith("2"), **kw)
    assert len(mels) == n * n and pads == [0] * n + [short] * n + [0] * n * (n - 2)
    assert all(a.shape == (T, 80) and a.dtype == np.float32 for a in mels)
    return mels


def _bn_state(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k.rsplit(".", 1)[-1] in BN_BUFFERS}


def _against_oracle(mels, name):
    ref = oracle_grid(name)
    rels = [rel_inf(a, r) for a, r in zip(mels, ref)]
    print(f"{name} fp32 batched grid vs oracle, rel-inf per pair:", " ".join(f"{r:.2e}" for r in rels))
    return rels


def _plain_batched(m, name):
    """The same rows through a plain batched forward, no context: batch-wide statistics (and moments)."""
    x, e = _padded(name)
    with torch.no_grad():
        xd, ed = torch.from_numpy(x).to(DEV), torch.from_numpy(e).to(DEV)
        return m(xd, ed, ed)[1].squeeze(1).cpu().numpy()


# ----------------------------------------------------------------------- parity, fp32, train mode
@pytest.mark.parametrize("name", ["MetaConv", "MetaPool", "AutoVC2", "MetaConv2"])
def test_batched_grid_matches_the_oracle_and_leaves_the_model(name):
    """Every pair of the batched train-mode grid equals the oracle's B = 1 train-mode conversion, rel-inf
    < 1e-3; every BatchNorm buffer is bit-identical before and after and the model is still in train mode."""
    from autoformer_amd.evaluate import grid_family

    m = _model(name)
    assert grid_family(m, False, name.endswith("2")) == ("adain" if name.endswith("2") else "meta")
    before = _bn_state(m)
    assert before and len(before) % 3 == 0
    rels = _against_oracle(_grid(m, name), name)
    assert max(rels) < BAR, rels
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert m.training


@pytest.mark.parametrize("name", ["MetaConv", "AutoVC2"])
def test_what_the_bar_excludes(name):
    """A plain batched forward of the same rows (statistics over the whole batch) misses the bar."""
    n = SETUP[name][2]
    plain = _plain_batched(_model(name), name)
    ref = oracle_grid(name)
    rels = [rel_inf(plain[s], ref[s * n + s]) for s in range(n)]
    print(f"{name} plain batched forward vs the B = 1 oracle:", " ".join(f"{r:.2e}" for r in rels))
    assert min(rels) > BAR, rels


@pytest.mark.parametrize("name", ["MetaConv", "AutoVC2"])
def test_chunking(name):
    """max_batch = 1, 4 and 64 (for AutoVC2's nine pairs: single rows; 4 + 4 + a ragged 1; one chunk) all
    meet the bar against the oracle and agree with each other within it."""
    m = _model(name)
    ref = oracle_grid(name)
    grids = [_grid(m, name, max_batch=k) for k in (1, 4, 64)]
    for g in grids:
        assert max(rel_inf(a, r) for a, r in zip(g, ref)) < BAR
    for g in grids[:2]:
        assert max(rel_inf(a, b) for a, b in zip(g, grids[2])) < BAR


@pytest.mark.parametrize("name", ["MetaConv", "AutoVC2"])
def test_same_draws_as_the_fallback(name):
    """Sources longer than len_crop: under the same numpy seed the batched call and the default (pair by
    pair) call draw the same plan -- the same pads, the same rng state afterwards, the result of a plan
    drawn beforehand under that seed bit for bit -- and their mels agree within the bar."""
    from autoformer_amd.evaluate import convert_grid, plan_grid

    T = SETUP[name][0]
    srcs, e = _sources(name, extra=40)
    assert max(s.shape[0] for s in srcs) > T > min(s.shape[0] for s in srcs)
    m = _model(name)
    kw = dict(len_crop=T, isAdain=name.endswith("2"), targets=srcs)
    np.random.seed(11)
    fast, pads_fast = convert_grid(m, srcs, e, batch_families=True, **kw)
    state_fast = np.random.get_state()
    np.random.seed(11)
    slow, pads_slow = convert_grid(m, srcs, e, **kw)
    state_slow = np.random.get_state()
    np.random.seed(11)
    lens = [s.shape[0] for s in srcs]
    plan = plan_grid(lens, None, T, np.random, tgt_lens=lens)[0]
    assert any(left > 0 for left, _ in plan.src_crop)
    assert pads_fast == pads_slow == plan.pads
    assert np.array_equal(state_fast[1], state_slow[1]) and state_fast[2] == state_slow[2]
    planned, _ = convert_grid(m, srcs, e, batch_families=True, plan=plan, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(fast, planned))
    rels = [rel_inf(a, b) for a, b in zip(fast, slow)]
    print(f"{name} batched vs pair by pair, same draws:", " ".join(f"{r:.2e}" for r in rels))
    assert max(rels) < BAR, rels


def test_eval_mode_autovc2_equals_one_at_a_time():
    """An eval-mode AutoVC2 with running statistics that are not the identity: BatchNorm is row-independent
    already, AdaIN is not (it has no running statistics), so the batch still needs the per-segment ops.
    The batched grid equals Converter.convert(..., isAdain=True) at the eval-mode tolerance of
    tests/test_gpu_evaluate.py, rtol = atol = 1e-5."""
    from autoformer_amd.convert import Converter

    name = "AutoVC2"
    T, _, n, _, _ = SETUP[name]
    m = _model(name, train=False)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.linspace(-0.5, 0.5, v.numel()))
            elif k.endswith("running_var"):
                v.copy_(torch.linspace(0.5, 2.0, v.numel()))
    mels = _grid(m, name)
    srcs, e = _sources(name)
    conv = Converter(m, T, DEV)
    for i, (s, t) in enumerate((s, t) for s in range(n) for t in range(n)):
        one = conv.convert(srcs[s], e[s], e[t], isAdain=True)
        assert one.shape == (srcs[s].shape[0], 80)
        torch.testing.assert_close(torch.from_numpy(mels[i][:one.shape[0]]), torch.from_numpy(one), rtol=1e-5, atol=1e-5)
    assert not m.training


def test_adjust_stays_on_the_fallback_and_the_default_is_the_loop(monkeypatch):
    """AutoVC_Adjust with batch_families=True still goes pair by pair: one Converter.get_trans_mel call per
    pair, the default call's result.  MetaConv with the default batch_families=False is bit-identical to
    the Converter loop."""
    from autoformer_amd.convert import Converter
    from autoformer_amd.evaluate import convert_grid, grid_family

    name = "AutoVC_Adjust"
    T = SETUP[name][0]
    srcs, e = _sources(name)
    m = _model(name)
    assert grid_family(m, True, False) is None and grid_family(m) is None
    calls, inner = [], Converter.get_trans_mel

    def counted(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)

    monkeypatch.setattr(Converter, "get_trans_mel", counted)
    kw = dict(len_crop=T, isAdjust=True, targets=srcs)
    a, pads_a = convert_grid(m, srcs, e, batch_families=True, **kw)
    assert len(calls) == len(a) == 4
    b, pads_b = convert_grid(m, srcs, e, **kw)
    assert len(calls) == 8 and pads_a == pads_b
    assert max(rel_inf(x, y) for x, y in zip(a, b)) < BAR
    monkeypatch.undo()

    name = "MetaConv"
    T = SETUP[name][0]
    srcs, e = _sources(name)
    m = _model(name)
    mels, pads = convert_grid(m, srcs, e, len_crop=T)
    conv = Converter(m, T, DEV)
    for i, (s, t) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        assert np.array_equal(mels[i], conv.convert(srcs[s], e[s], e[t], trim=False)), (s, t)


def test_meta_refuses_another_len_crop():
    """A Meta family with len_crop != 176 raises what MetaBlock.frames raises."""
    from autoformer_amd.evaluate import convert_grid

    srcs, e = _sources("MetaConv")
    with pytest.raises(RuntimeError, match="MetaBlock needs L == crop_len"):
        convert_grid(_model("MetaConv"), srcs, e, len_crop=88, batch_families=True)


# ----------------------------------------------------------------------- bf16
@pytest.mark.parametrize("name", ["MetaConv", "AutoVC2"])
def test_bf16_batched_grid_against_the_loop(name):
    """bf16 compute against the fp32 oracle: relative Frobenius and rel-inf per pair, for the batched grid
    and for the B = 1 Converter loop (the parent path, not the code under test) on the same inputs.
    tests/test_gpu_model.py and tests/test_variants.py hold no bf16 mel_postnet bar for these families, so
    the bar is 2 x the loop's own distance (its worst pair, per figure): the batched path differs from the
    loop only in keeping the conv output in fp32 before the statistics, so it should sit at or below it.
    Measured on the MI355X, worst pair, relative Frobenius / rel-inf (per pair: DESIGN section 7):
      MetaConv  batched 2.46e-2 / 2.92e-2 (four pairs),  B = 1 loop 2.77e-2 / 3.12e-2
      AutoVC2   batched 5.10e-2 / 5.82e-2 (nine pairs),  B = 1 loop 5.92e-2 / 6.45e-2"""
    from autoformer_amd.convert import Converter

    T, _, n, _, _ = SETUP[name]
    ref = oracle_grid(name)
    m = _model(name, "bf16")
    mels = _grid(m, name)
    srcs, e = _sources(name)
    conv = Converter(m, T, DEV)
    loop = [conv.convert(srcs[s], e[s], e[t], trim=False, isAdain=name.endswith("2"))
            for s in range(n) for t in range(n)]
    got = ([frob(a, r) for a, r in zip(mels, ref)], [rel_inf(a, r) for a, r in zip(mels, ref)])
    par = ([frob(a, r) for a, r in zip(loop, ref)], [rel_inf(a, r) for a, r in zip(loop, ref)])
    for what, (f, r) in (("batched", got), ("B = 1 loop", par)):
        print(f"{name} bf16 {what} vs fp32 oracle: frob", " ".join(f"{v:.2e}" for v in f),
              "| rel-inf", " ".join(f"{v:.2e}" for v in r))
    assert all(np.isfinite(a).all() for a in mels)
    assert max(got[0]) <= 2 * max(par[0]) and max(got[1]) <= 2 * max(par[1]), (got, par)


# ----------------------------------------------------------------------- Evaluator
def _tree(root, T, n_spk=3, n_utt=6, seed=41):
    """<root>/<speaker>/<k>.npy mels (lengths around T, one shorter, some longer) and the test.pkl list."""
    from autoformer_amd.detinit import det_inputs

    lens = [T, T + 9, T - 7, T + 30, T, T + 3]
    meta = []
    for s in range(n_spk):
        spk = f"p{230 - s}"      # listed in descending order: build_metadata sorts
        os.makedirs(os.path.join(root, spk))
        x, e = det_inputs(n_utt, T + 40, seed=seed + s)
        row = [spk, e[0]]
        for u in range(n_utt):
            np.save(os.path.join(root, spk, f"{u}.npy"), x[u][:lens[(u + s) % len(lens)]])
            row.append(f"{spk}/{u}.npy")
        meta.append(row)
    with open(os.path.join(root, "test.pkl"), "wb") as f:
        pickle.dump(meta, f)
    return meta


class _Cfg:
    pass


def test_generate_result_batched_equals_pair_by_pair(tmp_path):
    """generate_result(..., isAdain=True, batch_families=True) of AutoVC2 on a generated tree (3 speakers x
    6 utterances) with an LstmDV judge on closed-form weights equals the batch_families=False result under
    the same seeds, to the absolute 1e-4 of tests/test_gpu_evaluate.py's generate_result test."""
    import random

    from autoformer_amd.detinit import det_init_
    from autoformer_amd.evaluate import Evaluator
    from autoformer_amd.factory.LstmDV import LstmDV

    name = "AutoVC2"
    T = SETUP[name][0]
    m = _model(name)
    judge = LstmDV()
    det_init_(judge)
    judge = judge.to(DEV).eval()
    meta = _tree(str(tmp_path), T)
    c = _Cfg()
    c.root, c.num_speaker, c.batch_size, c.max_uttr_idx, c.erroment_num = str(tmp_path), 3, 2, 8, 2
    c.len_crop, c.device, c.embedder, c.metadata = T, DEV, judge, meta
    c.all_speaker = sorted(d[0] for d in meta)
    random.seed(3)
    np.random.seed(3)
    E = Evaluator(c)
    res = []
    for flag in (True, False):
        random.seed(17)
        np.random.seed(17)
        out = E.generate_result([m], sound_id=2, isAdain=True, batch_families=flag)
        assert len(out) == 1 and out[0].shape == (3, 3, 3)
        res.append(out[0])
    print("generate_result batched vs pair by pair: max abs", float(np.abs(res[0] - res[1]).max()))
    assert np.abs(res[0] - res[1]).max() < 1e-4
    assert (res[0] >= 0).all() and (res[0] <= 1 + 1e-6).all() and res[0].max() > 0
