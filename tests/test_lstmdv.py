"""The LstmDV speaker embedder (factory/LstmDV.py) and the embedding interface
(autoformer_amd/embed.py) without a GPU: state_dict layout, the golden fixture's
self-consistency against a torch.nn restatement of the reference module written here, and the
batching bookkeeping of embed_utterances / speaker_dvector / build_metadata / cos_scores with a
stub model.  The restatement (RefDV) and the bf16 emulation (emulate_bf16) also serve the GPU
tests of tests/test_gpu_lstmdv.py."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from .conftest import GOLDEN
from .helpers import rel_inf


def golden():
    return np.load(os.path.join(GOLDEN, "lstmdv.npz"))


class RefDV(nn.Module):
    """nn.LSTM(80, 768, 3, batch_first) -> last step -> nn.Linear(768, 256) -> x / ||x||."""

    def __init__(self, num_layers=3, dim_input=80, dim_cell=768, dim_emb=256):
        super().__init__()
        self.lstm = nn.LSTM(dim_input, dim_cell, num_layers, batch_first=True)
        self.embedding = nn.Linear(dim_cell, dim_emb)

    def forward(self, x):
        out, _ = self.lstm(x)
        e = self.embedding(out[:, -1, :])
        return e / e.norm(p=2, dim=-1, keepdim=True)


def ref_model():
    from autoformer_amd.detinit import det_state_dict

    m = RefDV()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in det_state_dict(m.state_dict()).items()})
    return m


def emulate_bf16(sd, x, lens=None):
    """The bf16 compute mode's rounding points on the CPU: bf16 weights, bf16 input and inter-layer
    h, h_{t-1} rounded to bf16 before the recurrent product, fp32 state and accumulation, fp32
    head.  sd: name -> fp32 tensor, x (B, T, 80); row b is captured at step lens[b] - 1."""
    def r(t):
        return t.bfloat16().float()

    B, T, _ = x.shape
    inp = r(x)
    n_layers = sum(1 for k in sd if k.startswith("lstm.weight_ih_l"))
    for n in range(n_layers):
        wih, whh = r(sd[f"lstm.weight_ih_l{n}"]), r(sd[f"lstm.weight_hh_l{n}"])
        bias = sd[f"lstm.bias_ih_l{n}"] + sd[f"lstm.bias_hh_l{n}"]
        Hn = whh.shape[1]
        xp = inp @ wih.t() + bias
        h = torch.zeros(B, Hn)
        c = torch.zeros(B, Hn)
        outs = []
        for t in range(T):
            i, f, g, o = (xp[:, t] + r(h) @ whh.t()).chunk(4, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        hs = torch.stack(outs, 1)  # fp32; only the top layer's captured rows stay fp32
        inp = r(hs)
    last = torch.stack([hs[b, (lens[b] if lens is not None else T) - 1] for b in range(B)])
    e = last @ sd["embedding.weight"].t() + sd["embedding.bias"]
    return e / e.norm(p=2, dim=-1, keepdim=True)


def test_state_dict_layout_matches_reference():
    import factory.LstmDV as M

    g = golden()
    sd = M.LstmDV().state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert isinstance(M.LstmDV().embedding, nn.Linear)


def test_fixture_is_self_consistent():
    g = golden()
    m = ref_model()
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    x24 = torch.from_numpy(g["x24"])
    lens = [int(v) for v in g["lens24"]]
    assert lens == [24, 7, 1]
    with torch.no_grad():
        assert rel_inf(m(x24).numpy(), g["emb24_full"]) < 1e-5
        alone = np.concatenate([m(x24[b:b + 1, :n]).numpy() for b, n in enumerate(lens)])
        assert rel_inf(alone, g["emb24_lens"]) < 1e-5
        assert rel_inf(m(torch.from_numpy(g["x176"])).numpy(), g["emb176"]) < 1e-5
    # a wrong step (T instead of lens[b]) or a wrong row is far outside every bar used against this fixture
    assert rel_inf(g["emb24_full"][1:], g["emb24_lens"][1:]) > 0.1
    assert rel_inf(g["emb176"][0], g["emb176"][1]) > 0.1
    x = torch.from_numpy(g["x176"]).requires_grad_(True)
    loss = F.cosine_embedding_loss(m(x), torch.from_numpy(g["e176"]), torch.ones(2))
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g["step_loss"]), rtol=1e-5)
    grads = dict((n, p.grad) for n, p in m.named_parameters())
    grads["dx"] = x.grad
    for n, gr in grads.items():
        ref_n = float(g["step_gnorm/" + n])
        assert abs(gr.norm().item() - ref_n) <= 1e-4 * ref_n + 1e-9, n
        head = g["step_ghead/" + n]
        assert np.abs(gr.reshape(-1)[:64].numpy() - head).max() <= 1e-4 * max(np.abs(head).max(), 1e-9) + 1e-9, n


def test_bf16_emulation_drift_is_small_and_sees_wrong_steps():
    """The emulation the GPU bar is built from sits a few 1e-3 from the fp32 fixture, while the
    embedding captured at the wrong step (T instead of lens[b]) is two orders further away."""
    g = golden()
    sd = {k: v.detach() for k, v in ref_model().state_dict().items()}
    x24 = torch.from_numpy(g["x24"])
    lens = [int(v) for v in g["lens24"]]
    d_emu = rel_inf(emulate_bf16(sd, x24, lens).numpy(), g["emb24_lens"])
    assert d_emu < 1e-2, d_emu
    wrong = rel_inf(emulate_bf16(sd, x24, None).numpy(), g["emb24_lens"])
    assert wrong > 20 * d_emu, (wrong, d_emu)


class _Stub:
    """(x, lens) -> (B, 4): [first frame's first bin, reported length, padded T, frame sum up to
    the length]; records every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, x, lens):
        self.calls.append((tuple(x.shape), list(lens)))
        rows = [[float(x[b, 0, 0]), float(n), float(x.shape[1]), float(x[b, :n].sum())] for b, n in enumerate(lens)]
        # nothing but zeros may sit past a row's own length
        assert all(float(x[b, n:].abs().sum()) == 0.0 for b, n in enumerate(lens))
        return torch.tensor(rows)


def _mels(lengths, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.rand(n, 80).astype(np.float32) + 0.5) for n in lengths]


def test_embed_utterances_bookkeeping():
    from autoformer_amd.embed import embed_utterances, speaker_dvector

    lengths = [3, 176, 176, 200, 41, 300]
    mels = _mels(lengths)
    stub = _Stub()
    out = embed_utterances(stub, mels, len_crop=176, max_batch=4)
    assert out.shape == (6, 4) and out.dtype == np.float32
    # input order, each row about its own utterance; short ones count as len_crop frames
    for i, m in enumerate(mels):
        assert out[i, 0] == m[0, 0]
        assert out[i, 1] == max(lengths[i], 176)
        np.testing.assert_allclose(out[i, 3], m.sum(), rtol=1e-5)
    # sorted by length into batches of at most max_batch, each padded to its longest member
    assert [c[0][0] for c in stub.calls] == [4, 2]
    assert stub.calls[0] == ((4, 176, 80), [176] * 4) and stub.calls[1] == ((2, 300, 80), [200, 300])
    assert list(out[:, 2]) == [176, 176, 176, 300, 176, 300]
    # one batch when the cap allows; the default cap of a plain callable
    stub = _Stub()
    embed_utterances(stub, mels, len_crop=176)
    assert stub.calls == [((6, 300, 80), [176, 176, 176, 176, 200, 300])]
    stub = _Stub()
    embed_utterances(stub, mels, len_crop=10, max_batch=1)
    assert [c[1] for c in stub.calls] == [[max(n, 10)] for n in sorted(lengths)]
    np.testing.assert_allclose(speaker_dvector(_Stub(), mels, 176, 4), out.mean(axis=0), rtol=1e-6)
    with pytest.raises(ValueError):
        embed_utterances(stub, [])
    with pytest.raises(ValueError):
        embed_utterances(stub, mels, max_batch=0)


def test_build_metadata_structure(tmp_path):
    from autoformer_amd.data import Utterances
    from autoformer_amd.embed import build_metadata, speaker_dvector

    spk_lengths = {"p226": [30, 12, 50], "p225": [20, 64, 9, 41]}
    store = {}
    for spk, lens in spk_lengths.items():
        os.makedirs(tmp_path / spk)
        for k, m in enumerate(_mels(lens, seed=len(spk_lengths[spk]))):
            np.save(tmp_path / spk / f"u{9 - k}.npy", m)
            store[(spk, f"u{9 - k}.npy")] = m
    (tmp_path / "p225" / "notes.txt").write_text("not a mel")
    meta = build_metadata(str(tmp_path), _Stub(), num_uttrs=3, len_crop=32)
    assert [e[0] for e in meta] == ["p225", "p226"]
    for e in meta:
        files = sorted(f for (s, f) in store if s == e[0])[:3]
        assert e[2:] == [os.path.join(e[0], f) for f in files]
        want = speaker_dvector(_Stub(), [store[(e[0], f)] for f in files], 32)
        assert e[1].shape == (4,) and e[1].dtype == np.float32
        np.testing.assert_allclose(e[1], want, rtol=1e-6)
    with pytest.raises(ValueError):
        build_metadata(str(tmp_path), _Stub(), num_uttrs=4, len_crop=32)  # p226 has three
    # the list is what the training loader reads
    with open(tmp_path / "train.pkl", "wb") as f:
        pickle.dump(meta, f)
    ds = Utterances(str(tmp_path), 32, num_threads=2)
    assert len(ds) == 2 and ds.train_dataset[0][0] == "p225" and len(ds.train_dataset[0]) == 5
    np.testing.assert_array_equal(ds.train_dataset[1][2], store[("p226", "u7.npy")])


def test_cos_scores_match_torch():
    from autoformer_amd.embed import cos_scores

    rng = np.random.RandomState(2)
    a, b = rng.randn(3, 256).astype(np.float32), rng.randn(4, 256).astype(np.float32)
    b[1] = -a[0]  # a negative cosine clamps to 0
    got = cos_scores(a, b)
    assert got.shape == (3, 4)
    for i in range(3):
        for j in range(4):
            ref = torch.clamp(F.cosine_similarity(torch.from_numpy(a[i:i + 1]), torch.from_numpy(b[j:j + 1]), dim=1,
                                                  eps=1e-8), min=0.0).item()
            assert abs(got[i, j] - ref) < 1e-6
    assert got[0, 1] == 0.0
    assert cos_scores(a[0], torch.from_numpy(a[0])).shape == (1, 1)
    assert abs(cos_scores(a[0], a[0])[0, 0] - 1.0) < 1e-6


def test_lstmdv_refuses_cpu_tensors():
    import factory.LstmDV as M

    m = M.LstmDV()
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 24, 80))
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(torch.zeros(2, 24, 80), [24, 3])


def test_embed_cli_refuses_cpu():
    from autoformer_amd import embed

    with pytest.raises(SystemExit):
        embed.main(["--spmel", "x", "--ckpt", "y", "--device", "cpu"])
    with pytest.raises(SystemExit):
        embed.main(["--spmel", "x"])


def test_converter_embedder_is_optional():
    from autoformer_amd.convert import Converter

    c = Converter(None, 64, device="cpu")
    assert c.embedder is None
    with pytest.raises(RuntimeError):
        c.convert_between(np.zeros((10, 80), np.float32), [], [])
