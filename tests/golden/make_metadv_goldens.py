"""Generate the golden fixture of the MetaDV speaker classifier from the *reference* module (survey
container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metadv_goldens.py

Imports achyun/Autoformer's factory.MetaDV from /root/reference (read-only) on the CPU, loads the
closed-form weights of autoformer_amd.detinit and records into tests/golden/metadv.npz (inputs,
outputs, gradient norms and 64-element heads; no weights):

  keys, shapes            the reference MetaDV(256) state_dict key order and shapes
  x176, e176              det_inputs(2, 176)
  lefts176                the four window starts the reference draws under random.seed(7) at T = 176
  pred176, dvec176        its outputs for them
  pred128, dvec128        x176[:, :128]: T = crop_len, every start is 0
  lens200, lefts200       det_inputs(3, 200) with lengths [200, 150, 128]: each row embedded alone at
  pred200, dvec200        its own length, x[b:b+1, :lens[b]], as the reference embeds; lefts200 (4, 3)
                          holds the starts it drew for each row (random.seed(9) before row 0)
  step_*                  one training step on x176 (random.seed(7)): loss = cosine_embedding_loss(
                          d_vec, e176, ones) + cross_entropy(pred, [3, 200]); gnorm/ and ghead/ per
                          parameter (as make_goldens._grads) and of dx
The reference never travels to the GPU box; only these arrays do.
"""
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
from autoformer_amd.detinit import det_init_, det_inputs  # noqa: E402

sys.path.insert(0, REF)
torch.manual_seed(0)
torch.set_num_threads(8)

LENS200 = [200, 150, 128]
LABELS = [3, 200]
CROP, S = 128, 4


def _grads(named):
    out = {}
    for name, g in named:
        out["gnorm/" + name] = np.array(g.norm().item(), dtype=np.float64)
        out["ghead/" + name] = g.detach().reshape(-1)[:64].numpy().copy()
    return out


def _peek(T):
    """The starts the next forward at T frames will draw, without consuming them."""
    st = random.getstate()
    lefts = [random.randint(0, T - CROP) for _ in range(S)]
    random.setstate(st)
    return lefts


def make():
    from factory.MetaDV import MetaDV

    m = MetaDV(256)
    det_init_(m)
    m.train()
    sd = m.state_dict()
    rec = {"keys": np.array(list(sd.keys())),
           "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}
    x176, e176 = det_inputs(2, 176)
    x200, _ = det_inputs(3, 200)
    rec.update({"x176": x176, "e176": e176, "lens200": np.array(LENS200)})
    with torch.no_grad():
        random.seed(7)
        rec["lefts176"] = np.array(_peek(176))
        pred, dvec = m(torch.from_numpy(x176))
        rec.update({"pred176": pred.numpy(), "dvec176": dvec.numpy()})
        pred, dvec = m(torch.from_numpy(x176[:, :128]))
        rec.update({"pred128": pred.numpy(), "dvec128": dvec.numpy()})
        random.seed(9)
        lefts, preds, dvecs = [], [], []
        for b, n in enumerate(LENS200):
            lefts.append(_peek(n))
            pred, dvec = m(torch.from_numpy(x200[b:b + 1, :n]))
            preds.append(pred.numpy())
            dvecs.append(dvec.numpy())
        rec.update({"lefts200": np.array(lefts).T.copy(), "pred200": np.concatenate(preds),
                    "dvec200": np.concatenate(dvecs)})
    x = torch.from_numpy(x176).requires_grad_(True)
    random.seed(7)
    pred, dvec = m(x)
    loss = F.cosine_embedding_loss(dvec, torch.from_numpy(e176), torch.ones(2)) + F.cross_entropy(
        pred, torch.tensor(LABELS))
    m.zero_grad()
    loss.backward()
    rec["step_loss"] = np.array(loss.item(), dtype=np.float64)
    rec["step_labels"] = np.array(LABELS)
    rec.update({"step_" + k: v for k, v in _grads((n, p.grad) for n, p in m.named_parameters()).items()})
    rec.update({"step_" + k: v for k, v in _grads([("dx", x.grad)]).items()})
    path = os.path.join(HERE, "metadv.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes", "lefts176", rec["lefts176"], "lefts200", rec["lefts200"].tolist())


if __name__ == "__main__":
    make()
