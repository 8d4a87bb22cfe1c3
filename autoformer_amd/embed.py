"""Speaker embeddings from mel-spectrograms with the LstmDV d-vector net (factory/LstmDV.py) or the
MetaDV classifier (factory/MetaDV.py, `--embedder MetaDV`): what
the reference does in make_data/make_metadata.ipynb (the `train.pkl` speaker entries) and in the
second half of util/evaluate.py (get_dv :100-106, the cosine scores :140-146, :205-211).

  embed_utterances(model, mels)      one unit-norm embedding per utterance, (N, E) on the host
  speaker_dvector(model, mels)       their mean, not renormalised (make_metadata.ipynb cell 5)
  build_metadata(root, model)        the train.pkl list autoformer_amd.data.Utterances reads
  cos_scores(a, b)                   clamp(cosine_similarity, min=0) of every pair

The reference embeds utterances one at a time at B = 1: one shorter than `len_crop` is zero-padded
at the end to `len_crop` frames (and embedded as `len_crop` frames), a longer one goes in whole.
embed_utterances keeps those semantics and batches: utterances are sorted by length into batches no
larger than the forward-only recurrence admits in one launch, each batch is padded to its longest
member, and `lens` tells the model which frame is each row's last (rows are independent, so the
padding past a row's own length never reaches its embedding).

`model` is any callable (x (B, T, 80) tensor, lens list) -> (B, E) tensor; an LstmDV is called under
torch.no_grad() on its own device.  An embedder that returns a tuple -- MetaDV's (predictions, d_vec) --
contributes its last entry, the d-vector.  One with a `crop_len` of its own (MetaDV cuts 128-frame
windows) refuses a `len_crop` below it: a shorter utterance would be padded to less than one window.

MetaDV draws its windows from Python's `random`, one utterance's crops after another's within a
batch, and the batches are sorted by length: the batched call therefore does NOT reproduce the draw
order of the reference's one-utterance-at-a-time loop.  `lefts` (one row of window starts per
utterance, in input order) fixes the windows and gives exact parity with single-utterance calls.

  python -m autoformer_amd.embed --spmel DIR --ckpt FILE --out train.pkl
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

DEFAULT_MAX_BATCH = 64


def _pad_short(mel, len_crop):
    """make_metadata.ipynb cell 4-5: zero padding at the end up to len_crop frames."""
    mel = np.asarray(mel, dtype=np.float32)
    if mel.ndim != 2 or mel.shape[0] < 1:
        raise ValueError(f"an utterance is a (T >= 1, n_mels) array, got shape {mel.shape}")
    if mel.shape[0] >= len_crop:
        return mel
    out = np.zeros((len_crop, mel.shape[1]), dtype=np.float32)
    out[:mel.shape[0]] = mel
    return out


def _model_device(model):
    if isinstance(model, torch.nn.Module):
        for p in model.parameters():
            return p.device
    return None


def _batch_cap(model, max_batch):
    if max_batch is not None:
        if int(max_batch) < 1:
            raise ValueError(f"max_batch must be >= 1, got {max_batch}")
        return int(max_batch)
    admit = getattr(model, "max_infer_batch", None)
    n = admit() if callable(admit) else 0
    return n if n > 0 else DEFAULT_MAX_BATCH


@torch.no_grad()
def embed_utterances(model, mels, len_crop=176, max_batch=None, lefts=None):
    """(N, E) float32 embeddings of the utterances `mels` (each (T_i, 80)), in input order.
    max_batch None: what model.max_infer_batch() admits per launch (64 for a plain callable).
    lefts (an embedder that crops windows only): per utterance, in input order, its window starts;
    None lets the embedder draw them (not in the reference's per-utterance order, see above)."""
    need = getattr(model, "crop_len", None)
    if need is not None and len_crop < int(need):
        raise ValueError(f"len_crop = {len_crop} is below the embedder's crop_len = {int(need)}: an utterance padded "
                         f"to {len_crop} frames is shorter than one of its windows")
    mels = [_pad_short(m, len_crop) for m in mels]
    if not mels:
        raise ValueError("embed_utterances: no utterances")
    if lefts is not None and len(lefts) != len(mels):
        raise ValueError(f"lefts must hold one row of window starts per utterance ({len(mels)}), got {len(lefts)}")
    cap = _batch_cap(model, max_batch)
    dev = _model_device(model)
    order = sorted(range(len(mels)), key=lambda i: mels[i].shape[0])  # stable: ties keep input order
    out = [None] * len(mels)
    for k in range(0, len(order), cap):
        idx = order[k:k + cap]
        lens = [int(mels[i].shape[0]) for i in idx]
        x = np.zeros((len(idx), max(lens), mels[idx[0]].shape[1]), dtype=np.float32)
        for r, i in enumerate(idx):
            x[r, :lens[r]] = mels[i]
        xt = torch.from_numpy(x)
        if dev is not None:
            xt = xt.to(dev)
        if lefts is None:
            emb = model(xt, lens)
        else:  # the embedder takes crops-major rows: sample_count rows of B starts
            emb = model(xt, lens, lefts=[list(col) for col in zip(*[lefts[i] for i in idx])])
        if isinstance(emb, (tuple, list)):
            emb = emb[-1]  # (predictions, d_vec): the d-vector
        emb = emb.detach().float().cpu().numpy()
        if dev is not None and dev.type == "cuda":
            from . import kernels as K

            K.check_faults(dev)  # a recurrence that timed out left this batch unfinished
        if emb.shape[0] != len(idx):
            raise RuntimeError(f"the embedder returned {emb.shape[0]} rows for a batch of {len(idx)}")
        for r, i in enumerate(idx):
            out[i] = emb[r]
    return np.stack(out).astype(np.float32)


def speaker_dvector(model, mels, len_crop=176, max_batch=None, lefts=None):
    """The speaker's d-vector (E,): the mean of its utterances' embeddings, not renormalised
    (make_metadata.ipynb cell 5 np.mean(embs, axis=0); evaluate.py:100-106)."""
    return embed_utterances(model, mels, len_crop, max_batch, lefts).mean(axis=0)


def build_metadata(root, model, num_uttrs=68, len_crop=176, max_batch=None):
    """The train.pkl list for the mel folder `root` (<root>/<speaker>/*.npy): per speaker, in sorted
    order, [speaker, d-vector of its first num_uttrs utterances (sorted by name), every one of those
    utterances' relative paths, sorted].  A speaker with fewer than num_uttrs utterances is an error,
    as in the notebook."""
    speakers = []
    for spk in sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))):
        files = sorted(f for f in os.listdir(os.path.join(root, spk)) if f.endswith(".npy"))[:num_uttrs]
        if len(files) < num_uttrs:
            raise ValueError(f"speaker {spk}: {len(files)} utterances, num_uttrs = {num_uttrs}")
        mels = [np.load(os.path.join(root, spk, f)) for f in files]
        dvec = speaker_dvector(model, mels, len_crop, max_batch)
        speakers.append([spk, dvec] + [os.path.join(spk, f) for f in files])
    if not speakers:
        raise ValueError(f"{root}: no speaker folders")
    return speakers


def cos_scores(a, b):
    """evaluate.py:140-146: clamp(cosine_similarity(a_i, b_j, eps=1e-8), min=0) for every pair,
    (Na, Nb); a (Na, E) / (E,), b (Nb, E) / (E,), arrays or tensors."""
    a = torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).float().cpu()
    b = torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b).float().cpu()
    a = a.reshape(-1, a.shape[-1])
    b = b.reshape(-1, b.shape[-1])
    cos = torch.nn.functional.cosine_similarity(a[:, None, :], b[None, :, :], dim=2, eps=1e-8)
    return torch.clamp(cos, min=0.0).numpy()


def _parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m autoformer_amd.embed",
                                description="speaker d-vectors + train.pkl for a folder of mel-spectrograms "
                                            "(make_data/make_metadata.ipynb)")
    p.add_argument("--spmel", required=True, help="folder with one sub-folder of (T, 80) .npy mels per speaker")
    p.add_argument("--embedder", choices=["LstmDV", "MetaDV"], default="LstmDV", help="the speaker embedder")
    p.add_argument("--num_classes", type=int, default=256, help="MetaDV: classes of its checkpoint's classifier head")
    p.add_argument("--ckpt", help="the embedder's state_dict (torch.save); required unless --det_init")
    p.add_argument("--out", help="metadata file to write (default: <spmel>/train.pkl)")
    p.add_argument("--num_uttrs", type=int, default=68)
    p.add_argument("--len_crop", type=int, default=176)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--det_init", action="store_true", help="closed-form weights instead of --ckpt (smoke runs)")
    return p


def main(argv=None):
    args = _parser().parse_args(argv)
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    if not args.ckpt and not args.det_init:
        raise SystemExit(f"--ckpt FILE (an {args.embedder} state_dict) is required unless --det_init is given")
    import autoformer_amd as A

    A.set_compute(args.dtype)
    if args.embedder == "MetaDV":
        from .factory.MetaDV import MetaDV

        model = MetaDV(args.num_classes)
        if args.len_crop < model.crop_len:
            raise SystemExit(f"--len_crop {args.len_crop} is below MetaDV's crop_len = {model.crop_len}")
    else:
        from .factory.LstmDV import LstmDV

        model = LstmDV()
    if args.det_init:
        from .detinit import det_init_

        det_init_(model)
    else:
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu", weights_only=True))
    model.to(args.device).eval()
    meta = build_metadata(args.spmel, model, args.num_uttrs, args.len_crop)
    out = args.out or os.path.join(args.spmel, "train.pkl")
    with open(out, "wb") as f:
        pickle.dump(meta, f)
    print(f"{out}: {len(meta)} speakers, {len(meta[0]) - 2} utterances each")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
