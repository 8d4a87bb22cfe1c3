"""All-pairs voice conversion and the Evaluator (reference util/evaluate.py, second half:
generate_real_dv :108-121, get_real_data_cos :123-151, get_cos_rc :153-162, get_cos_trans :164-175,
generate_result :177-218; and the all-pairs wav export of generate.ipynb cell 8).

  plan_grid(src_lens, pairs, len_crop)     the crop draws of a grid, in the reference's order (host only)
  convert_grid(model, sources, emb)        every (source, target) conversion, batched where that is exact
  grid_family(model)                       which batched path batch_families=True gives a model, or None
  Evaluator(config)                        the reference's class: same fields, same method names
  python -m autoformer_amd.evaluate        cosine summaries of a model, optionally the grid as wavs

The reference converts one utterance at a time with the model in TRAIN mode, so every BatchNorm takes
the statistics of the utterance in flight.  A plain batched forward would take them over the whole
batch -- a different function.  convert_grid batches under layers.per_utterance_bn(): BatchNorm
statistics per utterance segment (bn_seg.hip), which makes each row of the batch the B = 1 forward.
The encoder output depends on the source alone, so it runs once per distinct (source, crop offset)
instead of once per pair; only the decoder and the postnet run per pair.

Batched by default: AutoVC (train or eval mode).  Every other family is converted pair by pair through
convert.Converter.get_trans_mel, the one-utterance path, on the crops the plan drew: the same draws, the
same results, no batching.

Batched on request (batch_families=True, `--batch_families`; grid_family names the path):
  MetaConv / MetaPool         their GroupNorms and mixers are per utterance already, their BatchNorms
                              (the L = 344 and L = 88 segments of the decoder included) take the
                              per-segment statistics like AutoVC's; len_crop must be 176
  AutoVC2 / MetaConv2 / MetaPool2 with isAdain
                              the AdaIN moments and the AdaIN itself are whole-tensor ops -- at B = 1 the
                              utterance; under per_utterance_bn() they are taken per utterance segment
                              (seg_moments.hip), in train and in eval mode.  The reference takes the
                              postnet's statistics from the SOURCE mel and runs the encoder twice on it
                              (util/evaluate.py:80-81); here one encoder pass per distinct (source, crop
                              offset) gives the codes and the features, gathered per pair.
Left pair by pair whatever the flag: the `*_Adjust` models.  Their target-side Adjust pass depends on
each pair's own target crop and runs a 3-layer recurrence per pair -- a separate piece of work.

Random draws follow the reference: crop offsets from numpy's global state (source, then target, per
pair and per model), enrolment utterances and MetaDV windows from Python's `random`.
"""
from __future__ import annotations

import os
import pickle
import random
import wave

import numpy as np
import torch

from .convert import Converter, crop_mel

SAMPLE_RATE, HOP = 22050, 256


# ----------------------------------------------------------------------------- the plan (host only)
def _draw(T, len_crop, rng):
    """crop_mel's bookkeeping on a length: (left, pad_size), one rng draw when T > len_crop."""
    if T < len_crop:
        return 0, len_crop - T
    if T == len_crop:
        return 0, 0
    return int(rng.randint(0, T - len_crop)), 0


def _cut(mel, left, len_crop):
    """The planned crop of a host mel: rows [left, left + len_crop), zero-padded at the end."""
    mel = np.asarray(mel, dtype=np.float32)
    out = np.zeros((len_crop,) + mel.shape[1:], dtype=np.float32)
    part = mel[left:left + len_crop]
    out[:part.shape[0]] = part
    return out


class GridPlan:
    """pairs[i] = (source, target); src_crop[i] / tgt_crop[i] = (left, pad_size) of that pair's crops
    (tgt_crop None when no target mels are drawn); enc_rows: the distinct (source, left) in first-use
    order -- one encoder row each; pair_enc[i]: pair i's row of enc_rows."""

    def __init__(self, pairs, src_crop, tgt_crop):
        self.pairs, self.src_crop, self.tgt_crop = pairs, src_crop, tgt_crop
        rows = {}
        self.pair_enc = [rows.setdefault((s, c[0]), len(rows)) for (s, _), c in zip(pairs, src_crop)]
        self.enc_rows = list(rows)
        self.pads = [c[1] for c in src_crop]


def all_pairs(n):
    return [(s, t) for s in range(n) for t in range(n)]


def plan_grid(src_lens, pairs=None, len_crop=176, rng=np.random, tgt_lens=None, copies=1):
    """The crop draws of a grid in the reference's order (evaluate.py:185-199, :66-67): pair after
    pair, within a pair model after model (`copies` plans, one per model), and for each the source
    crop first, then -- when target mels are loaded (tgt_lens) -- the target crop.  Lengths only: no
    device, no mel is touched.  Returns `copies` GridPlans."""
    pairs = all_pairs(len(src_lens)) if pairs is None else [(int(s), int(t)) for s, t in pairs]
    src = [[] for _ in range(copies)]
    tgt = [[] for _ in range(copies)]
    for s, t in pairs:
        for k in range(copies):
            src[k].append(_draw(int(src_lens[s]), len_crop, rng))
            if tgt_lens is not None:
                tgt[k].append(_draw(int(tgt_lens[t]), len_crop, rng))
    return [GridPlan(pairs, src[k], tgt[k] if tgt_lens is not None else None) for k in range(copies)]


# ----------------------------------------------------------------------------- the grid
def batched_family(model, isAdjust=False, isAdain=False):
    """Whether convert_grid batches this model: AutoVC alone (see the module docstring)."""
    from .factory.AutoVC import AutoVC

    return type(model) is AutoVC and not isAdjust and not isAdain


def grid_family(model, isAdjust=False, isAdain=False):
    """The batched path convert_grid(..., batch_families=True) takes for this model, by exact type:
    "autovc" (AutoVC), "meta" (MetaConv, MetaPool), "adain" (AutoVC2, MetaConv2, MetaPool2 called with
    isAdain) -- or None: the `*_Adjust` models, isAdjust, an AdaIN model called without isAdain, anything
    else.  None stays on the pair-by-pair path."""
    from .factory.AutoVC import AutoVC
    from .factory.AutoVC2 import AutoVC2
    from .factory.MetaConv import MetaConv
    from .factory.MetaConv2 import MetaConv2
    from .factory.MetaPool import MetaPool
    from .factory.MetaPool2 import MetaPool2

    if isAdjust:
        return None
    if type(model) in (AutoVC2, MetaConv2, MetaPool2):
        return "adain" if isAdain else None
    if isAdain:
        return None
    return {AutoVC: "autovc", MetaConv: "meta", MetaPool: "meta"}.get(type(model))


@torch.no_grad()
def convert_grid(model, sources, emb, pairs=None, len_crop=176, max_batch=64, rng=np.random, targets=None,
                 isAdjust=False, isAdain=False, plan=None, device=None, batch_families=False):
    """Converted mels of every pair: (mels, pads) -- mels[i] the (len_crop, 80) float32 host mel of
    pairs[i] = (source, target) (default: all N*N pairs, source-major), pads[i] the zero frames that
    padded its source (cut them with mels[i][:len_crop - pads[i]], the reference's isPlay branch).

    sources: N host mels (T_i, 80); emb: (N, E) speaker embeddings; targets: N host mels whose crops
    are drawn after each pair's source crop as get_trans_mel does (needed by isAdjust, otherwise only
    their draws matter); plan: a GridPlan drawn beforehand (plan_grid) instead of drawing here.

    AutoVC is batched: the encoder once per distinct (source, crop offset), decoder + postnet over the
    pairs in chunks of at most max_batch, all under layers.per_utterance_bn() -- a train-mode model
    gives each row its B = 1 train-mode result and its BatchNorm buffers are left as they were; an
    eval-mode model takes its usual path.  Any other family (MetaConv / MetaPool, the AdaIN `*2`
    variants, `*_Adjust`) is NOT batched by default: each pair goes through Converter.get_trans_mel on
    the planned crops, exactly the one-utterance path.

    batch_families=True: every family for which grid_family is not None runs batched the same way --
    MetaConv / MetaPool (len_crop 176 only: MetaBlock.frames raises otherwise) and, with isAdain, the
    AdaIN `*2` variants, whose encoder pass also returns the per-row AdaIN features (the reference takes
    them from the source mel); the decode gathers them by plan.pair_enc.  The plan, the draws, the pads
    and the return shapes are those of the pair-by-pair path.  The reference's loop -- and the
    pair-by-pair path here -- moves a train-mode model's BatchNorm running statistics and
    num_batches_tracked with every forward; the batched path leaves the model as it was.  The `*_Adjust`
    models stay pair by pair."""
    if not isinstance(batch_families, (bool, np.bool_)):
        raise TypeError(f"batch_families must be a bool, got {type(batch_families).__name__}")
    if int(max_batch) < 1:
        raise ValueError(f"max_batch must be >= 1, got {max_batch}")
    emb = np.asarray(emb, dtype=np.float32)
    if emb.ndim != 2 or emb.shape[0] != len(sources):
        raise ValueError(f"emb must be (N = {len(sources)}, E), got {emb.shape}")
    if isAdjust and targets is None:
        raise ValueError("isAdjust conversion needs the target mels (evaluate.py:79)")
    if plan is None:
        plan = plan_grid([m.shape[0] for m in sources], pairs, len_crop, rng,
                         None if targets is None else [m.shape[0] for m in targets])[0]
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if batch_families:
        family = grid_family(model, isAdjust, isAdain)
    else:
        family = "autovc" if batched_family(model, isAdjust, isAdain) else None
    if family is None:
        conv = Converter(model, len_crop, device)
        mels = []
        for i, (s, t) in enumerate(plan.pairs):
            src = _cut(sources[s], plan.src_crop[i][0], len_crop)  # len_crop long: the Converter draws nothing
            tgt = None if targets is None else _cut(targets[t], plan.tgt_crop[i][0], len_crop)
            _, _, trans = conv.get_trans_mel(src, tgt, emb[s], emb[t], isAdjust, isAdain)
            mels.append(trans[0].float().cpu().numpy())
        return mels, list(plan.pads)

    from . import layers as Lyr
    from .factory.AutoVC import decode

    K_ = int(max_batch)
    x_rows = torch.from_numpy(np.stack([_cut(sources[s], left, len_crop) for s, left in plan.enc_rows])).to(device)
    e_all = torch.from_numpy(emb).to(device)
    e_rows = e_all[torch.tensor([s for s, _ in plan.enc_rows], device=device)]
    pair_enc = torch.tensor(plan.pair_enc, device=device)
    pair_trg = torch.tensor([t for _, t in plan.pairs], device=device)
    out, feats = [], None
    with Lyr.per_utterance_bn():
        chunks = [(x_rows[k:k + K_].contiguous(), e_rows[k:k + K_].contiguous()) for k in range(0, x_rows.shape[0], K_)]
        if family == "adain":
            # one encoder pass per row: the codes and the three [mean (rows,), std (rows,)] feature pairs
            parts = [model.encoder.codes_and_features(x, e) for x, e in chunks]
            codes = torch.cat([c for c, _ in parts])
            feats = [[torch.cat([f[j][i] for _, f in parts]) for i in range(2)] for j in range(3)]
        else:
            codes = torch.cat([model.encoder.codes_flat(x, e) for x, e in chunks])
        for k in range(0, len(plan.pairs), K_):
            rows = pair_enc[k:k + K_]
            f_rows = None if feats is None else [[f[0][rows].contiguous(), f[1][rows].contiguous()] for f in feats]
            _, psnt, _ = decode(model, x_rows[rows], codes[rows].contiguous(), e_all[pair_trg[k:k + K_]].contiguous(),
                                f_rows)
            out.append(psnt.squeeze(1).float().cpu().numpy())
    if device.type == "cuda":
        from . import kernels as K

        K.check_faults(device)
    allm = np.concatenate(out)
    return [allm[i] for i in range(allm.shape[0])], list(plan.pads)


# ----------------------------------------------------------------------------- scores
def get_cos_rc(cos_res):
    """evaluate.py:153-162 on an (N, N, N) array cos[source][target][judged speaker]: the mean over
    speakers i of the reconstruction i -> i scored against i, and of the same reconstruction scored
    against the other N - 1 speakers."""
    cos_res = np.asarray(cos_res)
    N = len(cos_res)
    own = np.array([cos_res[i, i, i] for i in range(N)])
    others = np.array([(cos_res[i, i].sum() - cos_res[i, i, i]) / (N - 1) for i in range(N)])
    return own.sum() / N, others.sum() / N


def get_cos_trans(cos_res):
    """evaluate.py:164-175: for source i, the conversions i -> t scored against their target t
    (t != i, mean over the N - 1 targets), and every off-diagonal score cos[i][t][k != t] (mean over
    its (N - 1) N entries -- the reference's count, the i -> i row included); both averaged over i."""
    cos_res = np.asarray(cos_res)
    N = len(cos_res)
    hit = [(np.trace(cos_res[i]) - cos_res[i, i, i]) / (N - 1) for i in range(N)]
    miss = [(cos_res[i].sum() - np.trace(cos_res[i])) / ((N - 1) * N) for i in range(N)]
    return sum(hit) / N, sum(miss) / N


# ----------------------------------------------------------------------------- Evaluator
class Evaluator:
    """util/evaluate.py's Evaluator.  config carries root, num_speaker, batch_size, max_uttr_idx,
    erroment_num, len_crop, device, all_speaker, embedder (an LstmDV / MetaDV judge or None) and
    metadata (the test.pkl list: [speaker, d-vector, relative mel paths ...]); optionally `vocoder`,
    a melgan.MelVocoder -- the reference loads model/static/multi_speaker.pt unconditionally, here a
    missing vocoder only disables get_wavs.  With a judge, the enrolment d-vectors (all_dv) are made
    at construction, as in the reference."""

    def __init__(self, config):
        self.root = config.root
        self.num_speaker = config.num_speaker
        self.batch_size = config.batch_size
        self.max_uttr_idx = config.max_uttr_idx
        self.erroment_num = config.erroment_num
        self.len_crop = config.len_crop
        self.device = config.device
        self.all_speaker = config.all_speaker
        self.embedder = config.embedder
        self.enrroment_idx = []
        self.remain_idx = np.arange(2, config.max_uttr_idx)
        self.metadata = self.build_metadata(config.metadata)
        self.vocoder = getattr(config, "vocoder", None)
        if self.embedder is not None:
            self.all_dv = self.generate_real_dv()

    # ---- data
    def build_metadata(self, metadata):
        """The entries whose speaker is in all_speaker, sorted (by speaker name)."""
        keep = [data for data in metadata if str(data[0]) in self.all_speaker]
        return sorted(keep, key=lambda d: str(d[0]))

    def _load(self, speaker_id, sound_id):
        path_ = self.metadata[speaker_id][sound_id].replace("\\", "/")
        return np.load(f"{self.root}/{path_}")

    def crop_mel(self, tmp):
        """(T, 80) host mel -> ((1, len_crop, 80) device tensor, pad_size); numpy's global rng."""
        mel, pad = crop_mel(np.asarray(tmp), self.len_crop)
        t = torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32))
        return t.unsqueeze(0).to(self.device), pad

    def get_mel(self, speaker_id, sound_id):
        return self.crop_mel(self._load(speaker_id, sound_id))

    def _emb(self):
        return np.stack([np.asarray(d[1], dtype=np.float32).reshape(-1) for d in self.metadata])

    def get_trans_mel(self, model, source_id, target_id, sound_id, isAdjust, isAdain, isPlay=False):
        """(mel_source, mel_target, mel_trans), (1, T, 80) device tensors (evaluate.py:56-94)."""
        emb = self._emb()
        return Converter(model, self.len_crop, self.device).get_trans_mel(
            self._load(source_id, sound_id), self._load(target_id, sound_id), emb[source_id], emb[target_id],
            isAdjust, isAdain, isPlay)

    def get_wavs(self, mel):
        """(B, 80, T) mel -> (B, T*256) waveform."""
        if self.vocoder is None:
            raise RuntimeError("Evaluator was built without a vocoder (config.vocoder = MelVocoder(...))")
        return self.vocoder.inverse(mel)

    # ---- the judge
    def _embed(self, mels):
        """Batched embeddings of len_crop-frame host mels, (n, E); a MetaDV judge's windows are drawn
        one utterance after another from Python's `random`, the order of one-utterance calls."""
        from .embed import embed_utterances

        lefts = None
        if hasattr(self.embedder, "draw_lefts"):
            lefts = [self.embedder.draw_lefts(int(m.shape[0])) for m in mels]
        return embed_utterances(self.embedder, mels, self.len_crop, lefts=lefts)

    def _cropped(self, speaker_id, sound_ids):
        return [crop_mel(self._load(speaker_id, i), self.len_crop)[0] for i in sound_ids]

    def get_dv(self, speaker_id):
        """(1, E): the enrolment utterances' embeddings summed and divided by erroment_num."""
        embs = self._embed(self._cropped(speaker_id, self.enrroment_idx))
        dv = embs.astype(np.float32).sum(axis=0, keepdims=True) / self.erroment_num
        return torch.from_numpy(dv).to(self.device)

    def generate_real_dv(self):
        for _ in range(self.erroment_num):
            pick = random.choice(self.remain_idx)
            self.remain_idx = np.delete(self.remain_idx, np.where(self.remain_idx == pick))
            self.enrroment_idx.append(pick)
        return [self.get_dv(i) for i in range(len(self.all_speaker))]

    def _all_dv(self):
        return np.concatenate([d.detach().float().cpu().numpy().reshape(1, -1) for d in self.all_dv])

    def get_real_data_cos(self):
        """(N, N) mean and (N, N) standard deviation: row i, column j -- speaker i's remaining
        (non-enrolment) utterances scored against speaker j's d-vector."""
        from .embed import cos_scores

        cos_result = np.zeros((self.num_speaker, self.num_speaker))
        var_result = np.zeros((self.num_speaker, self.num_speaker))
        dvs = self._all_dv()
        for i in range(len(self.all_speaker)):
            cos = cos_scores(self._embed(self._cropped(i, self.remain_idx)), dvs).astype(np.float32)
            cos_result[i, :cos.shape[1]] = cos.mean(axis=0)
            var_result[i, :cos.shape[1]] = cos.std(axis=0)
        return cos_result, var_result

    def get_cos_rc(self, cos_res):
        return get_cos_rc(cos_res)

    def get_cos_trans(self, cos_res):
        return get_cos_trans(cos_res)

    def generate_result(self, models: list, sound_id=2, isAdjust=False, isAdain=False, max_batch=64,
                        batch_families=False):
        """One (N, N, N) array per model: cos[source][target][k], the conversion source -> target of
        utterance `sound_id` scored by the judge against speaker k's d-vector.  batch_families: passed
        on to convert_grid (the Meta and AdaIN families batched too; `*_Adjust` stays pair by pair)."""
        from .embed import cos_scores

        if self.embedder is None:
            raise RuntimeError("generate_result needs a judge (config.embedder)")
        N = len(self.metadata)
        mels = [self._load(s, sound_id) for s in range(N)]
        lens = [m.shape[0] for m in mels]
        plans = plan_grid(lens, None, self.len_crop, np.random, tgt_lens=lens, copies=len(models))
        trans = [convert_grid(m, mels, self._emb(), len_crop=self.len_crop, max_batch=max_batch, targets=mels,
                              isAdjust=isAdjust, isAdain=isAdain, plan=p, device=self.device,
                              batch_families=batch_families)[0]
                 for m, p in zip(models, plans)]
        # the judge's draws in the reference's order: pair after pair, model after model
        flat = [trans[k][i] for i in range(N * N) for k in range(len(models))]
        cos = cos_scores(self._embed(flat), self._all_dv()).astype(np.float32)
        cos = cos.reshape(N, N, len(models), -1)
        cos_result = []
        for k in range(len(models)):
            res = np.zeros((self.num_speaker, self.num_speaker, self.num_speaker))
            res[:N, :N, :cos.shape[3]] = cos[:, :, k]
            cos_result.append(res)
        return cos_result


# ----------------------------------------------------------------------------- wav export
def write_wav(path, audio, sample_rate=SAMPLE_RATE):
    """float audio in [-1, 1] -> 16-bit PCM mono (the stdlib wave module)."""
    pcm = np.round(np.clip(np.asarray(audio, dtype=np.float64), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


@torch.no_grad()
def export_grid_wavs(vocoder, mels, pads, pairs, speakers, wav_dir, len_crop, max_batch=16):
    """generate.ipynb cell 8: <wav_dir>/<source speaker>/<source_id>_<target_id>.wav for every pair,
    the padded tail of the mel cut before vocoding (the isPlay=True call).  The vocoder runs batched
    over mels of equal length (MelVocoder.inverse_frames).  len_crop None: every mel at its own full length
    (the --whole export; pads is ignored), all pairs planned together into ragged batches
    (MelVocoder.inverse_ragged)."""
    written = []

    def write(i, wav):
        s, t = pairs[i]
        folder = os.path.join(wav_dir, str(speakers[s]))
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, f"{s}_{t}.wav")
        write_wav(path, wav)
        written.append(path)

    if len_crop is None:
        n = len(pads)
        for i, wav in enumerate(vocoder.inverse_ragged([mels[i] for i in range(n)], max_batch=max_batch)):
            write(i, wav.float().cpu().numpy())
        return written
    by_len = {}
    for i, pad in enumerate(pads):
        by_len.setdefault(len_crop - pad, []).append(i)
    for T, idx in sorted(by_len.items()):
        for k in range(0, len(idx), max_batch):
            part = idx[k:k + max_batch]
            x = torch.from_numpy(np.stack([mels[i][:T] for i in part])).to(vocoder.device)
            wav = vocoder.inverse_frames(x).float().cpu().numpy()
            for r, i in enumerate(part):
                write(i, wav[r])
    return written


# ----------------------------------------------------------------------------- CLI
class _Config:
    pass


def _parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m autoformer_amd.evaluate",
                                description="all-pairs conversion of a trained model: cosine summaries by a speaker "
                                            "judge (util/evaluate.py) and the grid as wavs (generate.ipynb)")
    p.add_argument("--root", required=True, help="folder of the mel tree (<root>/<speaker>/*.npy)")
    p.add_argument("--meta", default="test.pkl", help="metadata file under --root (make_metadata's list)")
    p.add_argument("--model", default="AutoVC", help="a factory plugin name")
    p.add_argument("--ckpt", help="the model's state_dict (torch.save); required unless --det_init")
    p.add_argument("--det_init", action="store_true", help="closed-form weights instead of checkpoints (smoke runs)")
    p.add_argument("--embedder", choices=["LstmDV", "MetaDV"], help="the judge; without one no scores are printed")
    p.add_argument("--embedder_ckpt", help="the judge's state_dict; required with --embedder unless --det_init")
    p.add_argument("--num_classes", type=int, default=256, help="MetaDV: classes of its checkpoint's head")
    p.add_argument("--wav_dir", help="write <wav_dir>/<source speaker>/<source_id>_<target_id>.wav")
    p.add_argument("--vocoder_ckpt", help="MelGAN generator state_dict; required with --wav_dir")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--len_crop", type=int, default=176)
    p.add_argument("--freq", type=int, default=22)
    p.add_argument("--num_speaker", type=int, default=40)
    p.add_argument("--erroment_num", type=int, default=16)
    p.add_argument("--max_uttr_idx", type=int, default=60)
    p.add_argument("--sound_id", type=int, default=2)
    p.add_argument("--max_batch", type=int, default=64)
    p.add_argument("--batch_families", action="store_true",
                   help="batch the MetaConv / MetaPool and AdaIN (*2) grids too, not AutoVC's alone (*_Adjust "
                        "stays pair by pair)")
    p.add_argument("--whole", action="store_true",
                   help="with --wav_dir: export every pair at the source's full length (convert.convert_whole, "
                        "AutoVC only) instead of one len_crop window")
    p.add_argument("--seed", type=int, help="seed numpy's and Python's random (the crop / enrolment draws)")
    return p


def _load_module(factory_name, args_, ckpt, det, device):
    import importlib

    cls = getattr(importlib.import_module(f"autoformer_amd.factory.{factory_name}"), factory_name)
    m = cls(*args_)
    if ckpt:
        m.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True))
    elif det:
        from .detinit import det_init_

        det_init_(m)
    return m.to(device)


def main(argv=None):
    args = _parser().parse_args(argv)
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    if not args.ckpt and not args.det_init:
        raise SystemExit("--ckpt FILE (the model's state_dict) is required unless --det_init is given")
    if args.embedder and not args.embedder_ckpt and not args.det_init:
        raise SystemExit("--embedder_ckpt FILE is required with --embedder unless --det_init is given")
    if args.wav_dir and not args.vocoder_ckpt:
        raise SystemExit("--wav_dir needs --vocoder_ckpt FILE (a MelGAN generator state_dict)")
    if args.whole and not args.wav_dir:
        raise SystemExit("--whole exports wavs: it needs --wav_dir")
    if not args.embedder and not args.wav_dir:
        raise SystemExit("nothing to do: give --embedder (scores) and / or --wav_dir (wavs)")
    import autoformer_amd as A

    A.set_compute(args.dtype)
    if args.seed is not None:
        np.random.seed(args.seed)
        random.seed(args.seed)
    with open(os.path.join(args.root, args.meta), "rb") as f:
        metadata = pickle.load(f)
    # the reference converts in train mode: BatchNorm on the utterance's own statistics
    model = _load_module(args.model, (44, 256, 512, args.freq), args.ckpt, args.det_init, args.device).train()
    cfg = _Config()
    cfg.root, cfg.batch_size, cfg.len_crop, cfg.device = args.root, 2, args.len_crop, args.device
    cfg.max_uttr_idx, cfg.erroment_num = args.max_uttr_idx, args.erroment_num
    cfg.all_speaker = sorted(str(d[0]) for d in metadata)[:args.num_speaker]
    cfg.num_speaker = len(cfg.all_speaker)
    cfg.metadata = metadata
    cfg.embedder = None
    if args.embedder:
        ctor = (args.num_classes,) if args.embedder == "MetaDV" else ()
        cfg.embedder = _load_module(args.embedder, ctor, args.embedder_ckpt, args.det_init, args.device).eval()
    cfg.vocoder = None
    if args.wav_dir:
        from .melgan import Generator, MelVocoder

        g = Generator(80, 32, 3)
        g.load_state_dict(torch.load(args.vocoder_ckpt, map_location="cpu", weights_only=True))
        cfg.vocoder = MelVocoder(device=args.device, generator=g)
    E = Evaluator(cfg)
    adjust, adain = args.model.endswith("_Adjust"), args.model.endswith("2")
    if args.embedder:
        cos = E.generate_result([model], args.sound_id, adjust, adain, max_batch=args.max_batch,
                                batch_families=args.batch_families)[0]
        rc, rc_other = E.get_cos_rc(cos)
        tr, tr_other = E.get_cos_trans(cos)
        print(f"reconstruction: cos to own speaker {rc:.4f}, to the others {rc_other:.4f}")
        print(f"conversion: cos to the target speaker {tr:.4f}, to the others {tr_other:.4f}")
    if args.wav_dir:
        N = len(E.metadata)
        mels = [E._load(s, args.sound_id) for s in range(N)]
        if args.whole:
            from .convert import convert_whole

            pairs, emb = all_pairs(N), E._emb()
            trans = convert_whole(model, [mels[s] for s, _ in pairs], emb[[s for s, _ in pairs]],
                                  emb[[t for _, t in pairs]], max_batch=args.max_batch, device=args.device)
            written = export_grid_wavs(E.vocoder, trans, [0] * len(pairs), pairs, [d[0] for d in E.metadata],
                                       args.wav_dir, None)
            print(f"{args.wav_dir}: {len(written)} wavs")
            return 0
        trans, pads = convert_grid(model, mels, E._emb(), len_crop=args.len_crop, max_batch=args.max_batch,
                                   targets=mels, isAdjust=adjust, isAdain=adain, device=args.device,
                                   batch_families=args.batch_families)
        written = export_grid_wavs(E.vocoder, trans, pads, all_pairs(N), [d[0] for d in E.metadata], args.wav_dir,
                                   args.len_crop)
        print(f"{args.wav_dir}: {len(written)} wavs")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
