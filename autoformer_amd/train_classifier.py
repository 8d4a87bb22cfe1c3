"""Train the MetaDV speaker classifier (factory/MetaDV.py) with softmax cross-entropy (xent.py): the network the
GAN / StarGAN trainers take as their classifier C, and whose d-vectors `embed --embedder MetaDV` writes.

  UtteranceBatches(root, B, T)      B crops of T frames per batch with their speaker labels and window starts
  ClassifierStep(model, loss)       one step: forward, cross-entropy, backward, gradient clip, fused Adam
  validate(model, batches)          top-1 and mean loss over the held-out utterances, one fixed crop each

The classifier is closed-set: every speaker of the mel tree is a class (sorted order), and what is held out
for validation is every val_every-th utterance of each speaker, not speakers.  The loading runs on a
background thread (train_embedder.ReadAhead).

  python -m autoformer_amd.train_classifier --spmel DIR --out FILE [--batch 64] [--len_crop 176]
      [--num_iters N] [--lr 1e-4] [--smooth 0.0] [--val_every 10] [--eval_every K] [--eval_spmel DIR2]
      [--save_every K] [--log_every K] [--resume FILE] [--dtype bf16|fp32] [--device cuda:0] [--seed 0]
      [--det_init] [--deterministic]

FILE is torch.save(model.state_dict()): it loads into MetaDV(C) and into `embed --embedder MetaDV --num_classes
C --ckpt FILE` as it is.  FILE + ".speakers.json" lists the speakers in class order; FILE + ".state" holds what
--resume needs besides the weights: Adam's moments and step count, the sampler state, the iteration and a
digest of the weights it was written with.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import dist as D
from . import kernels as K
from .embed import _batch_cap
from .layers import join_side, prefetch_packs, set_grad_sink
from .train import FusedAdam
from .train_embedder import ReadAhead, _load_resume, _speaker_files, _weights_digest, verification_eer
from .xent import SoftmaxXent


# ------------------------------------------------------------------------- data
class UtteranceBatches:
    """An endless iterator of classification batches (x (B, T, 80) fp32, labels (B,) int64, lefts) from the
    mel tree `embed --spmel` reads (<root>/<speaker>/*.npy, each (T_i, 80)).

    The speakers in sorted order are the classes 0..C-1.  Each speaker's sorted utterance list is split by
    position: index % val_every == val_every - 1 is validation, the rest training.  Utterances shorter than
    T frames are then left out of both (how many is printed); a speaker left with no training utterance is
    an error.  A batch draws B times (speaker uniform, then utterance uniform among the speaker's training
    utterances, then the crop offset uniform over those that keep the crop inside the utterance), and after
    these the model's sample_count window starts, uniform in [0, T - crop_len] (one set per batch, as MetaDV
    draws them).  All draws come from a numpy.random.Generator of its own: the global numpy and `random`
    states are not touched, and state() / set_state() resume the sequence exactly.  `last` lists the draws
    of the latest batch, one (speaker, path, offset) per row; `train` and `val` are lists of (label, path)."""

    def __init__(self, root, B, T, val_every=10, seed=0, crop_len=128, sample_count=4):
        self.B, self.T, self.val_every = int(B), int(T), int(val_every)
        self.crop_len, self.sample_count = int(crop_len), int(sample_count)
        if self.B < 1:
            raise ValueError(f"UtteranceBatches: B = {B} rows per batch")
        if self.val_every < 2:
            raise ValueError(f"UtteranceBatches: val_every = {val_every} leaves nothing to train on (>= 2)")
        if self.T < self.crop_len or self.sample_count < 1:
            raise ValueError(f"UtteranceBatches: T = {T} frames is shorter than crop_len = {crop_len}")
        self.speakers, self.train, self.val, self._by_speaker, short = [], [], [], [], 0
        for label, (spk, files) in enumerate(_speaker_files(root)):
            self.speakers.append(spk)
            mine = []
            for i, f in enumerate(files):
                if np.load(f, mmap_mode="r").shape[0] < self.T:
                    short += 1
                elif i % self.val_every == self.val_every - 1:
                    self.val.append((label, f))
                else:
                    mine.append(f)
            if not mine:
                raise ValueError(f"{root}: speaker {spk} has no training utterance of at least {self.T} frames")
            self._by_speaker.append(mine)
            self.train += [(label, f) for f in mine]
        if not self.speakers:
            raise ValueError(f"{root}: no speaker folders")
        print(f"UtteranceBatches: {len(self.speakers)} speakers, {len(self.train)} training and {len(self.val)} "
              f"validation utterances, {short} left out (shorter than {self.T} frames)")
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.last = []

    def state(self):
        return json.dumps(self.rng.bit_generator.state)

    def set_state(self, state):
        self.rng.bit_generator.state = json.loads(state)

    def __iter__(self):
        return self

    def __next__(self):
        rng, T = self.rng, self.T
        x, labels, last = None, np.empty(self.B, dtype=np.int64), []
        for b in range(self.B):
            s = int(rng.integers(0, len(self.speakers)))
            files = self._by_speaker[s]
            path = files[int(rng.integers(0, len(files)))]
            mel = np.load(path, mmap_mode="r")
            off = int(rng.integers(0, mel.shape[0] - T + 1))
            if x is None:
                x = np.empty((self.B, T, mel.shape[1]), dtype=np.float32)
            x[b] = mel[off:off + T]
            labels[b] = s
            last.append((self.speakers[s], path, off))
        lefts = [int(v) for v in rng.integers(0, T - self.crop_len + 1, size=self.sample_count)]
        self.last = last
        return x, labels, lefts


# ------------------------------------------------------------------------- step
class ClassifierStep:
    """One classification step of a MetaDV: flat parameter and gradient buffers and the fused Adam, as
    train_embedder.EmbedderStep.  After the backward: the global-norm clip with torch's formula (coef =
    clamp(clip / (norm + 1e-6), max = 1), on the device, no host sync), then Adam.  The window starts are an
    argument of every step, so a step never draws from Python's `random`."""

    def __init__(self, model, loss, lr=1e-4, clip=3.0):
        self.model, self.loss_mod, self.clip = model, loss, float(clip)
        self.num_classes = model.metablock.output.out_features
        self.params, self.flat, self.gflat = D.flatten_params_(model)
        set_grad_sink(True)  # kernels accumulate straight into the flat gradient buffer
        self.opt = FusedAdam(self.flat, self.gflat, lr)
        self._fault = K.fault_word(self.flat.device)
        self._fault_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._fault_ev = None
        self._one = torch.ones((), device=self.flat.device)

    def _probe_fault(self):
        # as TrainStep: the word is read back asynchronously and checked at the next step
        if self._fault_ev is not None and self._fault_ev.query():
            K.raise_on_fault(self._fault_host.item())
        self._fault_host.copy_(self._fault, non_blocking=True)
        self._fault_ev = torch.cuda.Event()
        self._fault_ev.record()

    def check(self):
        """Raise DeviceFault if any kernel of the steps so far reported a fault (synchronises)."""
        torch.cuda.synchronize()
        K.raise_on_fault(self._fault.item())

    def step(self, x, labels, lefts):
        """x (B, T, 80) on the device; labels: a kernels.Labels, or host integers (checked against the
        model's classes here); lefts: the model's window starts.  Returns (loss, correct), device scalars."""
        K.require_device(x)
        if not isinstance(labels, K.Labels):
            labels = K.Labels(labels, self.num_classes, x.device)
        if labels.B != x.shape[0] or labels.C != self.num_classes:
            raise ValueError(f"ClassifierStep: {labels.B} labels for {labels.C} classes, x has {x.shape[0]} rows "
                             f"and the model {self.num_classes} classes")
        self.gflat.zero_()
        pred, _ = self.model(x, lefts=lefts)
        loss = self.loss_mod(pred, labels)
        loss.backward(self._one)
        join_side()  # weight-gradient GEMMs ran on the side stream
        with torch.no_grad():
            # the padding between the views is zero: the flat buffer's norm is the global norm
            coef = torch.clamp(self.clip / (torch.linalg.vector_norm(self.gflat) + 1e-6), max=1.0)
            self.gflat.mul_(coef)
            self.opt.step()
        prefetch_packs()
        self._probe_fault()
        return loss, self.loss_mod.correct


# ------------------------------------------------------------------------- validation
def centre_crop(mel, T):
    """The centre T frames of an utterance of at least T frames."""
    off = (mel.shape[0] - T) // 2
    return mel[off:off + T]


def even_lefts(T, crop_len, sample_count):
    """sample_count window starts spread evenly over [0, T - crop_len], both ends included."""
    if sample_count == 1:
        return [(T - crop_len) // 2]
    return [(s * (T - crop_len)) // (sample_count - 1) for s in range(sample_count)]


@torch.no_grad()
def validate(model, batches, max_batch=None):
    """(top-1 accuracy, mean loss, n) over batches.val: every validation utterance embedded once, at its
    centre T frames with the windows of even_lefts -- nothing is drawn.  Under no_grad, so the model's
    forward-only bf16 path runs where it admits the batch.  n = 0 gives (nan, nan, 0)."""
    n = len(batches.val)
    if n == 0:
        return float("nan"), float("nan"), 0
    dev = next(model.parameters()).device
    C = model.metablock.output.out_features
    lefts = even_lefts(batches.T, model.crop_len, model.metablock.sample_count)
    cap = _batch_cap(model, max_batch)
    hits = torch.zeros((), device=dev, dtype=torch.int64)
    total = torch.zeros((), device=dev, dtype=torch.float64)
    for k in range(0, n, cap):
        part = batches.val[k:k + cap]
        x = np.stack([centre_crop(np.load(f, mmap_mode="r"), batches.T) for _, f in part]).astype(np.float32)
        pred, _ = model(torch.from_numpy(x).to(dev), lefts=lefts)
        loss, _, correct = K.xent(pred, K.Labels([lab for lab, _ in part], C, dev), grads=False)
        hits += correct
        total += loss.double() * len(part)
    return hits.item() / n, total.item() / n, n


# ------------------------------------------------------------------------- CLI
def _parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m autoformer_amd.train_classifier",
                                description="train the MetaDV speaker classifier with softmax cross-entropy")
    p.add_argument("--spmel", required=True, help="folder with one sub-folder of (T, 80) .npy mels per speaker")
    p.add_argument("--out", required=True, help="checkpoint to write: the MetaDV state_dict (and OUT.state, "
                                                "OUT.speakers.json)")
    p.add_argument("--batch", type=int, default=64, help="B, crops per batch")
    p.add_argument("--len_crop", type=int, default=176, help="T, frames per crop")
    p.add_argument("--num_iters", type=int, default=100000)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--smooth", type=float, default=0.0, help="label smoothing in [0, 1)")
    p.add_argument("--val_every", type=int, default=10, help="every val_every-th utterance of a speaker is held out")
    p.add_argument("--eval_spmel", help="mel tree of held-out speakers for the d-vectors' verification EER")
    p.add_argument("--eval_every", type=int, default=1000)
    p.add_argument("--save_every", type=int, default=1000)
    p.add_argument("--log_every", type=int, default=10)
    p.add_argument("--resume", help="a checkpoint this tool wrote (FILE, FILE.state, FILE.speakers.json) to continue from")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--det_init", action="store_true", help="closed-form initial weights (smoke runs)")
    p.add_argument("--deterministic", action="store_true",
                   help="bitwise reproducible gradients (kernels.set_deterministic): slower weight-gradient GEMMs")
    return p


def _save(path, model, step, speakers, sampler_state, iteration):
    """FILE.speakers.json, FILE and FILE.state, each written under a temporary name and renamed into place;
    the state carries a digest of the weights it belongs to, so a pair torn by a kill between the renames is
    refused by --resume instead of continuing from weights and moments of different iterations."""
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    state = {"adam_m": step.opt.m.cpu(), "adam_v": step.opt.v.cpu(), "adam_state": step.opt.state.cpu(),
             "sampler": sampler_state, "iteration": int(iteration), "weights_sha256": _weights_digest(sd)}
    with open(path + ".speakers.json.tmp", "w") as f:
        json.dump(list(speakers), f)
    os.replace(path + ".speakers.json.tmp", path + ".speakers.json")
    for obj, dst in ((sd, path), (state, path + ".state")):
        torch.save(obj, dst + ".tmp")
        os.replace(dst + ".tmp", dst)


def _load_resume_classifier(path, speakers):
    """(state_dict, state) of a checkpoint this tool wrote; refuses a state that was not written with these
    weights (train_embedder._load_resume) and a class order other than `speakers`."""
    sd, state = _load_resume(path)
    with open(path + ".speakers.json") as f:
        saved = json.load(f)
    if list(saved) != list(speakers):
        raise SystemExit(f"--resume {path}: {path}.speakers.json lists {len(saved)} speakers that are not the "
                         f"{len(speakers)} of --spmel in the same order; the classes would not mean the same")
    return sd, state


def main(argv=None):
    args = _parser().parse_args(argv)
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    if not torch.cuda.is_available():
        raise SystemExit(f"--device {args.device}: no GPU is available, and the HIP kernels need one")
    import autoformer_amd as A
    from .factory.MetaDV import MetaDV

    A.set_compute(args.dtype)
    K.set_deterministic(args.deterministic)
    torch.manual_seed(args.seed)
    C = len(_speaker_files(args.spmel))  # every speaker folder is a class
    if C < 1:
        raise SystemExit(f"--spmel {args.spmel}: no speaker folders")
    model, loss = MetaDV(C), SoftmaxXent(args.smooth)
    batches = UtteranceBatches(args.spmel, args.batch, args.len_crop, args.val_every, args.seed, model.crop_len,
                               model.metablock.sample_count)
    state = None
    if args.resume:
        sd, state = _load_resume_classifier(args.resume, batches.speakers)
        model.load_state_dict(sd)
    elif args.det_init:
        from .detinit import det_init_

        det_init_(model)
    model.to(args.device).train()
    step = ClassifierStep(model, loss, lr=args.lr)
    start = 0
    if state is not None:
        step.opt.m.copy_(state["adam_m"])
        step.opt.v.copy_(state["adam_v"])
        step.opt.state.copy_(state["adam_state"])
        batches.set_state(state["sampler"])
        start = int(state["iteration"])
        print(f"resumed {args.resume} at iteration {start}")
    feed = ReadAhead(batches, count=args.num_iters - start)  # loading and cropping off the training thread
    for it in range(start, args.num_iters):
        x, labels, lefts = next(feed)
        val, correct = step.step(x.to(args.device, non_blocking=True), labels, lefts)
        done = it + 1
        if done % args.log_every == 0 or done == args.num_iters:
            print(f"[{done}/{args.num_iters}] xent {val.item():.4f}  top-1 {correct.item() / args.batch:.3f}")
        if done % args.eval_every == 0 or done == args.num_iters:
            top1, vloss, n = validate(model, batches)
            if n:
                print(f"[{done}/{args.num_iters}] validation top-1 {100 * top1:.2f} %  xent {vloss:.4f} ({n} utterances)")
            if args.eval_spmel:
                e, nt, nn_ = verification_eer(model, args.eval_spmel, len_crop=args.len_crop)
                print(f"[{done}/{args.num_iters}] EER {100 * e:.2f} % ({nt} target, {nn_} non-target trials)")
        if done % args.save_every == 0 and done != args.num_iters:
            _save(args.out, model, step, batches.speakers, feed.state, done)
    step.check()
    feed.close()
    _save(args.out, model, step, batches.speakers, feed.state, max(start, args.num_iters))
    print(f"{args.out}: MetaDV({C}) state_dict after {max(start, args.num_iters)} iterations (+ {args.out}.state, "
          f"{args.out}.speakers.json)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
