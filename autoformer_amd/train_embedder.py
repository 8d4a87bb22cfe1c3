"""Train the LstmDV speaker embedder (factory/LstmDV.py) with the GE2E loss (ge2e.py): the network whose
256-d embeddings embed.py, evaluate.py and convert.py consume through --ckpt / --embedder_ckpt.

  SpeakerBatches(root, N, M)        N speakers x M utterances per batch, one crop length per batch
  ReadAhead(batches, count)         the sampler on a background thread, with the state a checkpoint needs
  EmbedderStep(model, loss)         one step: forward, GE2E, backward, gradient scaling and clip, fused Adam
  eer(targets, nontargets)          the equal-error rate of two score sets (host side)
  verification_eer(model, root)     enrol / trial verification on a mel tree of held-out speakers

Recipe (Wan et al. 2018, section 3): utterance partials of 140..180 frames, one length per batch; the
gradient of the loss scale w is multiplied by 0.01, that of the projection (LstmDV.embedding) by 0.5, and
the global gradient norm is clipped to 3.  The optimiser is the project's fused Adam at lr 1e-4.

  python -m autoformer_amd.train_embedder --spmel DIR --out FILE [--speakers 64] [--utterances 10]
      [--partial 140 180] [--num_iters N] [--lr 1e-4] [--eval_spmel DIR2 --eval_every K] [--save_every K]
      [--resume FILE] [--dtype bf16|fp32] [--device cuda:0] [--seed 0] [--det_init] [--deterministic]

FILE is torch.save(model.state_dict()): it loads into LstmDV() and into `embed --ckpt`, `evaluate
--embedder_ckpt` and `convert --embedder_ckpt` as it is.  FILE + ".state" holds what --resume needs besides
the weights: w, Adam's moments and step count, the sampler state and the iteration.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import dist as D
from . import kernels as K
from .embed import cos_scores, embed_utterances, speaker_dvector
from .ge2e import GE2ELoss
from .layers import join_side, prefetch_packs, set_grad_sink
from .train import FusedAdam


# ------------------------------------------------------------------------- data
def _speaker_files(root):
    """[(speaker, [npy paths, sorted])] of the mel tree <root>/<speaker>/*.npy, speakers sorted."""
    out = []
    for spk in sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))):
        files = sorted(f for f in os.listdir(os.path.join(root, spk)) if f.endswith(".npy"))
        out.append((spk, [os.path.join(root, spk, f) for f in files]))
    return out


class SpeakerBatches:
    """An endless iterator of GE2E batches x (N*M, T, 80) fp32, speaker-major, from the mel tree
    `embed --spmel` reads (<root>/<speaker>/*.npy, each (T_i, 80)).

    Utterances shorter than partial[1] frames are left out (every crop length must fit every utterance),
    then speakers with fewer than M utterances; how many speakers that cost is printed.  Fewer than N
    speakers left is an error.  A batch draws, in this order, one length T uniform in [partial[0],
    partial[1]], N distinct speakers, and per speaker M distinct utterances and then one crop offset for
    each, uniform over the offsets that keep the crop inside the utterance.  All draws come from a
    numpy.random.Generator of its own: the global numpy and `random` states are not touched, and state() /
    set_state() resume the sequence exactly.  `last` lists the draws of the latest batch, one (speaker,
    path, offset) per row.  It yields x alone; zip it with a constant to feed data.DeviceFeed, which
    takes pairs; ReadAhead below is the trainer's own read-ahead, which keeps the state a checkpoint needs."""

    def __init__(self, root, N, M, partial=(140, 180), seed=0):
        self.N, self.M = int(N), int(M)
        self.lo, self.hi = int(partial[0]), int(partial[1])
        if self.N < 2 or self.M < 2:
            raise ValueError(f"SpeakerBatches: GE2E needs N >= 2 speakers and M >= 2 utterances, got {N}, {M}")
        if not 1 <= self.lo <= self.hi:
            raise ValueError(f"SpeakerBatches: partial = {tuple(partial)} is not 1 <= lo <= hi")
        self.speakers, thin = [], 0
        for spk, files in _speaker_files(root):
            keep = [f for f in files if np.load(f, mmap_mode="r").shape[0] >= self.hi]
            if len(keep) >= self.M:
                self.speakers.append((spk, keep))
            else:
                thin += 1
        print(f"SpeakerBatches: {len(self.speakers)} speakers, {thin} left out (fewer than {self.M} utterances of "
              f"at least {self.hi} frames)")
        if len(self.speakers) < self.N:
            raise ValueError(f"{root}: {len(self.speakers)} usable speakers, a batch needs N = {self.N}")
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.last = []

    def state(self):
        return json.dumps(self.rng.bit_generator.state)

    def set_state(self, state):
        self.rng.bit_generator.state = json.loads(state)

    def __iter__(self):
        return self

    def __next__(self):
        rng = self.rng
        T = int(rng.integers(self.lo, self.hi + 1))
        x, last = None, []
        for n, s in enumerate(rng.choice(len(self.speakers), self.N, replace=False)):
            spk, files = self.speakers[int(s)]
            picks = rng.choice(len(files), self.M, replace=False)
            mels = [np.load(files[int(u)], mmap_mode="r") for u in picks]
            for m, (u, mel) in enumerate(zip(picks, mels)):
                off = int(rng.integers(0, mel.shape[0] - T + 1))
                if x is None:
                    x = np.empty((self.N * self.M, T, mel.shape[1]), dtype=np.float32)
                x[n * self.M + m] = mel[off:off + T]
                last.append((spk, files[int(u)], off))
        self.last = last
        return x


class ReadAhead:
    """next(batches) on a background thread, up to `depth` batches ahead of the consumer: the N*M loads and
    crops of a batch overlap the device's work on the one before.  Yields host tensors (pinned where a
    device is there, so the consumer's copy can be non_blocking; each batch has a buffer of its own).
    `state` is the sampler state after the batch handed out last -- what a checkpoint must hold, not the
    state of the sampler itself, which is `depth` draws further on.  `count` batches are produced in all.
    A sampler that yields a tuple (x, ...) gets (tensor of x, ...) back: only x is converted and pinned."""

    def __init__(self, batches, count, depth=2, pin=None):
        import queue
        import threading

        self.state = batches.state()
        self._q, self._stop = queue.Queue(maxsize=depth), threading.Event()
        pin = torch.cuda.is_available() if pin is None else pin

        def put(item):
            while not self._stop.is_set():
                try:
                    return self._q.put(item, timeout=0.1)
                except queue.Full:
                    pass

        def produce():
            try:
                for _ in range(max(count, 0)):
                    if self._stop.is_set():
                        return
                    item = next(batches)
                    rest = ()
                    if isinstance(item, tuple):  # (x, ...): x as below, the rest handed through as it is
                        item, rest = item[0], item[1:]
                    x = torch.from_numpy(item)
                    x = x.pin_memory() if pin else x
                    put(((x,) + rest if rest else x, batches.state()))
            except BaseException as exc:  # surface loader errors in the consumer
                put(exc)
        self._thread = threading.Thread(target=produce, daemon=True)
        self._thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        item = self._q.get()
        if isinstance(item, BaseException):
            raise item
        x, self.state = item
        return x

    def close(self):
        self._stop.set()
        self._thread.join()


# ------------------------------------------------------------------------- step
class EmbedderStep:
    """One GE2E training step of an LstmDV: flat parameter and gradient buffers over [model, loss] and the
    fused Adam, as train.TrainStep.  After the backward, in this order: w.grad *= w_grad_scale, the
    projection's gradients *= proj_grad_scale, the global-norm clip with torch's formula (coef =
    clamp(clip / (norm + 1e-6), max = 1), on the device, no host sync), Adam; then w is clamped to >= 1e-6.

    In bf16 mode a batch the persistent recurrence does not admit in one launch (forward and backward) goes
    through the model in sub-batches of the largest admitted size inside the one autograd graph -- rows are
    independent, and in sink mode the weight gradients accumulate; `path` says what the last step did."""

    def __init__(self, model, loss, lr=1e-4, clip=3.0, w_grad_scale=0.01, proj_grad_scale=0.5):
        self.model, self.loss_mod = model, loss
        self.clip, self.w_grad_scale, self.proj_grad_scale = float(clip), float(w_grad_scale), float(proj_grad_scale)
        self.owner = torch.nn.ModuleList([model, loss])
        self.params, self.flat, self.gflat = D.flatten_params_(self.owner)
        set_grad_sink(True)  # kernels accumulate straight into the flat gradient buffer
        self.opt = FusedAdam(self.flat, self.gflat, lr)
        self._fault = K.fault_word(self.flat.device)
        self._fault_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._fault_ev = None
        self._one = torch.ones((), device=self.flat.device)
        self._cap = {}
        self.path = None

    def sub_batch(self, B):
        """The rows per pass through the model for a batch of B: B itself where no persistent recurrence
        is in play (fp32 mode, another cell size) or it admits B, else the largest batch it admits."""
        key = (B, K.compute())
        if key not in self._cap:
            H = self.model.lstm.hidden_size

            def ok(b):
                return K.lstm_persistent_fwd(b, H, 1) and K.lstm_persistent_bwd(b, H, 1)
            cap = B
            if K.compute() == K.BF16 and ok(1) and not ok(B):
                # a scan, once per batch size: it does not assume that the admitted sizes form a prefix, and
                # the size it returns was itself admitted (ok(1) ends it)
                cap = next(b for b in range(B - 1, 0, -1) if ok(b))
            self._cap[key] = cap
        return self._cap[key]

    def embed(self, x):
        B = x.shape[0]
        cap = self.sub_batch(B)
        if cap >= B:
            self.path = f"one pass (B = {B})"
            return self.model(x)
        self.path = f"{-(-B // cap)} sub-batches of at most {cap} rows (B = {B})"
        return torch.cat([self.model(x[i:i + cap]) for i in range(0, B, cap)])

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

    def step(self, x, N, M):
        """x (N*M, T, 80) on the device, speaker-major; returns the loss (a device scalar)."""
        K.require_device(x)
        if x.shape[0] != N * M:
            raise ValueError(f"EmbedderStep: x has {x.shape[0]} rows, N*M = {N * M}")
        self.gflat.zero_()
        loss = self.loss_mod(self.embed(x), N, M)
        loss.backward(self._one)
        join_side()  # weight-gradient GEMMs ran on the side stream
        with torch.no_grad():
            self.loss_mod.w.grad.mul_(self.w_grad_scale)
            self.model.embedding.weight.grad.mul_(self.proj_grad_scale)
            self.model.embedding.bias.grad.mul_(self.proj_grad_scale)
            # the padding between the views is zero: the flat buffer's norm is the global norm
            coef = torch.clamp(self.clip / (torch.linalg.vector_norm(self.gflat) + 1e-6), max=1.0)
            self.gflat.mul_(coef)
            self.opt.step()
            self.loss_mod.w.clamp_(min=1e-6)
        prefetch_packs()
        self._probe_fault()
        return loss


# ------------------------------------------------------------------------- verification
def eer(target_scores, nontarget_scores):
    """The equal-error rate.  At every distinct score t, FAR(t) is the share of non-targets >= t and FRR(t)
    the share of targets < t; the EER is where FAR = FRR on the piecewise-linear curve through those
    (FAR, FRR) points plus (1, 0) and (0, 1)."""
    tg = np.asarray(target_scores, dtype=np.float64).ravel()
    nt = np.asarray(nontarget_scores, dtype=np.float64).ravel()
    if tg.size == 0 or nt.size == 0:
        raise ValueError(f"eer: {tg.size} target and {nt.size} non-target scores; both sets must be non-empty")
    thr = np.unique(np.concatenate([tg, nt]))  # ascending: FAR falls, FRR rises
    tg, nt = np.sort(tg), np.sort(nt)
    far = np.concatenate([[1.0], 1.0 - np.searchsorted(nt, thr, side="left") / nt.size, [0.0]])
    frr = np.concatenate([[0.0], np.searchsorted(tg, thr, side="left") / tg.size, [1.0]])
    d = far - frr
    i = int(np.argmax(d <= 0.0))  # d runs from 1 down to -1: the first point at or past the crossing
    if d[i] == 0.0:
        return float(far[i])
    s = d[i - 1] / (d[i - 1] - d[i])
    return float(far[i - 1] + s * (far[i] - far[i - 1]))


def verification_eer(model, root, enrol=5, len_crop=176):
    """(eer, n_target, n_nontarget) of the mel tree `root`: speakers in sorted order; the first `enrol`
    utterances of each (sorted) make its enrolment vector (embed.speaker_dvector); every other utterance
    is a trial against every speaker's enrolment, scored with embed.cos_scores."""
    enrolled, trials, owner = [], [], []
    for k, (spk, files) in enumerate(_speaker_files(root)):
        if len(files) < enrol:
            raise ValueError(f"speaker {spk}: {len(files)} utterances, enrol = {enrol}")
        mels = [np.load(f) for f in files]
        enrolled.append(speaker_dvector(model, mels[:enrol], len_crop))
        if len(mels) > enrol:
            trials.append(embed_utterances(model, mels[enrol:], len_crop))
            owner += [k] * (len(mels) - enrol)
    if not trials or len(enrolled) < 2:
        raise ValueError(f"{root}: verification needs two speakers and an utterance beyond the {enrol} enrolled")
    scores = cos_scores(np.concatenate(trials), np.stack(enrolled))  # (trials, speakers)
    target = np.asarray(owner)[:, None] == np.arange(len(enrolled))[None, :]
    return eer(scores[target], scores[~target]), int(target.sum()), int((~target).sum())


# ------------------------------------------------------------------------- CLI
def _parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m autoformer_amd.train_embedder",
                                description="train the LstmDV speaker embedder with the GE2E loss")
    p.add_argument("--spmel", required=True, help="folder with one sub-folder of (T, 80) .npy mels per speaker")
    p.add_argument("--out", required=True, help="checkpoint to write: the LstmDV state_dict (and OUT.state)")
    p.add_argument("--speakers", type=int, default=64, help="N, speakers per batch")
    p.add_argument("--utterances", type=int, default=10, help="M, utterances per speaker")
    p.add_argument("--partial", type=int, nargs=2, default=(140, 180), metavar=("LO", "HI"),
                   help="crop length range in frames, one length per batch")
    p.add_argument("--num_iters", type=int, default=100000)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--eval_spmel", help="mel tree of held-out speakers for the verification EER")
    p.add_argument("--eval_every", type=int, default=1000)
    p.add_argument("--save_every", type=int, default=1000)
    p.add_argument("--log_every", type=int, default=10)
    p.add_argument("--resume", help="a checkpoint this tool wrote (FILE and FILE.state) to continue from")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--det_init", action="store_true", help="closed-form initial weights (smoke runs)")
    p.add_argument("--deterministic", action="store_true",
                   help="bitwise reproducible gradients (kernels.set_deterministic): slower weight-gradient GEMMs")
    return p


def _weights_digest(sd):
    """sha256 over the state_dict's tensors in key order: ties FILE.state to the FILE it was written beside."""
    import hashlib

    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _save(path, model, loss, step, sampler_state, iteration):
    """FILE and FILE.state, each written under a temporary name and renamed into place; the state carries a
    digest of the weights it belongs to, so a pair torn by a kill between the two renames is refused by
    --resume instead of continuing from weights and moments of different iterations."""
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    state = {"w": loss.w.detach().cpu().clone(), "adam_m": step.opt.m.cpu(), "adam_v": step.opt.v.cpu(),
             "adam_state": step.opt.state.cpu(), "sampler": sampler_state, "iteration": int(iteration),
             "weights_sha256": _weights_digest(sd)}
    for obj, dst in ((sd, path), (state, path + ".state")):
        torch.save(obj, dst + ".tmp")
        os.replace(dst + ".tmp", dst)


def _load_resume(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    state = torch.load(path + ".state", map_location="cpu", weights_only=True)
    if state.get("weights_sha256") != _weights_digest(sd):
        raise SystemExit(f"--resume {path}: {path}.state was not written with these weights (a save was interrupted "
                         "between the two files); it cannot be continued from")
    return sd, state


def main(argv=None):
    args = _parser().parse_args(argv)
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    if not torch.cuda.is_available():
        raise SystemExit(f"--device {args.device}: no GPU is available, and the HIP kernels need one")
    import autoformer_amd as A
    from .factory.LstmDV import LstmDV

    A.set_compute(args.dtype)
    K.set_deterministic(args.deterministic)
    torch.manual_seed(args.seed)
    model, loss = LstmDV(), GE2ELoss()
    state = None
    if args.resume:
        sd, state = _load_resume(args.resume)
        model.load_state_dict(sd)
        with torch.no_grad():
            loss.w.copy_(state["w"])
    elif args.det_init:
        from .detinit import det_init_

        det_init_(model)
    model.to(args.device).train()
    loss.to(args.device)
    N, M = args.speakers, args.utterances
    batches = SpeakerBatches(args.spmel, N, M, tuple(args.partial), args.seed)
    step = EmbedderStep(model, loss, lr=args.lr)
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
        x = next(feed).to(args.device, non_blocking=True)
        val = step.step(x, N, M)
        done = it + 1
        if it == start:
            print(f"N = {N}, M = {M}, T = {x.shape[1]}: {step.path}")
        if done % args.log_every == 0 or done == args.num_iters:
            print(f"[{done}/{args.num_iters}] ge2e {val.item():.4f}  w {loss.w.item():.4f}")
        if args.eval_spmel and (done % args.eval_every == 0 or done == args.num_iters):
            e, nt, nn_ = verification_eer(model, args.eval_spmel)
            print(f"[{done}/{args.num_iters}] EER {100 * e:.2f} % ({nt} target, {nn_} non-target trials)")
        if done % args.save_every == 0 and done != args.num_iters:
            _save(args.out, model, loss, step, feed.state, done)
    step.check()
    feed.close()
    _save(args.out, model, loss, step, feed.state, max(start, args.num_iters))
    print(f"{args.out}: LstmDV state_dict after {max(start, args.num_iters)} iterations (+ {args.out}.state)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
