"""The GAN trainer: train_with_gan_ver1.py (:15-288) over the HIP kernels -- a VC model, the MetaDV classifier C
that reads the style of the converted mel, and the Discriminator D that tells it from a real one.

  critic_due(i, n_critic, pretrained_step)    whether iteration i (from 0) is a critic iteration
  CriticStep(VC, C, Dm)                       the two kinds of iteration: vc_step and critic_step
  GanVer1Solver(loader, config)               the reference's Solver: module loading, the loop, the log line

Every iteration computes the VC loss of train.py (identity pass, encoder re-pass, two MSEs and the code L1).  A
critic iteration ((i + 1) % n_critic == 0 and (i + 1) > pretrained_step) draws a second batch (x_target,
target_style), converts the source to the target style, and adds

    lambda_cls * cosine_embedding_loss(C(x_conv).d_vec, target_style, 1) + lambda_dis * (BCE(D(x_target), 1) +
    BCE(D(x_conv), 0))

to it (critic.critic_loss_block: the whole tail, with its addition to the VC loss, in one launch and one more for
its backward); ONE backward, then all three Adams step -- C and D descend the same loss as VC, as in the
reference.  Any other iteration steps VC alone: C's and D's parameters and Adam state stay as they are.

  python -m autoformer_amd.train_gan --model_name AutoVC (--data_dir DIR | --synthetic) --classifier_ckpt FILE
      [--save_model_name NAME] [--use_adain 1] [--num_iters 10] [--n_critic 10] [--pretrained_step K]
      [--lambda_cls 0.1] [--lambda_dis 1] [--batch_size 2] [--dtype fp32|bf16] [--seed 1234] [--det_init]
      [--log_step 10] [--num_speaker C] [--device cuda:0]

FILE is what train_classifier writes (a MetaDV state_dict); NAME.pt receives VC's state_dict as the reference
saves it, NAME.C.pt and NAME.D.pt the classifier's and the discriminator's.
"""
from __future__ import annotations

import datetime
import importlib
import time

import torch

from . import dist as D
from . import kernels as K
from .critic import critic_loss_block
from .layers import join_side, prefetch_packs, set_grad_sink, weights_changed
from .train import FusedAdam, Solver, SyntheticUtterances, losses_for

DISC_LEN_CROP = 176  # factory/Discriminator.py: conv1 takes the crop's frames as channels, dense1 1628 inputs
LOG_KEYS = ["VC/loss_id", "VC/loss_id_psnt", "VC/loss_cd", "C/loss_trans", "D/loss"]


def critic_due(i, n_critic, pretrained_step):
    """train_with_gan_ver1.py:139 for the iteration counted from 0 (host only)."""
    return (i + 1) % n_critic == 0 and (i + 1) > pretrained_step


# ------------------------------------------------------------------------- step
class CriticStep:
    """The two iterations of train_with_gan_ver1.py:116-176 over three flat parameter / gradient buffers and
    three fused Adams (VC, C, D), in gradient-sink mode: the weight-gradient kernels add straight into the flat
    gradient buffers, so the decoder and postnet, which run twice inside a critic step's graph, end up with the
    sum of both passes.  There is no decoder-done hook, no early Adam slice and no recorded replay here: with two
    decoder passes in one graph the decoder gradients are not final when the first pass's backward is through."""

    def __init__(self, VC, C, Dm, lr=1e-4, lambda_cd=1, lambda_cls=0.1, lambda_dis=1, use_adain=False):
        from .factory._variants import AdaINModel, AdjustModel

        if isinstance(VC, AdjustModel):
            raise ValueError("CriticStep: the *_Adjust models return four outputs; train_with_gan_ver1.py has no step "
                             "for them")
        if bool(use_adain) != isinstance(VC, AdaINModel):
            raise ValueError(f"CriticStep: use_adain = {bool(use_adain)} with a {type(VC).__name__}: the AdaIN variants "
                             "(AutoVC2, MetaConv2, MetaPool2) need use_adain, the plain families must not have it")
        self.VC, self.C, self.D = VC, C, Dm
        self.use_adain = bool(use_adain)
        self.lambda_cd, self.lambda_cls, self.lambda_dis = float(lambda_cd), float(lambda_cls), float(lambda_dis)
        (_, self.vc_flat, self.vc_gflat), (_, self.c_flat, self.c_gflat), (_, self.d_flat, self.d_gflat) = (
            D.flatten_params_(m) for m in (VC, C, Dm))
        set_grad_sink(True)  # kernels accumulate straight into the flat gradient buffers
        self.vc_opt = FusedAdam(self.vc_flat, self.vc_gflat, lr)
        self.c_opt = FusedAdam(self.c_flat, self.c_gflat, lr)
        self.d_opt = FusedAdam(self.d_flat, self.d_gflat, lr)
        self.loss_fn = losses_for(VC)
        dev = self.vc_flat.device
        self._fault = K.fault_word(dev)
        self._fault_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._fault_ev = None
        self._one = torch.ones((), device=dev)

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

    def _zero(self):
        self.vc_gflat.zero_()
        self.c_gflat.zero_()
        self.d_gflat.zero_()

    def _finish(self, total, opts):
        total.backward(self._one)
        join_side()  # weight-gradient GEMMs ran on the side stream: before any Adam reads a gradient
        for opt in opts:
            opt.step()
        prefetch_packs()
        self._probe_fault()

    def vc_step(self, x, emb):
        """The non-critic iteration (train_with_gan_ver1.py:122-137, :173-176): x (B, T, 80), emb (B, 256) on the
        device.  Returns (l_id, l_id_psnt, l_cd), device scalars."""
        K.require_device(x, emb)
        self._zero()
        self.VC._decoder_bwd_done = None
        total, parts, _ = self.loss_fn(self.VC, x, emb, self.lambda_cd)
        self._finish(total, (self.vc_opt,))
        return parts

    def critic_step(self, x, emb, x_target, emb_target, lefts):
        """The critic iteration (train_with_gan_ver1.py:122-171).  lefts: C's window starts (C.draw_lefts(T)), an
        argument so that a step never draws from Python's `random`.  The forward calls, in the order that moves
        the BatchNorm running statistics: VC identity, encoder re-pass, (AdaIN: the target's feature pass,) VC
        conversion, D real, D fake.  Returns (l_id, l_id_psnt, l_cd, c_loss, d_loss), device scalars."""
        K.require_device(x, emb, x_target, emb_target)
        self._zero()
        VC = self.VC
        VC._decoder_bwd_done = None
        vc_total, parts, x_psnt = self.loss_fn(VC, x, emb, self.lambda_cd)
        if self.use_adain:
            _, target_feature = VC(x_psnt, emb_target, None)
            _, x_conv, _ = VC(x, emb, emb_target, target_feature)
        else:
            _, x_conv, _ = VC(x, emb, emb_target)
        x_conv = x_conv.squeeze(1)
        _, trans_style = self.C(x_conv, lefts=lefts)
        real = self.D(x_target)
        fake = self.D(x_conv)
        total, c_loss, d_loss = critic_loss_block(trans_style, emb_target, real, fake, self.lambda_cls,
                                                  self.lambda_dis, base=vc_total)
        self._finish(total, (self.vc_opt, self.c_opt, self.d_opt))
        return (*parts, c_loss, d_loss)


# ------------------------------------------------------------------------- solver
class Config:
    """train_with_gan_ver1.py:220-239."""

    def __init__(self, model_name, data_dir, use_adain, num_iters):
        self.model_name = model_name
        self.data_dir = data_dir
        self.num_iters = num_iters
        self.pretrained_step = int(num_iters / 10)
        self.use_adain = use_adain
        self.num_speaker = 80
        self.lambda_cd = 1
        self.lambda_ad = 0.1  # unused there as here
        self.lambda_cls = 0.1
        self.lambda_dis = 1
        self.n_critic = 10
        self.batch_size = 2
        self.len_crop = 176
        self.dim_neck = 44
        self.dim_emb = 256
        self.dim_pre = 512
        self.freq = 22
        self.log_step = 10
        # the build's: where the modules live, C's checkpoint (the reference hard-wires model/static/metadv_vctk80.pth)
        self.device = "cuda:0"
        self.classifier_ckpt = None


def load_classifier_state(path):
    """The MetaDV state_dict of a train_classifier checkpoint (or any plain MetaDV state_dict), on the host."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or "metablock.output.weight" not in sd:
        raise SystemExit(f"--classifier_ckpt {path}: not a MetaDV state_dict (no metablock.output.weight)")
    return sd


class GanVer1Solver(Solver):
    """Mirror of train_with_gan_ver1.py:Solver (:15-217) on the HIP models: CriticStep does the iterations.
    C is loaded from config.classifier_ckpt when given (its class count from the checkpoint's output layer unless
    config.num_speaker says otherwise).  The second batch of a critic iteration is the loader's next batch.  The
    log line carries the reference's five keys; C/loss_trans and D/loss show the latest critic iteration's values,
    0.0 before the first (the reference reads stale variables there, and raises NameError before the first).  The
    line is printed at every log_step, with one format; the reference has two branches for it
    (train_with_gan_ver1.py:178, :198), split at pretrained_step, which print the same keys."""

    def __init__(self, vcc_loader, config):
        self.lambda_cls, self.lambda_dis = config.lambda_cls, config.lambda_dis
        self.n_critic, self.pretrained_step = config.n_critic, config.pretrained_step
        self.num_speaker = getattr(config, "num_speaker", None)
        self.use_adain = bool(config.use_adain)
        self.classifier_ckpt = getattr(config, "classifier_ckpt", None)
        self.log_keys = list(LOG_KEYS)
        super().__init__(vcc_loader, config)

    def build_model(self):
        from .factory.Discriminator import Discriminator
        from .factory.MetaDV import MetaDV

        self.VC = getattr(importlib.import_module(f"autoformer_amd.factory.{self.model_name}"), self.model_name)(
            self.dim_neck, self.dim_emb, self.dim_pre, self.freq)
        sd = None
        if self.classifier_ckpt:
            print(f"Load Pretrained Embedder from --- {self.classifier_ckpt}")
            sd = load_classifier_state(self.classifier_ckpt)
            rows = sd["metablock.output.weight"].shape[0]
            if self.num_speaker is None:
                self.num_speaker = rows
            elif self.num_speaker != rows:
                raise SystemExit(f"--classifier_ckpt {self.classifier_ckpt} has {rows} classes, num_speaker is "
                                 f"{self.num_speaker}")
        if self.num_speaker is None:
            self.num_speaker = 80
        self.C = MetaDV(self.num_speaker)
        if sd is not None:
            self.C.load_state_dict(sd)
        self.D = Discriminator()
        for m in (self.VC, self.C, self.D):
            m.to(self.device)
        self.step = self.make_step()
        self.vc_optimizer, self.c_optimizer, self.d_optimizer = self.step.vc_opt, self.step.c_opt, self.step.d_opt

    def make_step(self):
        """The step object over the three modules (a subclass with another kind of iteration overrides it)."""
        return CriticStep(self.VC, self.C, self.D, 0.0001, self.lambda_cd, self.lambda_cls, self.lambda_dis,
                          self.use_adain)

    def critic_iteration(self, x_source, org_style):
        """A critic iteration: draws the second batch and C's window starts; returns the VC loss's three parts
        followed by the critic-only values, in log_keys' order."""
        x_target, target_style = self.get_data()
        lefts = self.C.draw_lefts(x_source.shape[-2])
        return self.step.critic_step(x_source, org_style, x_target, target_style, lefts)

    def reset_grad(self):
        self.vc_optimizer.zero_grad()
        self.c_optimizer.zero_grad()
        self.d_optimizer.zero_grad()

    def get_data(self):
        """The loader's next batch on the device; a loader that runs out is started again."""
        if self._data_iter is None:
            self._data_iter = iter(self.vcc_loader)
        try:
            x, style = next(self._data_iter)
        except StopIteration:
            self._data_iter = iter(self.vcc_loader)
            x, style = next(self._data_iter)
        return x.to(self.device), style.to(self.device)

    def print_log(self, loss, i, start_time):
        et = str(datetime.timedelta(seconds=time.time() - start_time))[:-7]
        log = "Elapsed [{}], Iteration [{}/{}]".format(et, i + 1, self.num_iters)
        for tag in self.log_keys:
            log += ", {}: {:.4f}".format(tag, loss[tag])
        print(log)

    def train(self):
        """The loop; returns the logged values of every iteration (read from the device once, at the end)."""
        print("Start training...")
        start_time = time.time()
        self._data_iter = None
        zero = torch.zeros((), device=self.device)
        last = [zero] * (len(self.log_keys) - 3)
        rows = []
        for i in range(self.num_iters):
            x_source, org_style = self.get_data()
            self.VC, self.C, self.D = self.VC.train(), self.C.train(), self.D.train()
            if critic_due(i, self.n_critic, self.pretrained_step):
                out = self.critic_iteration(x_source, org_style)
                parts, last = out[:3], list(out[3:])
            else:
                parts = self.step.vc_step(x_source, org_style)
            rows.append(torch.stack([*parts, *last]))
            if (i + 1) % self.log_step == 0:
                loss = dict(zip(self.log_keys, rows[-1].tolist()))
                K.check_faults(zero.device)
                self.print_log(loss, i, start_time)
        self.step.check()
        return torch.stack(rows).tolist() if rows else []


# ------------------------------------------------------------------------- command line
def build_parser():
    import argparse

    p = argparse.ArgumentParser(
        prog="python -m autoformer_amd.train_gan",
        description="train_with_gan_ver1.py on the MI355X: a VC model with the MetaDV classifier and the "
                    "Discriminator as its critics, over the HIP kernels.")
    # the reference's flags (train_with_gan_ver1.py:243-249)
    p.add_argument("--model_name", default="AutoVC", help="traning model name (a factory plugin)")
    p.add_argument("--data_dir", help="traning data folder (train.pkl + mel .npy files)")
    p.add_argument("--save_model_name")
    p.add_argument("--use_adain", default=False)
    p.add_argument("--num_iters", default=10, help="iter time")
    # the build's flags
    p.add_argument("--classifier_ckpt", help="the MetaDV state_dict train_classifier wrote (required unless --det_init)")
    p.add_argument("--num_speaker", type=int, default=None,
                   help="C's classes (default: the checkpoint's; 80 without a checkpoint)")
    p.add_argument("--n_critic", type=int, default=10)
    p.add_argument("--pretrained_step", type=int, default=None, help="default int(num_iters / 10)")
    p.add_argument("--lambda_cls", type=float, default=0.1)
    p.add_argument("--lambda_dis", type=float, default=1)
    p.add_argument("--batch_size", type=int, default=2)
    p.add_argument("--len_crop", type=int, default=176)
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32",
                   help="compute precision of the HIP kernels (fp32: the reference's arithmetic)")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--synthetic", action="store_true", help="synthetic batches instead of --data_dir")
    p.add_argument("--seed", type=int, default=1234, help="first synthetic batch seed")
    p.add_argument("--det_init", action="store_true",
                   help="closed-form weights (autoformer_amd.detinit, the goldens' initialiser)")
    p.add_argument("--log_step", type=int, default=10)
    return p


def config_from_args(args):
    """The reference's Config for the flags; refuses what the modules cannot take, before anything is built."""
    if not args.synthetic and not args.data_dir:
        raise SystemExit("one of --data_dir or --synthetic is required")
    if not args.classifier_ckpt and not args.det_init:
        raise SystemExit("--classifier_ckpt is required (a MetaDV state_dict, as train_classifier writes it) unless "
                         "--det_init")
    if args.len_crop < 128:
        raise SystemExit(f"--len_crop {args.len_crop}: MetaDV crops windows of 128 frames")
    if args.len_crop != DISC_LEN_CROP:
        raise SystemExit(f"--len_crop {args.len_crop}: the Discriminator is hard-wired to {DISC_LEN_CROP} frames")
    if args.n_critic < 1:
        raise SystemExit(f"--n_critic {args.n_critic}: at least 1")
    config = Config(args.model_name, args.data_dir, bool(args.use_adain), int(args.num_iters))
    if args.pretrained_step is not None:
        config.pretrained_step = args.pretrained_step
    config.num_speaker = args.num_speaker
    config.n_critic, config.lambda_cls, config.lambda_dis = args.n_critic, args.lambda_cls, args.lambda_dis
    config.batch_size, config.len_crop, config.log_step = args.batch_size, args.len_crop, args.log_step
    config.device, config.classifier_ckpt = args.device, args.classifier_ckpt
    return config


def main(argv=None):
    """Parse, build GanVer1Solver and train; returns the per-iteration losses."""
    args = build_parser().parse_args(argv)
    return run(args, config_from_args(args), GanVer1Solver)


def run(args, config, solver_cls, more_labels=()):
    """Train solver_cls on the parsed flags and save the three modules; more_labels: (label, value) pairs added to
    the printed configuration after the lambdas."""
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    if not torch.cuda.is_available():
        raise SystemExit(f"--device {args.device}: no GPU is available, and the HIP kernels need one")
    import autoformer_amd as A

    A.set_compute(args.dtype)
    print(" --- Use Config  ---")
    for label, v in (("Lambda cd", config.lambda_cd), ("Lambda cls", config.lambda_cls),
                     ("Lambda dis", config.lambda_dis), *more_labels, ("N critic", config.n_critic),
                     ("Use Adain", config.use_adain), ("VC Pretrained step", config.pretrained_step)):
        print(f" {label} --- {v}")
    print(" ----------------------")
    if args.synthetic:
        loader = SyntheticUtterances(args.batch_size, args.len_crop, config.dim_emb, args.seed)
    else:
        from .data import get_loader

        loader = get_loader(args.data_dir, dim_neck=config.dim_neck, batch_size=args.batch_size,
                            len_crop=args.len_crop)
    solver = solver_cls(loader, config)
    if args.det_init:
        from .detinit import det_init_

        for m in [solver.VC, solver.D] + ([] if args.classifier_ckpt else [solver.C]):
            det_init_(m)
        weights_changed()
    history = solver.train()
    if args.save_model_name:
        torch.cuda.synchronize()
        for m, suffix in ((solver.VC, ".pt"), (solver.C, ".C.pt"), (solver.D, ".D.pt")):
            # copies: the parameters are views of one flat buffer, which a view would drag into the file whole
            torch.save({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                       f"{args.save_model_name}{suffix}")
    return history


if __name__ == "__main__":
    main()
