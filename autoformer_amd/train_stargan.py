"""The StarGAN trainer: train_with_stargan.py (:15-279) over the HIP kernels -- the GAN trainer of train_gan.py with a
cycle: the converted mel is converted back to the source style, and the reconstruction has to match the source
mel and carry the source style.

  CycleStep(VC, C, Dm)                 CriticStep with a third kind of iteration, cycle_step
  StarGanSolver(loader, config)        the reference's Solver: GanVer1Solver's loop with cycle iterations

Every iteration computes the VC loss of train.py.  A cycle iteration ((i + 1) % n_critic == 0 and (i + 1) >
pretrained_step: train_gan.critic_due) draws a second batch (x_target, target_style) and adds

    lambda_cls * (cosine_embedding_loss(C(x_conv).d_vec, target_style, 1)
                  + cosine_embedding_loss(C(x_rec).d_vec, org_style, 1))
    + lambda_dis * (BCE(D(x_target), 1) + BCE(D(x_conv), 0)) + lambda_cycle * mse_loss(x_source, x_rec)

with x_conv = VC(x_source, org_style, target_style) and x_rec = VC(x_conv, target_style, org_style), the encoder
reading the converted mel with the graph attached (cycle.cycle_loss_block: the whole tail, with its addition to
the VC loss, in one launch and one more for its backward); ONE backward, then all three Adams step.  Any other
iteration steps VC alone.

  python -m autoformer_amd.train_stargan --model_name AutoVC (--data_dir DIR | --synthetic) --classifier_ckpt FILE
      [--save_model_name NAME] [--use_adain 1] [--num_iters 10] [--n_critic 10] [--pretrained_step K]
      [--lambda_cls 0.1] [--lambda_dis 1] [--lambda_cycle 1] [--batch_size 2] [--dtype fp32|bf16] [--seed 1234]
      [--det_init] [--log_step 10] [--num_speaker C] [--device cuda:0]

The flags, the files read and the three files written (NAME.pt, NAME.C.pt, NAME.D.pt) are train_gan's.
"""
from __future__ import annotations

import importlib

from . import kernels as K
from . import train_gan as G
from .cycle import cycle_loss_block

LOG_KEYS = ["VC/loss_id", "VC/loss_id_psnt", "VC/loss_cd", "C/loss_trans", "C/loss_reconst", "D/loss", "Cycle/loss"]


# ------------------------------------------------------------------------- step
class CycleStep(G.CriticStep):
    """CriticStep with the cycle iteration of train_with_stargan.py:118-198.  The decoder and postnet run three
    times inside one graph, the encoder four (AdaIN: six), the classifier twice; in gradient-sink mode every pass
    adds into the same flat gradient buffers.  There is no decoder-done hook, no early Adam slice and no recorded
    replay, for CriticStep's reason."""

    def __init__(self, VC, C, Dm, lr=1e-4, lambda_cd=1, lambda_cls=0.1, lambda_dis=1, lambda_cycle=1,
                 use_adain=False):
        super().__init__(VC, C, Dm, lr, lambda_cd, lambda_cls, lambda_dis, use_adain)
        self.lambda_cycle = float(lambda_cycle)

    def cycle_step(self, x, emb, x_target, emb_target, lefts_trans, lefts_reconst):
        """The cycle iteration.  lefts_trans, lefts_reconst: C's window starts for the converted and for the
        reconstructed mel (C.draw_lefts(T) each), arguments so that a step never draws from Python's `random`.
        The forward calls, in the order that moves the BatchNorm running statistics: VC identity, encoder re-pass,
        (AdaIN: the target's feature pass,) conversion, (AdaIN: the source's feature pass,) cycle pass, C on the
        conversion, C on the reconstruction, D real, D fake.  Returns (l_id, l_id_psnt, l_cd, c_trans, c_reconst,
        d_loss, cycle), device scalars."""
        K.require_device(x, emb, x_target, emb_target)
        self._zero()
        VC = self.VC
        VC._decoder_bwd_done = None
        vc_total, parts, x_psnt = self.loss_fn(VC, x, emb, self.lambda_cd)
        if self.use_adain:
            _, target_feature = VC(x_psnt, emb_target, None)
            _, x_conv, _ = VC(x, emb, emb_target, target_feature)
            x_conv = x_conv.squeeze(1)
            _, source_feature = VC(x, emb, None)
            _, x_rec, _ = VC(x_conv, emb_target, emb, source_feature)
        else:
            _, x_conv, _ = VC(x, emb, emb_target)
            x_conv = x_conv.squeeze(1)
            _, x_rec, _ = VC(x_conv, emb_target, emb)
        x_rec = x_rec.squeeze(1)
        _, trans_style = self.C(x_conv, lefts=lefts_trans)
        _, reconstruct_style = self.C(x_rec, lefts=lefts_reconst)
        real = self.D(x_target)
        fake = self.D(x_conv)
        total, c_trans, c_reconst, d_loss, cycle = cycle_loss_block(
            trans_style, emb_target, reconstruct_style, emb, real, fake, x, x_rec, self.lambda_cls, self.lambda_dis,
            self.lambda_cycle, base=vc_total)
        self._finish(total, (self.vc_opt, self.c_opt, self.d_opt))
        return (*parts, c_trans, c_reconst, d_loss, cycle)


# ------------------------------------------------------------------------- solver
class Config(G.Config):
    """train_with_stargan.py:246-265 (it has no lambda_ad; train_gan's Config keeps the unused one)."""

    def __init__(self, model_name, data_dir, use_adain, num_iters):
        super().__init__(model_name, data_dir, use_adain, num_iters)
        self.lambda_cycle = 1


class StarGanSolver(G.GanVer1Solver):
    """Mirror of train_with_stargan.py:Solver (:15-243): GanVer1Solver with CycleStep.  The log line carries the
    reference's seven keys in its order; C/loss_trans, C/loss_reconst, D/loss and Cycle/loss show the latest cycle
    iteration's values, 0.0 before the first (the reference prints 0.0 up to pretrained_step and reads stale
    variables after it)."""

    def __init__(self, vcc_loader, config):
        self.lambda_cycle = config.lambda_cycle
        super().__init__(vcc_loader, config)
        self.log_keys = list(LOG_KEYS)

    def make_step(self):
        return CycleStep(self.VC, self.C, self.D, 0.0001, self.lambda_cd, self.lambda_cls, self.lambda_dis,
                         self.lambda_cycle, self.use_adain)

    def critic_iteration(self, x_source, org_style):
        x_target, target_style = self.get_data()
        T = x_source.shape[-2]
        lefts_trans, lefts_reconst = self.C.draw_lefts(T), self.C.draw_lefts(T)
        return self.step.cycle_step(x_source, org_style, x_target, target_style, lefts_trans, lefts_reconst)


# ------------------------------------------------------------------------- command line
def build_parser():
    p = G.build_parser()
    p.prog = "python -m autoformer_amd.train_stargan"
    p.description = ("train_with_stargan.py on the MI355X: train_gan with a cycle back to the source style, over the "
                     "HIP kernels.")
    p.add_argument("--lambda_cycle", type=float, default=1)
    return p


def config_from_args(args):
    """The reference's Config for the flags; train_gan's refusals, and the two its step object would raise only
    after the modules are built: an *_Adjust model, and use_adain against the model's family."""
    from .factory._variants import AdaINModel, AdjustModel

    base = G.config_from_args(args)
    try:
        cls = getattr(importlib.import_module(f"autoformer_amd.factory.{args.model_name}"), args.model_name)
    except (ImportError, AttributeError):
        raise SystemExit(f"--model_name {args.model_name}: no such model in autoformer_amd.factory")
    if issubclass(cls, AdjustModel):
        raise SystemExit(f"--model_name {args.model_name}: the *_Adjust models return four outputs; "
                         "train_with_stargan.py has no step for them")
    if bool(args.use_adain) != issubclass(cls, AdaINModel):
        raise SystemExit(f"--use_adain {bool(args.use_adain)} with --model_name {args.model_name}: the AdaIN variants "
                         "(AutoVC2, MetaConv2, MetaPool2) need --use_adain 1, the plain families must not have it")
    config = Config(base.model_name, base.data_dir, base.use_adain, base.num_iters)
    config.__dict__.update(base.__dict__)
    config.lambda_cycle = args.lambda_cycle
    return config


def main(argv=None):
    """Parse, build StarGanSolver and train; returns the per-iteration losses (seven per iteration)."""
    args = build_parser().parse_args(argv)
    config = config_from_args(args)
    return G.run(args, config, StarGanSolver, more_labels=(("Lambda cycle", config.lambda_cycle),))


if __name__ == "__main__":
    main()
