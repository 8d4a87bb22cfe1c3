"""The loss tail of the StarGAN trainer's cycle step (train_with_stargan.py:162-188) over the fused HIP kernels of
csrc/cycle_loss.hip: what follows the networks, as two launches instead of about thirty-five.

    c_trans   = F.cosine_embedding_loss(trans_style, target_style, ones(B))
    c_reconst = F.cosine_embedding_loss(reconstruct_style, org_style, ones(B))
    d_loss    = nn.BCELoss()(real, ones) + nn.BCELoss()(fake, zeros)
    cycle     = F.mse_loss(x_source, x_rec)
    total     = base + lambda_cls * (c_trans + c_reconst) + lambda_dis * d_loss + lambda_cycle * cycle

  cycle_loss_block(trans_style, target_style, reconstruct_style, org_style, real, fake, x_source, x_rec,
                   lambda_cls, lambda_dis, lambda_cycle, base=None)
      -> (total, c_trans, c_reconst, d_loss, cycle), device scalars; gradients reach trans_style,
         reconstruct_style, real, fake, x_rec and base

Both style targets and x_source are data and get no gradient.  Everything is fp32 with fixed-order sums: the same
input gives the same bits.  The forward is one launch; the backward one more, which receives the upstream gradients
of all the outputs as device scalars.
"""
from __future__ import annotations

import torch

from . import kernels as K
from .critic import _rows


class _CycleLossFn(torch.autograd.Function):
    """(total, c_trans, c_reconst, d_loss, cycle, extra) of avc_cycle_loss, in the manner of critic._CriticLossFn: a
    term with no upstream gradient returns None, not zeros; base's gradient is total's upstream."""

    @staticmethod
    def forward(ctx, e1, t1, e2, t2, p_real, p_fake, x, y, base, lambda_cls, lambda_dis, lambda_cycle):
        e1, t1, e2, t2 = _rows(e1), _rows(t1), _rows(e2), _rows(t2)
        p_real, p_fake, x, y = p_real.contiguous(), p_fake.contiguous(), x.contiguous(), y.contiguous()
        ctx.set_materialize_grads(False)
        ctx.lam = (float(lambda_cls), float(lambda_dis), float(lambda_cycle))
        out, ws = K.cycle_loss(e1, t1, e2, t2, p_real, p_fake, x, y, *ctx.lam, base=base)
        ctx.save_for_backward(e1, t1, e2, t2, p_real, p_fake, x, y, ws)
        return out[5], out[0], out[1], out[2], out[3], out[4]

    @staticmethod
    def backward(ctx, d_total, d_ctrans, d_creconst, d_dloss, d_cycle, d_extra):
        *ins, ws = ctx.saved_tensors
        need = ctx.needs_input_grad
        both = d_total is not None or d_extra is not None
        want = ((both or d_ctrans is not None) and need[0], (both or d_creconst is not None) and need[2],
                (both or d_dloss is not None) and need[4], (both or d_dloss is not None) and need[5],
                (both or d_cycle is not None) and need[7])
        g_base = d_total if need[8] else None
        if not any(want):
            return (None,) * 8 + (g_base, None, None, None)
        d = [g.contiguous() if g is not None else None for g in (d_ctrans, d_creconst, d_dloss, d_cycle, d_extra, d_total)]
        de1, de2, dr, df, dy = K.cycle_loss_grad(*ins, *ctx.lam, ws, d, want)
        return de1, None, de2, None, dr, df, None, dy, g_base, None, None, None


def cycle_loss_block(trans_style, target_style, reconstruct_style, org_style, real, fake, x_source, x_rec, lambda_cls,
                     lambda_dis, lambda_cycle, base=None):
    """(total, c_trans, c_reconst, d_loss, cycle) of the module docstring, fused (_CycleLossFn).  The four styles:
    fp32 (B, E) on the device; real, fake: the discriminator's probabilities, any shape; x_source, x_rec: fp32 of
    one element count; base: a device scalar added into total inside the kernel (its gradient is total's upstream
    gradient), or None."""
    K.require_device(trans_style, target_style, reconstruct_style, org_style, real, fake, x_source, x_rec, base)
    for e, t in ((trans_style, target_style), (reconstruct_style, org_style)):
        if e.dim() != 2 or e.shape != t.shape or e.shape != trans_style.shape:
            raise ValueError(f"cycle_loss_block: the styles must all be one (B, E), got {tuple(e.shape)} and "
                             f"{tuple(t.shape)}")
    if x_source.numel() != x_rec.numel():
        raise ValueError(f"cycle_loss_block: x_source and x_rec must hold the same elements, got "
                         f"{tuple(x_source.shape)} and {tuple(x_rec.shape)}")
    total, c_trans, c_reconst, d_loss, cycle, _ = _CycleLossFn.apply(
        trans_style, target_style.detach(), reconstruct_style, org_style.detach(), real, fake, x_source.detach(), x_rec,
        base, lambda_cls, lambda_dis, lambda_cycle)
    return total, c_trans, c_reconst, d_loss, cycle
