"""The loss tail of the GAN trainer's critic step (train_with_gan_ver1.py:149-166) over the fused HIP kernels of
csrc/critic_loss.hip: what follows the three networks, as two launches instead of about twenty.

    c_loss = F.cosine_embedding_loss(trans_style, target_style, ones(B))
    d_loss = nn.BCELoss()(real, ones) + nn.BCELoss()(fake, zeros)
    total  = base + lambda_cls * c_loss + lambda_dis * d_loss          (base: the VC loss, a device scalar)

  critic_loss_block(trans_style, target_style, real, fake, lambda_cls, lambda_dis, base=None)
      -> (total, c_loss, d_loss), device scalars; gradients reach trans_style, real, fake and base

target_style is data and gets no gradient.  Everything is fp32 with fixed-order sums: the same input gives the
same bits.  The forward is one launch; the backward one more, which receives the upstream gradients of all the
outputs as device scalars.
"""
from __future__ import annotations

import torch

from . import kernels as K


def _rows(v):
    """(B, E) with unit column stride and a row stride of at least E (what the kernels index)."""
    if v.dim() == 2 and (v.shape[1] == 1 or v.stride(1) == 1) and (v.shape[0] == 1 or v.stride(0) >= v.shape[1]):
        return v
    return v.contiguous()


class _CriticLossFn(torch.autograd.Function):
    """(total, c_loss, d_loss, extra) of avc_critic_loss, extra = lambda_cls c_loss + lambda_dis d_loss; in the
    manner of train._VCLossFn: a term with no upstream gradient returns None, not zeros."""

    @staticmethod
    def forward(ctx, e, t, p_real, p_fake, base, lambda_cls, lambda_dis):
        e, t, p_real, p_fake = _rows(e), _rows(t), p_real.contiguous(), p_fake.contiguous()
        ctx.set_materialize_grads(False)
        ctx.lam = (float(lambda_cls), float(lambda_dis))
        out, ws = K.critic_loss(e, t, p_real, p_fake, *ctx.lam, base=base)
        ctx.save_for_backward(e, t, p_real, p_fake, ws)
        return out[3], out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, d_total, d_closs, d_dloss, d_extra):
        e, t, p_real, p_fake, ws = ctx.saved_tensors
        need = ctx.needs_input_grad
        both = d_total is not None or d_extra is not None
        hc, hd = both or d_closs is not None, both or d_dloss is not None
        want = (hc and need[0], hd and need[2], hd and need[3])
        g_base = d_total if need[4] else None
        if not any(want):
            return None, None, None, None, g_base, None, None
        d = [g.contiguous() if g is not None else None for g in (d_closs, d_dloss, d_extra, d_total)]
        de, dr, df = K.critic_loss_grad(e, t, p_real, p_fake, *ctx.lam, ws, d, want)
        return de, None, dr, df, g_base, None, None


def critic_loss_block(trans_style, target_style, real, fake, lambda_cls, lambda_dis, base=None):
    """(total, c_loss, d_loss) of the module docstring, fused (_CriticLossFn).  trans_style, target_style: fp32
    (B, E) on the device; real, fake: the discriminator's probabilities, any shape; base: a device scalar added
    into total inside the kernel (its gradient is total's upstream gradient), or None."""
    K.require_device(trans_style, target_style, real, fake, base)
    if trans_style.dim() != 2 or trans_style.shape != target_style.shape:
        raise ValueError(f"critic_loss_block: the styles must both be (B, E), got {tuple(trans_style.shape)} and "
                         f"{tuple(target_style.shape)}")
    total, c_loss, d_loss, _ = _CriticLossFn.apply(trans_style, target_style.detach(), real, fake, base, lambda_cls,
                                                   lambda_dis)
    return total, c_loss, d_loss
