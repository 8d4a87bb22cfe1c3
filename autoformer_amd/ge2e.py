"""The GE2E loss (Wan et al. 2018, "Generalized end-to-end loss for speaker verification", softmax form)
over the fused HIP kernels of csrc/ge2e.hip: what trains the LstmDV embedder (train_embedder.py).

For e (N, M, D) -- N speakers, M utterances each, rows of any norm -- and a scale w:

    c[k]       = e[k].mean(0)                                  the inclusive centroids
    c_ex[j, i] = (e[j].sum(0) - e[j, i]) / (M - 1)             own centroid without the utterance itself
    S[j, i, k] = cos(e[j, i], c[k]) for k != j,  cos(e[j, i], c_ex[j, i]) for k == j     (eps = 1e-8)
    L          = cross_entropy(w * S, target = j), mean over the N*M rows

The usual additive bias b (w * S + b) is left out.  Cross-entropy is invariant to a constant added to
every logit of a row, so L does not depend on b and dL/db is identically zero (a fp64 check on the CPU
gave 1e-17): a parameter that never moves is no parameter.

  ge2e_loss(e, N, M, w)    the autograd op: e (N*M, D) or (N, M, D) fp32 on the device, w a one-element
                           tensor; gradients reach e and w
  GE2ELoss()               the module: parameter w, initialised to 10.0 as in the paper

The kernels compute L, dL/de and dL/dw in one call (three launches) when a gradient is wanted; the
backward only scales them by the incoming gradient.  Everything is fp32 with fixed-order sums: the same
input gives the same bits.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K


class _GE2EFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, w, N, M):
        shape = e.shape
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, de, dw = K.ge2e(e.contiguous(), N, M, w.detach().reshape(1), grads=need)
        if need:
            ctx.save_for_backward(de, dw)
        ctx.shapes = (shape, w.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        de, dw = ctx.saved_tensors
        eshape, wshape = ctx.shapes
        ge = (de * g).reshape(eshape) if ctx.needs_input_grad[0] else None
        gw = (dw * g).reshape(wshape) if ctx.needs_input_grad[1] else None
        return ge, gw, None, None


def ge2e_loss(e, N, M, w):
    """L of the module docstring for e (N*M, D) or (N, M, D), speaker-major rows; a 0-d tensor.  w is a
    one-element tensor on the device (GE2ELoss's parameter: it gets a gradient), or a Python number, which
    is a constant scale."""
    if not isinstance(w, torch.Tensor):
        K.require_device(e)
        w = torch.tensor(float(w), device=e.device)
    K.require_device(e, w)
    if e.dtype != torch.float32 or w.dtype != torch.float32:
        raise TypeError(f"ge2e_loss: fp32 only, got e {e.dtype}, w {w.dtype}")
    N, M = int(N), int(M)
    if e.dim() not in (2, 3) or (e.dim() == 2 and e.shape[0] != N * M) or (e.dim() == 3 and e.shape[:2] != (N, M)):
        raise ValueError(f"ge2e_loss: e must be (N*M, D) or (N, M, D) with N = {N}, M = {M}, got {tuple(e.shape)}")
    return _GE2EFn.apply(e, w, N, M)


class GE2ELoss(nn.Module):
    """GE2E with its learned scale w (10.0 at the start; the trainer keeps it above 1e-6).  No bias: see
    the module docstring."""

    def __init__(self, init_w=10.0):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(float(init_w)))

    def forward(self, e, N, M):
        return ge2e_loss(e, N, M, self.w)
