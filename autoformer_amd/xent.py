"""Softmax cross-entropy over the fused HIP kernels of csrc/xent.hip: what trains the MetaDV speaker
classifier (train_classifier.py), and the classification term the GAN trainers' steps need.

For logits x (B, C), labels (B) and a label smoothing s, with y = (1 - s) * onehot(label) + s / C:

    L        = mean_b ( logsumexp(x_b) - sum_c y_c x_bc )      F.cross_entropy(x, labels, label_smoothing=s)
    correct  = the rows whose largest logit is at the label (the lowest index wins an exact tie)

  softmax_xent(logits, labels, smooth)    the autograd op: logits fp32 on the device; the gradient reaches logits
  SoftmaxXent(smooth)                     the module; `.correct` is the last call's count, a device tensor

The kernels compute L, dL/dlogits and the count in one call (two launches) when a gradient is wanted; the
backward only scales by the incoming gradient.  Everything is fp32 with fixed-order sums: the same input
gives the same bits.  Labels go in as a kernels.Labels (host integers, checked against [0, C) before they
reach the device); an integer device tensor is the caller's promise that its values were checked -- the
kernel never uses a label as an address, and a label outside [0, C) makes L NaN.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, smooth):
        need = ctx.needs_input_grad[0]
        loss, d, correct = K.xent(logits, labels, smooth, grads=need)
        if need:
            ctx.save_for_backward(d)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, g, _):
        (d,) = ctx.saved_tensors
        return d * g, None, None


def _device_labels(labels):
    if isinstance(labels, K.Labels):
        return labels
    if isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype in (torch.int32, torch.int64):
        return labels.to(torch.int32).contiguous()
    raise TypeError("softmax_xent: labels must be a kernels.Labels or an int32 / int64 tensor on the device")


def xent_with_count(logits, labels, smooth=0.0):
    """(L, correct): softmax_xent and the top-1 count of the same call (an int32 device scalar)."""
    K.require_device(logits)
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
        raise TypeError(f"softmax_xent: fp32 only, got {getattr(logits, 'dtype', type(logits))}")
    if logits.dim() != 2:
        raise ValueError(f"softmax_xent: logits must be (B, C), got {tuple(logits.shape)}")
    if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        logits = logits.contiguous()
    return _XentFn.apply(logits, _device_labels(labels), float(smooth))


def softmax_xent(logits, labels, smooth=0.0):
    """L of the module docstring for logits (B, C) fp32 on the device; a 0-d tensor."""
    return xent_with_count(logits, labels, smooth)[0]


class SoftmaxXent(nn.Module):
    """softmax_xent as a module; `correct` holds the last call's top-1 count (None before the first)."""

    def __init__(self, smooth=0.0):
        super().__init__()
        smooth = float(smooth)
        if not 0.0 <= smooth < 1.0:
            raise ValueError(f"SoftmaxXent: smooth = {smooth} outside [0, 1)")
        self.smooth = smooth
        self.correct = None

    def forward(self, logits, labels):
        loss, self.correct = xent_with_count(logits, labels, self.smooth)
        return loss
