"""Autograd ops of the MetaDV speaker classifier (factory/MetaDV.py), each a HIP kernel pair from
metadv.hip (include/autovc_hip_dv.h):

  crop_windows(h, lf, B, T, W)  -> (X, e1)   the conv operand of all S crops, one launch, and the
                                             LSTM output at each utterance's last frame;
                                             backward: one gather-sum that writes all of dh
  chan_mean(Y, S, B)            -> e2        mean over crops of the mixer's last output channel;
                                             backward: all of dY (zero outside that channel)
"""
import torch

from . import kernels as K


class _CropWindowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, lf, B, T, W, lens):
        h = h.contiguous()
        # bf16 mode: the crop reads the LSTM's bf16 twin (half the bytes; X is a bf16 operand only)
        src = getattr(h, "_bf16", None) if K.compute() == K.BF16 else None
        X = K.crop_windows(h if src is None else src, lf, B, T, W, lens=lens)
        if lf.last_dev is None:
            e1 = K.step_select(h, B, T, T - 1)
        else:
            e1 = h.index_select(0, lf.last_dev.long() + torch.arange(B, device=h.device) * T)
        ctx.lf, ctx.dims = lf, (B, T, h.shape[1])
        return X, e1

    @staticmethod
    def backward(ctx, dX, de1):
        B, T, E = ctx.dims
        # a bf16 X receives its gradient in bf16 (autograd casts the conv's fp32 data gradient to the
        # dtype of X); the gather-sum runs in fp32
        dX = dX.float().contiguous()
        de1 = None if de1 is None else de1.contiguous()
        return K.crop_windows_bwd(dX, de1, ctx.lf, B, T, E), None, None, None, None, None


def crop_windows(h, lf, B, T, W, lens=None):
    """Frame-major h (B*T, E) -> (X (S*B*E, W) in the compute dtype, e1 (B, E) fp32)."""
    return _CropWindowsFn.apply(h, lf, B, T, W, lens)


class _ChanMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, S, B):
        ctx.dims = (S, Y.shape[1])
        return K.chan_mean(Y.contiguous(), S, B)

    @staticmethod
    def backward(ctx, g):
        S, O = ctx.dims
        return K.chan_mean_bwd(g.contiguous(), S, O), None, None


def chan_mean(Y, S, B):
    """Mixer output Y (S*B*E, O) -> e2 (B, E), the mean over crops of column O - 1."""
    return _ChanMeanFn.apply(Y, S, B)
