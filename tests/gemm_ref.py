"""What an avc_gemm descriptor means, in float64 on the CPU, written from the field descriptions of
include/autovc_hip.h (avc_operand, avc_gemm_desc) and from nothing in the kernels.

An operand is described by `Op`: its flat storage (a 1-D CPU tensor), ld, kstrided, the frame window
(taps, pad, t_out, t_in, chans) or None, and the batch stride.  `product` returns, per batch, the
logical (M, N) matrix  sum_k A(m, k) B(n, k)  and the same sum of absolute values; `reference` adds
the epilogue terms (bias, row_bias, residual, a prior C under accumulate, the cperm column order, a
batch summed into one C) and returns (ref, S) with S = |A| |B|^T + |bias| + |row_bias| + |residual| +
|C0| -- the scale of the fp32 summation bound the tests hold every element to.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch


@dataclass
class Op:
    buf: torch.Tensor  # flat storage, any float dtype (values are read as float64)
    ld: int
    kstrided: bool = False
    window: Optional[Tuple[int, int, int, int, int]] = None  # (taps, pad, t_out, t_in, chans)
    batch_stride: int = 0


def operand_matrix(op: Op, rows: int, K: int, z: int = 0) -> torch.Tensor:
    """The logical rows x K matrix of batch z (float64).
    kstrided = 0: element (r, k) at ptr[r*ld + k]; kstrided = 1: at ptr[k*ld + r].  Window: the
    frame-indexed dimension (r when kstrided = 0, k when kstrided = 1) is f = b*t_out + t, the other is
    tap*chans + c, the element is src[(b*t_in + t + tap - pad)*ld + c], zero when t + tap - pad is
    outside [0, t_in)."""
    src = op.buf.double().reshape(-1)
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    off = z * op.batch_stride
    if op.window is None:
        idx = k * op.ld + r if op.kstrided else r * op.ld + k
        return src[off + idx]
    taps, pad, t_out, t_in, chans = op.window
    f, o = (k, r) if op.kstrided else (r, k)
    b, t = f // t_out, f % t_out
    tap, c = o // chans, o % chans
    assert int(tap.max()) < taps
    t2 = t + tap - pad
    ok = (t2 >= 0) & (t2 < t_in)
    idx = (off + (b * t_in + t2) * op.ld + c).clamp(0, src.numel() - 1)
    return torch.where(ok, src[idx], torch.zeros((), dtype=torch.float64)).expand(rows, K).contiguous()


def product(M, N, K, a: Op, b: Op, batch=1):
    """[(A_z B_z^T, |A_z| |B_z|^T)] for z < batch."""
    out = []
    for z in range(batch):
        A = operand_matrix(a, M, K, z)
        B = operand_matrix(b, N, K, z)
        out.append((A @ B.t(), A.abs() @ B.abs().t()))
    return out


def row_bias_matrix(S, M, N, rb_t, rb_pad):
    """row m = b*rb_t + t adds S[(b*(2 rb_pad + 1) + cls)*N + n], cls = t (t < rb_pad),
    2 rb_pad - (rb_t - 1 - t) (t >= rb_t - rb_pad), else rb_pad."""
    S = S.double().reshape(-1, N)
    m = torch.arange(M)
    b, t = m // rb_t, m % rb_t
    cls = torch.where(t < rb_pad, t, torch.where(t >= rb_t - rb_pad, 2 * rb_pad - (rb_t - 1 - t),
                                                  torch.full_like(t, rb_pad)))
    return S[b * (2 * rb_pad + 1) + cls]


def cperm_columns(x, taps):
    """Logical column n = tap*(N/taps) + ch lands at stored column ch*taps + tap."""
    M, N = x.shape
    return x.reshape(M, taps, N // taps).transpose(1, 2).reshape(M, N)


def reference(M, N, K, a: Op, b: Op, batch=1, batch_sum=False, bias=None, residual=None, c0=None, cperm=0,
              row_bias=None, prods=None):
    """(ref, S), each (batch, M, N) float64 -- (1, M, N) when the batch is summed into one C -- in
    C's STORED column order.  residual / c0: (batch or 1, M, N) in stored order, as C is.
    prods: product()'s result when several descriptors share it."""
    if prods is None:
        prods = product(M, N, K, a, b, batch)
    P = torch.stack([p for p, _ in prods])
    Sa = torch.stack([s for _, s in prods])
    if batch_sum:
        P, Sa = P.sum(0, keepdim=True), Sa.sum(0, keepdim=True)
    if bias is not None:
        P = P + bias.double()
        Sa = Sa + bias.double().abs()
    if row_bias is not None:
        rb = row_bias_matrix(row_bias[0], M, N, row_bias[1], row_bias[2])
        P = P + rb
        Sa = Sa + rb.abs()
    if cperm:
        P = torch.stack([cperm_columns(x, cperm) for x in P])
        Sa = torch.stack([cperm_columns(x, cperm) for x in Sa])
    for extra in (residual, c0):
        if extra is not None:
            P = P + extra.double().reshape(P.shape)
            Sa = Sa + extra.double().reshape(P.shape).abs()
    return P, Sa


def bn_backward(dA, y, mean, rstd, gamma, beta, act):
    """float64 BatchNorm1d + activation backward from the stored conv output y and the batch
    statistics: dz = dA * act'(z), z = yhat*gamma + beta, yhat = (y - mean)*rstd;
    dy = gamma*rstd*(dz - mean(dz) - yhat*mean(dz*yhat)), dgamma = sum dz*yhat, dbeta = sum dz.
    act: 0 none, 1 ReLU, 2 tanh."""
    dA, y = dA.double(), y.double()
    yh = (y - mean.double()) * rstd.double()
    z = yh * gamma.double() + beta.double()
    dz = dA * {0: torch.ones_like(z), 1: (z > 0).double(), 2: 1 - torch.tanh(z) ** 2}[act]
    dy = gamma.double() * rstd.double() * (dz - dz.mean(0) - yh * (dz * yh).mean(0))
    return dy, (dz * yh).sum(0), dz.sum(0)
