"""The GE2E loss and the embedder's training step on the HIP path:

  fused         ge2e_loss forward + backward (avc_ge2e: three launches, plus the backward's two scalings) at
                N = 64, M = 10, D = 256 on unit-norm rows
  torch         the plain-torch text of the same loss (cosine_similarity, where, cross_entropy) with autograd
                on the same device, same input
  step          one EmbedderStep (LstmDV 3 x 768 + GE2ELoss, bf16 compute) at N = 64, M = 10, T = 160, with
                the path the batch of 640 takes and the share of the step the fused loss accounts for

Each figure is the median of REPS windows of n calls between device events, after WARM warm-up calls of the
same shape; fused and torch alternate window by window inside one process.  Prints one JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import autoformer_amd as A  # noqa: E402
from autoformer_amd import kernels as K  # noqa: E402
from autoformer_amd.factory.LstmDV import LstmDV  # noqa: E402
from autoformer_amd.ge2e import GE2ELoss, ge2e_loss  # noqa: E402
from autoformer_amd.train_embedder import EmbedderStep  # noqa: E402

DEV = "cuda:0"
N, M, D, T = 64, 10, 256, 160
WARM, REPS, CALLS = 3, 7, 400


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def restatement(e, w):
    c = e.mean(1)
    c_ex = (e.sum(1, keepdim=True) - e) / (M - 1)
    S = F.cosine_similarity(e[:, :, None, :], c[None, None, :, :], dim=-1, eps=1e-8)
    own = F.cosine_similarity(e, c_ex, dim=-1, eps=1e-8)
    S = torch.where(EYE, own[:, :, None].expand(N, M, N), S)
    return F.cross_entropy((w * S).reshape(N * M, N), TARGET)


def stats(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


torch.manual_seed(0)
EYE = torch.eye(N, dtype=torch.bool, device=DEV)[:, None, :].expand(N, M, N)
TARGET = torch.arange(N, device=DEV).repeat_interleave(M)
e = F.normalize(torch.randn(N, M, D, device=DEV), dim=-1).requires_grad_(True)
w = torch.tensor(10.0, device=DEV, requires_grad=True)


def run(loss_fn):
    e.grad = w.grad = None
    loss_fn().backward()


forms = {"fused": lambda: run(lambda: ge2e_loss(e, N, M, w)), "torch": lambda: run(lambda: restatement(e, w))}
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in forms}
for _ in range(REPS):
    for k, fn in forms.items():  # alternating: both forms see the same box conditions
        ms[k].append(window(fn, CALLS))
res = {"N": N, "M": M, "D": D, "T": T, "warmup": WARM, "windows": REPS, "loss_calls_per_window": CALLS}
res.update({k: stats(v) for k, v in ms.items()})
res["torch_over_fused"] = round(res["torch"]["ms"] / res["fused"]["ms"], 2)

A.set_compute("bf16")
model, crit = LstmDV().to(DEV).train(), GE2ELoss().to(DEV)
step = EmbedderStep(model, crit)
x = torch.randn(N * M, T, 80, device=DEV)
for _ in range(2):
    step.step(x, N, M)
step.check()
torch.cuda.reset_peak_memory_stats()
res["step"] = dict(stats([window(lambda: step.step(x, N, M), 2) for _ in range(5)]), compute="bf16", path=step.path,
                   peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20), calls_per_window=2)
step.check()
K.check_faults()
res["loss_share_of_step"] = round(res["fused"]["ms"] / res["step"]["ms"], 5)
print(json.dumps(res))
