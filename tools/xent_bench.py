"""Softmax cross-entropy and the classifier's training step on the HIP path:

  fused         softmax_xent forward + backward (avc_xent: two launches, plus the backward's scaling) at
                B = 64, C = 256, label smoothing 0.1
  torch         F.cross_entropy(label_smoothing = 0.1) with autograd on the same device, same input
  step          one ClassifierStep (MetaDV(256) + SoftmaxXent, bf16 compute) at B = 64, T = 176, with the share
                of the step the fused loss accounts for and the peak memory

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
from autoformer_amd.factory.MetaDV import MetaDV  # noqa: E402
from autoformer_amd.train_classifier import ClassifierStep  # noqa: E402
from autoformer_amd.xent import SoftmaxXent, softmax_xent  # noqa: E402

DEV = "cuda:0"
B, C, T, SMOOTH = 64, 256, 176, 0.1
WARM, REPS, CALLS = 3, 7, 400


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


torch.manual_seed(0)
x = (4.0 * torch.randn(B, C, device=DEV)).requires_grad_(True)
host_labels = torch.randint(0, C, (B,))
labels, labels64 = K.Labels(host_labels, C, DEV), host_labels.to(DEV)


def run(loss_fn):
    x.grad = None
    loss_fn().backward()


forms = {"fused": lambda: run(lambda: softmax_xent(x, labels, SMOOTH)),
         "torch": lambda: run(lambda: F.cross_entropy(x, labels64, label_smoothing=SMOOTH))}
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in forms}
for _ in range(REPS):
    for k, fn in forms.items():  # alternating: both forms see the same box conditions
        ms[k].append(window(fn, CALLS))
res = {"B": B, "C": C, "T": T, "smooth": SMOOTH, "warmup": WARM, "windows": REPS, "loss_calls_per_window": CALLS}
res.update({k: stats(v) for k, v in ms.items()})
res["torch_over_fused"] = round(res["torch"]["ms"] / res["fused"]["ms"], 2)

A.set_compute("bf16")
torch.manual_seed(0)
model = MetaDV(C).to(DEV).train()
step = ClassifierStep(model, SoftmaxXent(SMOOTH))
xs = torch.randn(B, T, 80, device=DEV)
lefts = [0, 16, 32, 48]
for _ in range(2):
    step.step(xs, labels, lefts)
step.check()
torch.cuda.reset_peak_memory_stats()
res["step"] = dict(stats([window(lambda: step.step(xs, labels, lefts), 4) for _ in range(5)]), compute="bf16",
                   peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20), calls_per_window=4)
step.check()
K.check_faults()
res["loss_share_of_step"] = round(res["fused"]["ms"] / res["step"]["ms"], 5)
print(json.dumps(res))
