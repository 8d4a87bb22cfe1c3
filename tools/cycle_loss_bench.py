"""The cycle step's loss tail and the StarGAN trainer's cycle iteration on the HIP path:

  fused         cycle_loss_block forward + backward (avc_cycle_loss + avc_cycle_loss_grad: two launches) at
                B = 64, E = 256, n_r = n_f = 64, n_x = 64 * 176 * 80 = 901120, with a base, lambda_cls 0.1,
                lambda_dis 1, lambda_cycle 1
  torch         the same expression in plain torch with autograd on the same device, same inputs:
                base + 0.1 (F.cosine_embedding_loss + F.cosine_embedding_loss) + (BCELoss(real, 1) +
                BCELoss(fake, 0)) + F.mse_loss(x, x_rec)
  cycle_step    one CycleStep.cycle_step (AutoVC + MetaDV(80) + Discriminator, bf16 compute) at B = 64, T = 176,
                with the share of it the fused loss tail accounts for and the peak memory
  vc_step       one CycleStep.vc_step of the same modules

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
from autoformer_amd.cycle import cycle_loss_block  # noqa: E402
from autoformer_amd.detinit import det_inputs  # noqa: E402
from autoformer_amd.factory.AutoVC import AutoVC  # noqa: E402
from autoformer_amd.factory.Discriminator import Discriminator  # noqa: E402
from autoformer_amd.factory.MetaDV import MetaDV  # noqa: E402
from autoformer_amd.train_stargan import CycleStep  # noqa: E402

DEV = "cuda:0"
B, E, T, LC, LD, LY = 64, 256, 176, 0.1, 1.0, 1.0
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
e1 = torch.randn(B, E, device=DEV).requires_grad_(True)
e2 = torch.randn(B, E, device=DEV).requires_grad_(True)
t1 = F.normalize(torch.randn(B, E, device=DEV), dim=1)
t2 = F.normalize(torch.randn(B, E, device=DEV), dim=1)
real = (0.02 + 0.96 * torch.rand(B, 1, device=DEV)).requires_grad_(True)
fake = (0.02 + 0.96 * torch.rand(B, 1, device=DEV)).requires_grad_(True)
x = torch.randn(B, T, 80, device=DEV)
x_rec = (x + 0.5 * torch.randn(B, T, 80, device=DEV)).requires_grad_(True)
base = torch.tensor(13.8, device=DEV).requires_grad_(True)
ones = torch.ones(B, device=DEV)
bce = torch.nn.BCELoss()
leaves = (e1, e2, real, fake, x_rec, base)


def torch_tail():
    c = F.cosine_embedding_loss(e1, t1, ones) + F.cosine_embedding_loss(e2, t2, ones)
    d = bce(real, torch.ones_like(real)) + bce(fake, torch.zeros_like(fake))
    return base + LC * c + LD * d + LY * F.mse_loss(x, x_rec)


def run(loss_fn):
    for v in leaves:
        v.grad = None
    loss_fn().backward()


forms = {"fused": lambda: run(lambda: cycle_loss_block(e1, t1, e2, t2, real, fake, x, x_rec, LC, LD, LY, base=base)[0]),
         "torch": lambda: run(torch_tail)}
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in forms}
for _ in range(REPS):
    for k, fn in forms.items():  # alternating: both forms see the same box conditions
        ms[k].append(window(fn, CALLS))
res = {"B": B, "E": E, "n_r": B, "n_f": B, "n_x": B * T * 80, "T": T, "warmup": WARM, "windows": REPS,
       "loss_calls_per_window": CALLS}
res.update({k: stats(v) for k, v in ms.items()})
res["torch_over_fused"] = round(res["torch"]["ms"] / res["fused"]["ms"], 2)

A.set_compute("bf16")
torch.manual_seed(0)
mods = [m.to(DEV).train() for m in (AutoVC(44, 256, 512, 22), MetaDV(80), Discriminator())]
step = CycleStep(*mods)
(xs, emb), (xt, et) = [[torch.from_numpy(v).to(DEV) for v in det_inputs(B, T, seed=s)] for s in (1, 2)]
lefts_a, lefts_b = [0, 16, 32, 48], [7, 40, 19, 2]
for _ in range(2):
    step.cycle_step(xs, emb, xt, et, lefts_a, lefts_b)
    step.vc_step(xs, emb)
step.check()
torch.cuda.reset_peak_memory_stats()
res["cycle_step"] = dict(stats([window(lambda: step.cycle_step(xs, emb, xt, et, lefts_a, lefts_b), 4) for _ in range(5)]),
                         compute="bf16", peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20),
                         calls_per_window=4)
torch.cuda.reset_peak_memory_stats()
res["vc_step"] = dict(stats([window(lambda: step.vc_step(xs, emb), 4) for _ in range(5)]), compute="bf16",
                      peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20), calls_per_window=4)
step.check()
K.check_faults()
res["loss_share_of_cycle_step"] = round(res["fused"]["ms"] / res["cycle_step"]["ms"], 5)
print(json.dumps(res))
