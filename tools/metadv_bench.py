"""MetaDV speaker classifier (factory/MetaDV.py) on the HIP path, bf16 compute, closed-form weights,
T = 176 frames, B = 1 and B = 64:

  infer         the forward-only path under torch.no_grad() (avc_lstm_infer -> crop_windows from the
                bf16 h -> conv -> mixer -> avc_metadv_head)
  train_form    the training composition under torch.no_grad(), same inputs and windows
  step          one training step: forward + backward of cosine_embedding_loss + cross_entropy

Each figure is the median of REPS windows of N calls between device events, after WARM warm-up
calls of the same shape; the two no_grad paths alternate window by window inside one process.
Peak memory is torch's allocator peak over the timed windows of that figure.  Prints one JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import autoformer_amd as A  # noqa: E402
from autoformer_amd import kernels as K  # noqa: E402
from autoformer_amd.detinit import det_init_, det_inputs  # noqa: E402
from autoformer_amd.factory.MetaDV import MetaDV  # noqa: E402

DEV = "cuda:0"
T, WARM, REPS = 176, 3, 7
LEFTS = [20, 9, 25, 41]

A.set_compute(os.environ.get("AUTOVC_COMPUTE", "bf16"))
m = MetaDV(256)
det_init_(m)
m = m.to(DEV).train()


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench(B, n):
    x, e = det_inputs(B, T)
    x, e = torch.from_numpy(x).to(DEV), torch.from_numpy(e).to(DEV)
    labels = (torch.arange(B, device=DEV) * 7) % 256
    ones = torch.ones(B, device=DEV)

    def fwd(infer):
        m.metablock.infer_path = infer
        with torch.no_grad():
            m(x, lefts=LEFTS)

    def step():
        pred, dvec = m(x, lefts=LEFTS)
        loss = F.cosine_embedding_loss(dvec, e, ones) + F.cross_entropy(pred, labels)
        m.zero_grad(set_to_none=True)
        loss.backward()

    forms = {"infer": lambda: fwd(True), "train_form": lambda: fwd(False)}
    ms = {k: [] for k in forms}
    peak = {}
    for k, fn in forms.items():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for _ in range(REPS):
        for k, fn in forms.items():  # alternating: both paths see the same box conditions
            torch.cuda.reset_peak_memory_stats()
            ms[k].append(window(fn, n))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms["step"] = [window(step, n) for _ in range(REPS)]
    peak["step"] = torch.cuda.max_memory_allocated()
    K.check_faults()
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                  "utt_per_s": round(B * 1e3 / med, 1), "peak_mem_mb": round(peak[k] / 2 ** 20)}
    return out


res = {"T": T, "compute": os.environ.get("AUTOVC_COMPUTE", "bf16"), "warmup": WARM, "windows": REPS}
for B, n in ((1, 10), (64, 2)):
    res[f"B{B}"] = dict(bench(B, n), calls_per_window=n)
print(json.dumps(res))
