"""48 kHz -> 22.05 kHz on the HIP path: Resample.frames (resample.hip, one launch, fp32) against a
plain torch composition on the same GPU in the same process, and against the traffic floor of 4 B
read per input sample plus 4 B written per output sample.

64 utterances of 192,000 samples (4 s at 48 kHz) -> 88,200 samples each.  The composition is the same
polyphase table as one F.conv1d: L = 147 output channels (one per residue, its taps placed at the
residue's input offset inside a common kernel of max offset + taps samples), stride M = 320 over the
zero-padded rows, then the (B, L, periods) result interleaved to (B, periods * L).  Each figure is the
median of REPS windows of N calls between device events, after WARM warm-up calls; the two forms
alternate window by window.  If the convolution does not run on this build the fact is recorded and
the kernel is timed alone.  Also prints the largest difference between the two outputs relative to
the output's peak.  Prints one JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from autoformer_amd.resample import Resample  # noqa: E402

DEV = "cuda:0"
B, N_IN, FS, WARM, REPS, N = 64, 192000, 48000, 3, 7, 20
HBM_TBPS = 8.0  # MI355X peak HBM bandwidth, TB/s

rs = Resample(FS)
tb = rs.table
n_out = rs.out_len(N_IN)
g = torch.Generator().manual_seed(0)
x = (0.1 * torch.randn(B, N_IN, generator=g)).to(DEV)

# the table as one strided convolution
off, cnt = tb.table[:, 0].astype(np.int64), tb.table[:, 2].astype(np.int64)
lo = int(off.min())
klen = int((off + cnt).max()) - lo
kern = np.zeros((tb.L, 1, klen), dtype=np.float32)
for r in range(tb.L):
    kern[r, 0, off[r] - lo:off[r] - lo + cnt[r]] = tb.weights[:cnt[r], r]
kern = torch.from_numpy(kern).to(DEV)
periods = -(-n_out // tb.L)
right = max(0, (periods - 1) * tb.M + lo + klen - N_IN)


def hip():
    return rs.frames(x)[0]


def composition():
    y = F.conv1d(F.pad(x, (-lo, right)).unsqueeze(1), kern, stride=tb.M)[:, :, :periods]
    return y.transpose(1, 2).reshape(B, periods * tb.L)[:, :n_out]


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


res = {"B": B, "fs_in": FS, "fs_out": rs.fs_out, "samples_in": N_IN, "samples_out": n_out, "L": tb.L, "M": tb.M,
       "taps": tb.taps, "tile": tb.tile(), "warmup": WARM, "windows": REPS, "calls_per_window": N}
out = hip()
torch.cuda.synchronize()
forms = {"hip": hip}
try:
    ref_out = composition()
    torch.cuda.synchronize()
    forms["torch_gpu"] = composition
    res["torch_conv1d_on_gpu"] = True
    res["max_difference_over_peak"] = float((out - ref_out).abs().max() / ref_out.abs().max())
except Exception as exc:  # recorded; the kernel is timed alone
    res["torch_conv1d_on_gpu"] = False
    res["torch_conv1d_error"] = f"{type(exc).__name__}: {str(exc)[:200]}"

ms = {k: [] for k in forms}
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
for _ in range(REPS):
    for k, fn in forms.items():  # alternating: both forms see the same conditions
        ms[k].append(window(fn, N))
floor_bytes = 4 * B * N_IN + 4 * B * n_out
res["traffic_floor_bytes"] = floor_bytes
res["traffic_floor_ms_at_peak_hbm"] = round(floor_bytes / (HBM_TBPS * 1e12) * 1e3, 4)
res["fma_per_call"] = int(B * n_out * tb.taps)
for k, v in ms.items():
    med = statistics.median(v)
    res[k] = {"ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
              "out_samples_per_s": round(B * n_out * 1e3 / med), "floor_bytes_per_s_TB": round(floor_bytes / med / 1e9, 3)}
print(json.dumps(res))
