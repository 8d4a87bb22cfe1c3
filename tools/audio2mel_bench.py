"""Waveform -> log-mel on the HIP path: Audio2Mel.frames (audio.hip, one launch, fp32) against the
plain torch composition (F.pad reflect + torch.stft + matmul + log10) on the same GPU in the same
process, and against the traffic floor of 4 B per sample read plus 320 B per frame written.

64 utterances of 88,200 samples (4 s at 22050 Hz, T = 344 frames each).  Each figure is the median
of REPS windows of N calls between device events, after WARM warm-up calls; the two forms alternate
window by window.  The compute mode (bf16 / fp32) is irrelevant: the path is fp32 throughout.
If torch.stft does not run on this build the fact is recorded and the CPU composition on 16 threads
is timed with a host clock instead.  Also prints the largest difference between the two outputs
in the tests' peak-relative linear metric.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from autoformer_amd.melgan import Audio2Mel  # noqa: E402

DEV = "cuda:0"
B, L, WARM, REPS, N = 64, 88200, 3, 7, 20
HBM_TBPS = 8.0  # MI355X peak HBM bandwidth, TB/s

a2m = Audio2Mel().to(DEV)
T = a2m.n_frames(L)
g = torch.Generator().manual_seed(0)
x = (0.1 * torch.randn(B, L, generator=g)).to(DEV)


def hip():
    return a2m.frames(x)


def composition(xx, basis, win):
    p = (1024 - 256) // 2
    padded = F.pad(xx.unsqueeze(1), (p, p), "reflect").squeeze(1)
    spec = torch.stft(padded, n_fft=1024, hop_length=256, win_length=1024, window=win, center=False,
                      return_complex=True)
    return torch.log10(torch.clamp(torch.matmul(basis, spec.abs()), min=1e-5))


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def host_window(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n


res = {"B": B, "L": L, "T": T, "frames": B * T, "warmup": WARM, "windows": REPS, "calls_per_window": N}
try:
    ref_out = composition(x, a2m.mel_basis, a2m.window)
    torch.cuda.synchronize()
    forms = {"hip": (hip, window, N), "torch_gpu": (lambda: composition(x, a2m.mel_basis, a2m.window), window, N)}
    res["torch_stft_on_gpu"] = True
except Exception as exc:  # recorded, and the CPU composition is timed instead
    res["torch_stft_on_gpu"] = False
    res["torch_stft_error"] = f"{type(exc).__name__}: {str(exc)[:200]}"
    torch.set_num_threads(16)
    xc, bc, wc = x.cpu(), a2m.mel_basis.cpu(), a2m.window.cpu()
    ref_out = composition(xc, bc, wc).to(DEV)
    forms = {"hip": (hip, window, N), "torch_cpu16": (lambda: composition(xc, bc, wc), host_window, 1)}

out = hip()
lin, rl = torch.clamp(10.0 ** out.double(), min=1e-5), torch.clamp(10.0 ** ref_out.transpose(1, 2).double(), min=1e-5)
res["max_peak_relative_difference"] = float(((lin - rl).abs().amax(dim=2) / rl.amax(dim=2)).max())

ms = {k: [] for k in forms}
for k, (fn, _, _) in forms.items():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
for _ in range(REPS):
    for k, (fn, win_fn, n) in forms.items():  # alternating: both forms see the same conditions
        ms[k].append(win_fn(fn, n))
floor_bytes = 4 * B * L + 320 * B * T
res["traffic_floor_bytes"] = floor_bytes
res["traffic_floor_ms_at_peak_hbm"] = round(floor_bytes / (HBM_TBPS * 1e12) * 1e3, 4)
for k, v in ms.items():
    med = statistics.median(v)
    res[k] = {"ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
              "frames_per_s": round(B * T * 1e3 / med), "floor_bytes_per_s_TB": round(floor_bytes / med / 1e9, 3)}
print(json.dumps(res))
