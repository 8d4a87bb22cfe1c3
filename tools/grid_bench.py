"""All-pairs conversion of N speakers: autoformer_amd.evaluate.convert_grid (batched under per-utterance
BatchNorm, the encoder once per source) against the loop of Converter.convert at B = 1 it replaces --
both from this tree, on the same device, in the same process, alternating.  AutoVC(44, 256, 512, 22) on
closed-form weights, train mode, T = 176, bf16 compute, host mels in -> host mels out.

Each timed pass ends with its results on the host (the device-to-host copy synchronises), so the host
clock covers the device work.  Passes alternate grid / loop after a warm-up of both; the table gives
the median and the range over the passes.  The two paths' outputs are compared pair by pair.

Also records the per-segment BatchNorm kernel's error on a large-mean / small-spread segment next to an
fp32 two-pass computation on the CPU (tests/test_gpu_bn_seg.py::test_large_mean_small_spread).

--model NAME --batch_families times the opt-in batched grid of another family (MetaConv, MetaPool, the
AdaIN variants AutoVC2 / MetaConv2 / MetaPool2 with isAdain) against the same loop, and adds the peak
device memory of a grid pass and, for an AdaIN model, the per-segment AdaIN kernel's error on the
large-mean segment (tests/test_gpu_seg_moments.py::test_large_mean_small_spread).  Without the two options
the run and its report are as before.

  python tools/grid_bench.py [--speakers 20 40] [--passes 3] [--out profiles/eval_grid_bench.txt]
                             [--model AutoVC2 --batch_families]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats_line(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def large_mean_numbers():
    from autoformer_amd import kernels as K

    B, T, C, eps = 3, 176, 80, 1e-5
    g = torch.Generator().manual_seed(3)
    y = (1e3 + 1e-2 * torch.randn(B * T, C, generator=g)).float()
    y3 = y.reshape(B, T, C)
    yd = y3.double()
    want = ((yd - yd.mean(1, keepdim=True)) / torch.sqrt(yd.var(1, unbiased=False, keepdim=True) + eps)).reshape(B * T, C)
    m32 = y3.mean(1, keepdim=True)
    two = ((y3 - m32) / torch.sqrt(((y3 - m32) ** 2).mean(1, keepdim=True) + eps)).reshape(B * T, C)
    got = K.bn_seg_apply(y.cuda(), B, T, torch.ones(C).cuda(), torch.zeros(C).cuda(), eps, K.ACT_NONE)
    return float((two.double() - want).abs().max()), float((got.cpu().double() - want).abs().max())


def large_mean_adain_numbers():
    from autoformer_amd import kernels as K

    n = 176 * 80
    g = torch.Generator().manual_seed(3)
    x = torch.stack([1e3 + 1e-2 * torch.randn(n, generator=g), torch.randn(n, generator=g)]).float()
    xd = x[0].double()
    want = (xd - xd.mean()) / xd.std()
    cpu32 = (x[0] - x[0].mean()) / x[0].std()
    got = K.adain_seg(x.cuda().reshape(-1), 2, torch.zeros(2).cuda(), torch.ones(2).cuda()).reshape(2, n)
    return float((cpu32.double() - want).abs().max()), float((got[0].cpu().double() - want).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, nargs="+", default=[20, 40])
    ap.add_argument("--len-crop", type=int, default=176)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--model", default="AutoVC", help="a factory plugin name")
    ap.add_argument("--batch_families", action="store_true", help="convert_grid(..., batch_families=True)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_bench needs the GPU: a timing taken anywhere else says nothing")
    import autoformer_amd as A
    from autoformer_amd.convert import Converter
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.evaluate import convert_grid

    import importlib

    cls = getattr(importlib.import_module(f"autoformer_amd.factory.{args.model}"), args.model)
    adain = args.model.endswith("2")
    extra = args.model != "AutoVC" or args.batch_families
    A.set_compute("bf16")
    T = args.len_crop
    freq = 22 if T % 22 == 0 else 16
    m = cls(44, 256, 512, freq)
    det_init_(m)
    m = m.cuda().train()
    conv = Converter(m, T)
    lines = [f"device: {torch.cuda.get_device_name(0)}; {args.model}(44, 256, 512, {freq}) det_init, train mode, bf16, "
             f"T = {T}, max_batch = {args.max_batch}, {args.passes} alternating passes after one warm-up pass of each",
             "times in seconds: median (min .. max); host mels in -> host mels out", ""]
    if extra:
        lines.insert(1, f"convert_grid(..., isAdain={adain}, batch_families={args.batch_families}) against the loop of "
                        f"Converter.convert(..., isAdain={adain}) at B = 1")
    lines.append(f"{'N':>4} {'pairs':>6} {'grid':>26} {'B = 1 loop':>26} {'loop / grid':>12} {'max rel-inf grid vs loop':>26}")
    for n in args.speakers:
        x, e = det_inputs(n, T, seed=500 + n)
        srcs = [x[i] for i in range(n)]

        def grid():
            return convert_grid(m, srcs, e, len_crop=T, max_batch=args.max_batch, isAdain=adain,
                                batch_families=args.batch_families)[0]

        def loop():
            return [conv.convert(srcs[s], e[s], e[t], isAdain=adain) for s in range(n) for t in range(n)]

        g0, l0 = grid(), loop()     # warm-up of every shape both use; and the comparison of their results
        rel = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g0, l0))
        tg, tl = [], []
        for _ in range(args.passes):
            for fn, ts in ((grid, tg), (loop, tl)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        (gm, g_lo, g_hi), (lm, l_lo, l_hi) = stats_line(tg), stats_line(tl)
        lines.append(f"{n:>4} {n * n:>6} {f'{gm:.3f} ({g_lo:.3f} .. {g_hi:.3f})':>26} "
                     f"{f'{lm:.3f} ({l_lo:.3f} .. {l_hi:.3f})':>26} {lm / gm:>12.2f} {rel:>26.2e}")
        if extra:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            grid()
            torch.cuda.synchronize()
            lines.append(f"{'':>4} peak device memory of one grid pass at N = {n}: "
                         f"{torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB allocated, "
                         f"{torch.cuda.max_memory_reserved() / 2 ** 20:.0f} MiB reserved")
    if adain:
        cpu_err, gpu_err = large_mean_adain_numbers()
        lines += ["", "avc_adain_seg on a segment of mean 1e3, sigma 1e-2 beside a unit one (n = 176 x 80; max abs error "
                  "of the unit-spread output against fp64):",
                  f"  torch fp32 on the CPU {cpu_err:.3e}; kernel {gpu_err:.3e}; the test's bar 4 x CPU = "
                  f"{4 * cpu_err:.3e}"]
    cpu_err, gpu_err = large_mean_numbers()
    lines += ["", "avc_bn_seg_apply on a segment of mean 1e3, sigma 1e-2 (B, T, C = 3, 176, 80; max abs error of the "
              "unit-spread output against fp64):",
              f"  fp32 two-pass on the CPU (torch) {cpu_err:.3e}; kernel {gpu_err:.3e}; the test's bar 4 x CPU = "
              f"{4 * cpu_err:.3e}"]
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
