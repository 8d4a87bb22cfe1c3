"""Whole-utterance conversion of a set of recordings of different lengths: autoformer_amd.convert.convert_whole
(ragged batches under layers.per_utterance_bn(lens=...)) against the loop of the one-utterance path it
replaces, Converter(model, len_crop = P_b).convert at B = 1 -- both from this tree, on the same device, in
the same process, alternating.  64 synthetic utterances whose lengths are drawn once (seed 7) uniformly
from 96 .. 640 frames (1.1 .. 7.4 s); AutoVC(44, 256, 512, 22) on closed-form weights, train mode, bf16
compute, host mels in -> host mels out.

Each timed pass ends with its results on the host (the device-to-host copy synchronises, and an explicit
synchronise follows), so the host clock covers the device work.  Passes alternate whole / loop after a
warm-up of both (every shape either uses); a convert_whole pass is --reps calls back to back (one call is
tens of milliseconds: too short a window on its own) and its time is per call; the table gives the median
and the range over the passes.  The
two paths' outputs are compared utterance by utterance, and the plan's batches are listed with the share
of their frames that is padding (rows past an utterance's own P_b).

  python tools/convert_whole_bench.py [--n 64] [--passes 5] [--reps 10] [--max-batch 64] [--max-frames 16384]
                                      [--out profiles/convert_whole_bench.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

FREQ = 22


def stats_line(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    from autoformer_amd.convert import MAX_FRAMES

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--lo", type=int, default=96)
    ap.add_argument("--hi", type=int, default=640)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="convert_whole calls per timed pass")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--max-frames", type=int, default=MAX_FRAMES)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convert_whole_bench needs the GPU: a timing taken anywhere else says nothing")
    import autoformer_amd as A
    from autoformer_amd.convert import Converter, convert_whole, padded_len, plan_whole
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.factory.AutoVC import AutoVC

    A.set_compute("bf16")
    m = AutoVC(44, 256, 512, FREQ)
    det_init_(m)
    m = m.cuda().train()
    lens = [int(v) for v in np.random.RandomState(args.seed).randint(args.lo, args.hi + 1, size=args.n)]
    x, e = det_inputs(args.n, max(lens), seed=700)
    mels = [np.ascontiguousarray(x[i][:lens[i]]) for i in range(args.n)]
    eo, et = e, np.roll(e, -1, axis=0)
    P = [padded_len(T, FREQ) for T in lens]
    plan = plan_whole(lens, FREQ, args.max_batch, args.max_frames)

    def whole():
        return convert_whole(m, mels, eo, et, max_batch=args.max_batch, max_frames=args.max_frames)

    def loop():
        return [Converter(m, P[i]).convert(mels[i], eo[i], et[i]) for i in range(args.n)]

    w0, l0 = whole(), loop()   # warm-up of every shape both use; and the comparison of their results
    rel = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(w0, l0)]
    tw, tl = [], []
    for _ in range(args.passes):
        for fn, ts, reps in ((whole, tw, args.reps), (loop, tl, 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / reps)
    (wm, w_lo, w_hi), (lm, l_lo, l_hi) = stats_line(tw), stats_line(tl)
    frames = sum(lens)
    lines = [f"device: {torch.cuda.get_device_name(0)}; AutoVC(44, 256, 512, {FREQ}) det_init, train mode, bf16; "
             f"{args.n} utterances of {min(lens)} .. {max(lens)} frames (seed {args.seed}, uniform {args.lo} .. {args.hi}), "
             f"{frames} frames = {frames * 256 / 22050:.0f} s of audio",
             f"max_batch = {args.max_batch}, max_frames = {args.max_frames}; {args.passes} alternating passes after one "
             f"warm-up pass of each, a convert_whole pass = {args.reps} calls; seconds per call: median (min .. max); "
             "host mels in -> host mels out", "",
             f"{'convert_whole':>28} {'B = 1 loop':>28} {'loop / whole':>13} {'max rel-inf whole vs loop':>27}",
             f"{f'{wm:.3f} ({w_lo:.3f} .. {w_hi:.3f})':>28} {f'{lm:.3f} ({l_lo:.3f} .. {l_hi:.3f})':>28} {lm / wm:>13.2f} "
             f"{max(rel):>27.2e}",
             f"per utterance: whole {1e3 * wm / args.n:.2f} ms, loop {1e3 * lm / args.n:.2f} ms; "
             f"{frames / wm / 1e3:.0f} k frames/s against {frames / lm / 1e3:.0f} k", "",
             f"the plan: {len(plan)} batches", f"{'batch':>6} {'rows':>5} {'Tmax':>5} {'shortest P':>11} {'padded frames':>14}"]
    for k, (idx, Tmax) in enumerate(plan):
        own = sum(P[i] for i in idx)
        lines.append(f"{k:>6} {len(idx):>5} {Tmax:>5} {min(P[i] for i in idx):>11} {1 - own / (len(idx) * Tmax):>13.1%}")
    total = sum(len(idx) * Tmax for idx, Tmax in plan)
    lines.append(f"{'all':>6} {args.n:>5} {'':>5} {'':>11} {1 - sum(P) / total:>13.1%}")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    whole()
    torch.cuda.synchronize()
    lines.append(f"peak device memory of one convert_whole pass: {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB "
                 f"allocated, {torch.cuda.max_memory_reserved() / 2 ** 20:.0f} MiB reserved")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
