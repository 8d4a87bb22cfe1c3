"""The vocoder over a set of recordings of different lengths: MelVocoder.inverse_ragged (ragged batches through
Generator.frames_ragged) against the loop it replaces, MelVocoder.inverse_frames at B = 1 per utterance -- the
wav-to-wav CLI's last loop before the ragged path -- both from this tree, on the same device, in the same process,
alternating.  Then the wav-to-wav total both ways: convert_whole(..., vocoder=...) against convert_whole followed by
that loop.  The 64 lengths of tools/convert_whole_bench.py (seed 7, uniform 96 .. 640 frames), Generator(80, 32, 3)
and AutoVC(44, 256, 512, 22) on closed-form weights, bf16 compute, host mels in -> host wavs out.

Each timed pass ends with its results on the host (the device-to-host copies synchronise, and an explicit
synchronise follows), so the host clock covers the device work.  Passes alternate ragged / loop after a warm-up of
both (every shape either uses); a pass is --reps (ragged) or --loop-reps (loop) calls back to back, so that a
window is some tenths of a second, and its time is per call; the table gives the median and the range over the
passes.  The two paths' wavs are compared utterance by utterance, and the plan's batches are listed with the share
of their frames that is padding (rows past an utterance's own length).

  python tools/vocoder_ragged_bench.py [--n 64] [--passes 5] [--reps 10] [--loop-reps 3] [--max-batch 32]
                                       [--max-frames 8192] [--out profiles/vocoder_ragged_bench.txt]
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


def alternate(fa, fb, passes, reps_a, reps_b):
    ta, tb = [], []
    for _ in range(passes):
        for fn, ts, reps in ((fa, ta, reps_a), (fb, tb, reps_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / reps)
    return stats_line(ta), stats_line(tb)


def fmt(s):
    return f"{s[0]:.4f} ({s[1]:.4f} .. {s[2]:.4f})"


def main():
    from autoformer_amd.melgan import VOCODER_MAX_BATCH, VOCODER_MAX_FRAMES

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--lo", type=int, default=96)
    ap.add_argument("--hi", type=int, default=640)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="ragged calls per timed pass")
    ap.add_argument("--loop-reps", type=int, default=3, help="loop calls per timed pass")
    ap.add_argument("--max-batch", type=int, default=VOCODER_MAX_BATCH)
    ap.add_argument("--max-frames", type=int, default=VOCODER_MAX_FRAMES)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_ragged_bench needs the GPU: a timing taken anywhere else says nothing")
    import autoformer_amd as A
    from autoformer_amd.convert import convert_whole, plan_whole
    from autoformer_amd.detinit import det_init_, det_inputs, det_melgan_state
    from autoformer_amd.factory.AutoVC import AutoVC
    from autoformer_amd.melgan import Generator, MelVocoder

    A.set_compute("bf16")
    dev = "cuda:0"
    g = Generator(80, 32, 3)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in
                       det_melgan_state([(k, tuple(v.shape)) for k, v in g.state_dict().items()]).items()})
    voc = MelVocoder(device=dev, generator=g)
    m = AutoVC(44, 256, 512, FREQ)
    det_init_(m)
    m = m.cuda().train()
    lens = [int(v) for v in np.random.RandomState(args.seed).randint(args.lo, args.hi + 1, size=args.n)]
    x, e = det_inputs(args.n, max(lens), seed=700)
    mels = [np.ascontiguousarray(x[i][:lens[i]]) for i in range(args.n)]
    eo, et = e, np.roll(e, -1, axis=0)
    plan = plan_whole(lens, 1, args.max_batch, args.max_frames)

    def loop_over(ms):  # the CLI's loop before the ragged path: one utterance at a time
        return [voc.inverse_frames(torch.from_numpy(mel).unsqueeze(0).to(dev))[0].float().cpu().numpy() for mel in ms]

    def ragged():
        return [w.cpu().numpy() for w in voc.inverse_ragged(mels, max_batch=args.max_batch, max_frames=args.max_frames)]

    def loop():
        return loop_over(mels)

    def total_ragged():
        return convert_whole(m, mels, eo, et, vocoder=voc)[1]

    def total_loop():
        return loop_over(convert_whole(m, mels, eo, et))

    r0, l0 = ragged(), loop()  # warm-up of every shape both use; and the comparison of their results
    rel = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(r0, l0)]
    assert all(a.shape == (T * 256,) for a, T in zip(r0, lens))
    tr0, tl0 = total_ragged(), total_loop()
    rel_t = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(tr0, tl0)]
    sr, sl = alternate(ragged, loop, args.passes, args.reps, args.loop_reps)
    str_, stl = alternate(total_ragged, total_loop, args.passes, args.reps, args.loop_reps)
    frames = sum(lens)
    head = f"{'':>22} {'ragged batches':>28} {'B = 1 loop':>28} {'loop / ragged':>14} {'max rel-inf ragged vs loop':>28}"
    lines = [f"device: {torch.cuda.get_device_name(0)}; Generator(80, 32, 3) and AutoVC(44, 256, 512, {FREQ}) det_init, bf16; "
             f"{args.n} utterances of {min(lens)} .. {max(lens)} frames (seed {args.seed}, uniform {args.lo} .. {args.hi}), "
             f"{frames} frames = {frames * 256 / 22050:.0f} s of audio",
             f"vocoder max_batch = {args.max_batch}, max_frames = {args.max_frames}; {args.passes} alternating passes after "
             f"one warm-up pass of each, a pass = {args.reps} ragged / {args.loop_reps} loop calls; seconds per call: median "
             "(min .. max); host mels in -> host wavs out", "", head,
             f"{'vocoder':>22} {fmt(sr):>28} {fmt(sl):>28} {sl[0] / sr[0]:>14.2f} {max(rel):>28.2e}",
             f"{'wav-to-wav total':>22} {fmt(str_):>28} {fmt(stl):>28} {stl[0] / str_[0]:>14.2f} {max(rel_t):>28.2e}",
             f"vocoder per utterance: ragged {1e3 * sr[0] / args.n:.2f} ms, loop {1e3 * sl[0] / args.n:.2f} ms; "
             f"{frames / sr[0] / 1e3:.0f} k frames/s against {frames / sl[0] / 1e3:.0f} k",
             "(wav-to-wav total: convert_whole(vocoder=...) against convert_whole followed by the loop; its ragged "
             "batches are convert_whole's own, cut to melgan.VOCODER_MAX_FRAMES)", "",
             f"the vocoder's plan: {len(plan)} batches", f"{'batch':>6} {'rows':>5} {'Tmax':>5} {'shortest':>9} {'padded frames':>14}"]
    for k, (idx, Tmax) in enumerate(plan):
        own = sum(lens[i] for i in idx)
        lines.append(f"{k:>6} {len(idx):>5} {Tmax:>5} {min(lens[i] for i in idx):>9} {1 - own / (len(idx) * Tmax):>13.1%}")
    total = sum(len(idx) * Tmax for idx, Tmax in plan)
    lines.append(f"{'all':>6} {args.n:>5} {'':>5} {'':>9} {1 - frames / total:>13.1%}")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ragged()
    torch.cuda.synchronize()
    lines.append(f"peak device memory of one inverse_ragged pass: {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB "
                 f"allocated, {torch.cuda.max_memory_reserved() / 2 ** 20:.0f} MiB reserved")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
