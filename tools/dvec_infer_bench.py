"""A/B of the LstmDV embedding paths on one device (profiles/dvec_infer_ab.txt):

  train   the training composition under torch.no_grad() (everything kept for a backward)
  rows8   the forward-only recurrence (avc_lstm_infer), 8 utterances per group
  rows16  the same with 16 utterances per group

For each (B, T): utterances per second (median and min..max over the rounds; the paths alternate
inside every round, so drift on a shared host hits all three alike) and the peak of
torch.cuda.max_memory_allocated over one call (weights and packs included, the same for all
paths), plus the rel-inf distance of each inference path's embeddings from the training
composition's.  bf16 compute, closed-form weights.

  python tools/dvec_infer_bench.py [--rounds 5] [--window 0.4]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SHAPES = [(1, 176), (64, 176), (160, 176)]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window", type=float, default=0.4, help="seconds of work per timed window")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dvec_infer_bench: needs the GPU (no CPU fallback)")
    import autoformer_amd as A
    from autoformer_amd import kernels as K
    from autoformer_amd.detinit import det_init_, det_inputs
    from autoformer_amd.factory.LstmDV import LstmDV

    A.set_compute("bf16")
    dev = torch.device("cuda:0")
    m = LstmDV()
    det_init_(m)
    m = m.to(dev).eval()
    H = m.lstm.hidden_size

    def run(path, x, B, T):
        mel = x.reshape(B * T, 80)
        if path == "train":
            return m._train_form(mel, B, T, None)
        m.infer_rows = 8 if path == "rows8" else 16
        return m._infer_form(mel, B, T, None)

    print(f"device {torch.cuda.get_device_name(0)}, CUs {K.num_cus()}, rounds {args.rounds}, window {args.window} s")
    print(f"{'B':>4} {'T':>4} {'path':>7} {'utt/s median':>13} {'min':>9} {'max':>9} {'peak MiB':>9} {'rel-inf vs train':>17}")
    with torch.no_grad():
        for B, T in SHAPES:
            x = torch.from_numpy(det_inputs(B, T)[0]).to(dev)
            paths = ["train"] + [n for n, r in (("rows8", 8), ("rows16", 16)) if K.lstm_infer_persistent(B, H, r)]
            iters, peak, out = {}, {}, {}
            for path in paths:  # warm-up, the window's iteration count, the peak of one call
                for _ in range(3):
                    out[path] = run(path, x, B, T)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    run(path, x, B, T)
                torch.cuda.synchronize()
                iters[path] = max(5, int(args.window / ((time.perf_counter() - t0) / 5)))
                torch.cuda.reset_peak_memory_stats()
                run(path, x, B, T)
                torch.cuda.synchronize()
                peak[path] = torch.cuda.max_memory_allocated() / 2 ** 20
            K.check_faults()
            rates = {path: [] for path in paths}
            for _ in range(args.rounds):
                for path in paths:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters[path]):
                        run(path, x, B, T)
                    torch.cuda.synchronize()
                    rates[path].append(B * iters[path] / (time.perf_counter() - t0))
            K.check_faults()
            ref = out["train"].float().cpu().numpy()
            for path in ("train", "rows8", "rows16"):
                if path not in paths:
                    print(f"{B:>4} {T:>4} {path:>7} {'not admitted (grid > CUs)':>33}")
                    continue
                r = rates[path]
                d = np.abs(out[path].float().cpu().numpy() - ref).max() / np.abs(ref).max()
                print(f"{B:>4} {T:>4} {path:>7} {statistics.median(r):>13.1f} {min(r):>9.1f} {max(r):>9.1f} "
                      f"{peak[path]:>9.1f} {d:>17.3e}")
    m.infer_rows = 0


if __name__ == "__main__":
    main()
