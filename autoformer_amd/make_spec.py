"""Waveforms -> the log-mel tree that data.py and embed.build_metadata read: the reference's
make_data/make_spec.ipynb as a tool, with the mel computed by the HIP Audio2Mel kernel.

    python -m autoformer_amd.make_spec --wav_dir D --out_dir O [--max_batch N]

walks ``D/<speaker>/*.wav`` in sorted order and writes ``O/<speaker>/<name>.npy``, each a
``(T, 80)`` float32 log-mel.  Per utterance (notebook cell `mel_gan_handler` and the loop after it):
first channel of a multi-channel file, peak normalisation ``x / max|x|`` (librosa.util.normalize;
an all-zero utterance stays zero), then Audio2Mel's chain.  The notebook names its output
``fileName[:-3]`` and lets ``np.save`` append the extension, so ``a.wav`` becomes ``a..npy``;
the names here are the same.

Wavs are read with the standard library's ``wave`` module (PCM, 16 or 32 bit, scaled to [-1, 1) as
soundfile does).  The notebook resamples every file to 22050 Hz with librosa; resampling is not
restated here, and a file at another rate is refused by name.

Utterances are batched by length (sorted, ``max_batch`` per launch), the peaks are one ``amax`` on
the device and travel to the kernel as its per-utterance ``scale``.
"""
from __future__ import annotations

import argparse
import os
import wave

import numpy as np
import torch

from .melgan import Audio2Mel, n_frames

TARGET_FS = 22050


def read_wav(path):
    """(x float32 (N,) or (N, C), fs) of a PCM 16- or 32-bit wav."""
    with wave.open(path, "rb") as w:
        nch, width, fs, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if w.getcomptype() != "NONE" or width not in (2, 4):
            raise ValueError(f"{path}: only PCM 16- or 32-bit wavs are read (sample width {width}, "
                             f"compression {w.getcomptype()})")
        raw = w.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    else:
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    return (x.reshape(-1, nch) if nch > 1 else x), fs


def wav_info(path):
    """(samples per channel, fs) from the header alone."""
    with wave.open(path, "rb") as w:
        return w.getnframes(), w.getframerate()


def first_channel(x):
    x = np.asarray(x)
    return x[:, 0] if x.ndim > 1 else x


def check_rate(fs, name="input"):
    if int(fs) != TARGET_FS:
        raise ValueError(f"{name}: sampling rate {fs} Hz, expected {TARGET_FS} Hz (resampling is not part of this "
                         "tool; resample the file first)")


def out_name(file_name):
    """The notebook's np.save(fileName[:-3]) -> 'a.wav' is saved as 'a..npy'."""
    return file_name[:-3] + ".npy"


def plan_batches(lengths, max_batch):
    """Index lists: utterances sorted by length (ties by index), max_batch to a launch, so a batch pads
    each row only up to its longest neighbour in length."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    return [order[i:i + max_batch] for i in range(0, len(order), max_batch)]


def mels_of(a2m, waves):
    """Peak-normalised log-mels [(T_i, n_mel) float32] of a list of 1-D float32 waveforms: one launch."""
    dev = a2m.mel_basis.device
    lens = [int(w.shape[0]) for w in waves]
    host = np.zeros((len(waves), max(lens)), dtype=np.float32)
    for i, w in enumerate(waves):
        host[i, :lens[i]] = w
    buf = torch.from_numpy(host).to(dev)
    peak = buf.abs().amax(dim=1)  # the zero padding cannot raise a peak
    scale = torch.where(peak > 0, 1.0 / peak, torch.ones_like(peak))
    out = a2m.frames(buf, lens=lens, scale=scale).cpu().numpy()
    return [np.ascontiguousarray(out[i, :n_frames(lens[i])]) for i in range(len(waves))]


def wav_to_mel(x, fs, a2m=None, device="cuda:0"):
    """One utterance: x (N,) or (N, C) samples at fs = 22050 Hz -> (T, 80) float32 log-mel."""
    check_rate(fs)
    a2m = Audio2Mel().to(device) if a2m is None else a2m
    return mels_of(a2m, [np.ascontiguousarray(first_channel(x), dtype=np.float32)])[0]


def list_wavs(wav_dir):
    """[(speaker, file name)] of wav_dir/<speaker>/*.wav, speakers and files sorted."""
    found = []
    for spk in sorted(d for d in os.listdir(wav_dir) if os.path.isdir(os.path.join(wav_dir, d))):
        for fn in sorted(os.listdir(os.path.join(wav_dir, spk))):
            if fn.lower().endswith(".wav") and os.path.isfile(os.path.join(wav_dir, spk, fn)):
                found.append((spk, fn))
    return found


def convert_tree(wav_dir, out_dir, max_batch=32, device="cuda:0", a2m=None, mels_fn=mels_of):
    """Convert every wav of the tree; returns the written paths in input order.  Every header is
    checked (rate, length) before anything is computed or written."""
    files = list_wavs(wav_dir)
    lengths = []
    for spk, fn in files:
        n, fs = wav_info(os.path.join(wav_dir, spk, fn))
        check_rate(fs, os.path.join(spk, fn))
        try:
            n_frames(n)
        except ValueError as e:
            raise ValueError(f"{os.path.join(spk, fn)}: {e}") from None
        lengths.append(n)
    if a2m is None and files:
        a2m = Audio2Mel().to(device)
    written = [None] * len(files)
    for batch in plan_batches(lengths, max_batch):
        waves = []
        for i in batch:
            spk, fn = files[i]
            x, _ = read_wav(os.path.join(wav_dir, spk, fn))
            waves.append(np.ascontiguousarray(first_channel(x), dtype=np.float32))
        for i, mel in zip(batch, mels_fn(a2m, waves)):
            spk, fn = files[i]
            os.makedirs(os.path.join(out_dir, spk), exist_ok=True)
            path = os.path.join(out_dir, spk, out_name(fn))
            with open(path, "wb") as f:  # an open file: np.save appends nothing to the name
                np.save(f, mel.astype(np.float32), allow_pickle=False)
            written[i] = path
    return written


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--wav_dir", required=True, help="root of <speaker>/*.wav")
    ap.add_argument("--out_dir", required=True, help="root of the <speaker>/<name>.npy tree to write")
    ap.add_argument("--max_batch", type=int, default=32, help="utterances per launch")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    if not torch.cuda.is_available() or torch.device(args.device).type != "cuda":
        raise SystemExit("make_spec needs the HIP device (there is no CPU path)")
    written = convert_tree(args.wav_dir, args.out_dir, args.max_batch, args.device)
    print(f"wrote {len(written)} mels under {args.out_dir}")


if __name__ == "__main__":
    main()
