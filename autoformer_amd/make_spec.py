"""Waveforms -> the log-mel tree that data.py and embed.build_metadata read: the reference's
make_data/make_spec.ipynb as a tool, with the mel computed by the HIP Audio2Mel kernel.

    python -m autoformer_amd.make_spec --wav_dir D --out_dir O [--max_batch N] [--resample]

walks ``D/<speaker>/*.wav`` in sorted order and writes ``O/<speaker>/<name>.npy``, each a
``(T, 80)`` float32 log-mel.  Per utterance (notebook cell `mel_gan_handler` and the loop after it):
first channel of a multi-channel file, peak normalisation ``x / max|x|`` (librosa.util.normalize;
an all-zero utterance stays zero), then Audio2Mel's chain.  The notebook names its output
``fileName[:-3]`` and lets ``np.save`` append the extension, so ``a.wav`` becomes ``a..npy``;
the names here are the same.

Wavs are read with the standard library's ``wave`` module (PCM, 16 or 32 bit, scaled to [-1, 1) as
soundfile does).  The notebook resamples every file to 22050 Hz with ``librosa.resample`` before the
peak normalisation.  That step is opt-in here: with ``--resample`` (``resample=True``) a file at another
rate goes through the HIP converter of ``autoformer_amd.resample`` first (resampy's kaiser_best
interpolator as a polyphase FIR, one launch per batch); without it, the default, such a file is refused
by name before anything is written.

Utterances are batched by length (sorted, ``max_batch`` per launch), the peaks are one ``amax`` on
the device and travel to the kernel as its per-utterance ``scale``.  With ``--resample`` the files are
grouped by source rate first (a batch never mixes rates: one table, one resampling launch), the
lengths that plan the batches and decide "too short" are the resampled ones, and the peak is taken on
the resampled buffer, whose pad sample and zero padding cannot raise it.
"""
from __future__ import annotations

import argparse
import os
import wave

import numpy as np
import torch

from .melgan import Audio2Mel, n_frames
from .resample import TARGET_FS, Resample, out_len


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


def pack_rows(waves, device):
    """(buf (B, max len) float32 on the device, zero padded; lens) of a list of 1-D float32 waveforms."""
    lens = [int(w.shape[0]) for w in waves]
    host = np.zeros((len(waves), max(lens)), dtype=np.float32)
    for i, w in enumerate(waves):
        host[i, :lens[i]] = w
    return torch.from_numpy(host).to(device), lens


def mels_of(a2m, waves, lens=None):
    """Peak-normalised log-mels [(T_i, n_mel) float32]: one launch.  waves: a list of 1-D float32
    waveforms, or (with lens) a (B, stride) device buffer whose row i holds lens[i] samples and zeros
    after them, as resample_waves returns it."""
    buf, lens = pack_rows(waves, a2m.mel_basis.device) if lens is None else (waves, [int(n) for n in lens])
    peak = buf.abs().amax(dim=1)  # the zero padding cannot raise a peak
    scale = torch.where(peak > 0, 1.0 / peak, torch.ones_like(peak))
    out = a2m.frames(buf, lens=lens, scale=scale).cpu().numpy()
    return [np.ascontiguousarray(out[i, :n_frames(lens[i])]) for i in range(len(lens))]


_RESAMPLERS = {}


def resample_waves(fs, waves, device):
    """A list of 1-D float32 waveforms at fs Hz -> (buf (B, max out_len) on the device at 22050 Hz,
    out_lens): one launch of the HIP converter (autoformer_amd.resample)."""
    fs = int(fs)
    if fs not in _RESAMPLERS:
        _RESAMPLERS[fs] = Resample(fs, TARGET_FS)
    buf, lens = pack_rows(waves, device)
    return _RESAMPLERS[fs].frames(buf, lens=lens)


def wav_to_mel(x, fs, a2m=None, device="cuda:0", resample=False):
    """One utterance: x (N,) or (N, C) samples at fs Hz -> (T, 80) float32 log-mel.  fs must be 22050
    unless resample is set, in which case another rate is converted first."""
    if not resample:
        check_rate(fs)
    a2m = Audio2Mel().to(device) if a2m is None else a2m
    wave_ = np.ascontiguousarray(first_channel(x), dtype=np.float32)
    if int(fs) == TARGET_FS:
        return mels_of(a2m, [wave_])[0]
    n_frames(out_len(wave_.shape[0], fs, TARGET_FS))   # too short after resampling: refused before any launch
    buf, lens = resample_waves(fs, [wave_], a2m.mel_basis.device)
    return mels_of(a2m, buf, lens)[0]


def list_wavs(wav_dir):
    """[(speaker, file name)] of wav_dir/<speaker>/*.wav, speakers and files sorted."""
    found = []
    for spk in sorted(d for d in os.listdir(wav_dir) if os.path.isdir(os.path.join(wav_dir, d))):
        for fn in sorted(os.listdir(os.path.join(wav_dir, spk))):
            if fn.lower().endswith(".wav") and os.path.isfile(os.path.join(wav_dir, spk, fn)):
                found.append((spk, fn))
    return found


def convert_tree(wav_dir, out_dir, max_batch=32, device="cuda:0", a2m=None, mels_fn=mels_of, resample=False,
                 resample_fn=resample_waves):
    """Convert every wav of the tree; returns the written paths in input order.  Every header is
    checked (rate, length) before anything is computed or written.  resample: files at another rate
    than 22050 Hz are converted (resample_fn(fs, waves, device) -> (device buffer, resampled lengths),
    handed on as mels_fn(a2m, buffer, lengths)) instead of refused; batches are planned per source
    rate, on the resampled lengths."""
    files = list_wavs(wav_dir)
    lengths, rates = [], []
    for spk, fn in files:
        n, fs = wav_info(os.path.join(wav_dir, spk, fn))
        if not resample:
            check_rate(fs, os.path.join(spk, fn))
        try:
            n = out_len(n, fs, TARGET_FS) if int(fs) != TARGET_FS else n
            n_frames(n)
        except ValueError as e:
            at = "" if int(fs) == TARGET_FS else f" (after resampling {fs} -> {TARGET_FS} Hz)"
            raise ValueError(f"{os.path.join(spk, fn)}: {e}{at}") from None
        lengths.append(n)
        rates.append(int(fs))
    if a2m is None and files:
        a2m = Audio2Mel().to(device)
    written = [None] * len(files)
    batches = []  # (source rate, indices): a batch never mixes rates
    for fs in sorted(set(rates)):
        group = [i for i in range(len(files)) if rates[i] == fs]
        batches += [(fs, [group[k] for k in b]) for b in plan_batches([lengths[i] for i in group], max_batch)]
    for fs, batch in batches:
        waves = []
        for i in batch:
            spk, fn = files[i]
            x, _ = read_wav(os.path.join(wav_dir, spk, fn))
            waves.append(np.ascontiguousarray(first_channel(x), dtype=np.float32))
        if fs == TARGET_FS:
            mels = mels_fn(a2m, waves)
        else:
            buf, out_lens = resample_fn(fs, waves, getattr(getattr(a2m, "mel_basis", None), "device", device))
            if [int(n) for n in out_lens] != [lengths[i] for i in batch]:
                raise RuntimeError(f"resample_fn returned lengths {list(out_lens)} for {fs} Hz, expected "
                                   f"{[lengths[i] for i in batch]}")
            mels = mels_fn(a2m, buf, out_lens)
        for i, mel in zip(batch, mels):
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
    ap.add_argument("--resample", action="store_true",
                    help="convert files at another rate to 22050 Hz on the device instead of refusing them")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    if not torch.cuda.is_available() or torch.device(args.device).type != "cuda":
        raise SystemExit("make_spec needs the HIP device (there is no CPU path)")
    written = convert_tree(args.wav_dir, args.out_dir, args.max_batch, args.device, resample=args.resample)
    print(f"wrote {len(written)} mels under {args.out_dir}")


if __name__ == "__main__":
    main()
