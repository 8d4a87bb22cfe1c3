"""Band-limited sample-rate conversion on the HIP path: the `librosa.resample(x, fs, 22050)` of the
reference's make_data/make_spec.ipynb (notebook-era default res_type='kaiser_best', i.e. resampy's
Kaiser-windowed sinc interpolator), as the exact polyphase FIR it is.

resampy walks a table of the filter's right half -- 64 zero crossings, 512 samples each, Kaiser
beta 14.7697, roll-off 0.9476 -- with linear interpolation between entries.  For a reduced pair
fs_out / fs_in = L / M the table positions of output t depend only on r = t mod L, so the weights
are tabulated once per rate pair (fp64, rounded once to fp32) as W[tap][r] and one kernel
(resample.hip, include/autovc_hip_resample.h) applies them.  What the library does is kept as it
is, quirks included:

  * the table step is int(min(1, L/M) * 512): 235 at 48000 -> 22050, not 235.2, so the filter is
    slightly stretched and its DC gain is about 1.00047;
  * a wing ends at (32769 - off) // step taps (one short of the table's last reachable entry);
  * there is no gain rescale, and the output has ceil(N L / M) samples of which resampy fills
    floor(N L / M): the last one is 0.0 when M does not divide N L (librosa's fix_length pad).

    rs = Resample(48000)                      # -> 22050 Hz
    out, out_lens = rs.frames(audio, lens)    # (B, stride) fp32 on the device -> (B, max out_len)

There is no CPU or torch fallback: the kernel raises on host tensors.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

TARGET_FS = 22050
NUM_ZEROS, NUM_TABLE = 64, 512          # zero crossings of a wing; table samples per zero crossing (precision 9)
BETA, ROLLOFF = 14.769656459379492, 0.9475937167399596   # resampy's kaiser_best
NWIN = NUM_ZEROS * NUM_TABLE + 1


def rate_pair(fs_in, fs_out=TARGET_FS):
    """(L, M) with fs_out / fs_in = L / M in lowest terms."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError(f"resample: sampling rates must be positive, got {fs_in} -> {fs_out}")
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def out_len(N, fs_in, fs_out=TARGET_FS):
    """ceil(N L / M): the length librosa.resample returns."""
    Lr, M = rate_pair(fs_in, fs_out)
    return -((-int(N) * Lr) // M)


@functools.lru_cache(maxsize=None)
def _half_window():
    """The table's right half in fp64: win[i] = rolloff sinc(rolloff i / 512) kaiser(i / n), i = 0 .. n."""
    n = NUM_ZEROS * NUM_TABLE
    i = np.arange(n + 1, dtype=np.float64)
    kaiser = np.i0(BETA * np.sqrt(1.0 - (i / n) ** 2)) / np.i0(BETA)   # np.kaiser(2n + 1, beta)[n + i]
    return ROLLOFF * np.sinc(ROLLOFF * i / NUM_TABLE) * kaiser


class Table:
    """The polyphase form of one rate pair.  weights64 / weights: (taps, L) fp64 / fp32, tap-major;
    table: (L, 3) int32 rows (offset, first tap, count): output t = j L + r is
    sum_{k in [first, first + count)} weights[k, r] * x[j M + offset + k]."""

    def __init__(self, fs_in, fs_out):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M = rate_pair(fs_in, fs_out)
        ratio = self.L / self.M
        self.scale = min(1.0, ratio)
        self.step = int(self.scale * NUM_TABLE)
        if self.step < 1:
            raise ValueError(f"resample: {fs_in} -> {fs_out} Hz: the table step int({self.scale:.3g} * {NUM_TABLE}) "
                             "is 0 (the ratio is too steep for the filter table)")
        # a wing has at most (NWIN - off) // step taps with off >= 0; the left one at off = 0 reaches it
        bound = 2 * (NWIN // self.step)
        if bound * self.L > 2 * L.RESAMPLE_MAX_WEIGHTS:   # far above the cap: do not build it to find out
            self._refuse(bound * self.L, "about ")
        win = _half_window()
        if ratio < 1:
            win = win * ratio
        delta = np.zeros_like(win)
        delta[:-1] = win[1:] - win[:-1]
        cols, rows = [], []
        for r in range(self.L):
            q, p = divmod(r * self.M, self.L)
            wings = []
            for frac in (self.scale * (p / self.L), self.scale - self.scale * (p / self.L)):
                off = int(frac * NUM_TABLE)
                eta = frac * NUM_TABLE - off
                idx = off + self.step * np.arange((NWIN - off) // self.step)
                wings.append(win[idx] + eta * delta[idx])
            left, right = wings           # left[i] weighs x[n - i], right[k] weighs x[n + 1 + k]
            cols.append(np.concatenate((left[::-1], right)))
            rows.append((q - (left.size - 1), 0, left.size + right.size))
        self.taps = max(c.size for c in cols)
        if self.taps * self.L > L.RESAMPLE_MAX_WEIGHTS:
            self._refuse(self.taps * self.L)
        self.weights64 = np.zeros((self.taps, self.L), dtype=np.float64)
        for r, c in enumerate(cols):
            self.weights64[:c.size, r] = c
        self.weights = self.weights64.astype(np.float32)
        self.table = np.asarray(rows, dtype=np.int32)
        self._host = (L.c_int * self.table.size)(*[int(v) for v in self.table.reshape(-1)])
        self._dev = {}

    def _refuse(self, n, about=""):
        raise ValueError(f"resample: {self.fs_in} -> {self.fs_out} Hz reduces to L / M = {self.L} / {self.M}; its "
                         f"polyphase table has {about}{n} weights, more than the {L.RESAMPLE_MAX_WEIGHTS} of "
                         "AVC_RESAMPLE_MAX_WEIGHTS (a rate pair with a large reduced L, or a steep downsampling, is "
                         "not supported)")

    @property
    def n_weights(self):
        return self.taps * self.L

    def tile(self):
        """Output samples per workgroup of the kernel for this pair (host arithmetic of the library)."""
        n = L.lib().avc_resample_tile(self.L, self.M, self.taps)
        if n < 0:
            L.check(n, "avc_resample_tile")
        return n

    def on(self, device):
        """(host int table, device int table, device weights) -- uploaded once per device."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (self._host, torch.from_numpy(self.table.reshape(-1).copy()).to(device),
                              torch.from_numpy(self.weights.reshape(-1).copy()).to(device))
        return self._dev[key]


@functools.lru_cache(maxsize=None)
def _table(fs_in, fs_out):
    return Table(fs_in, fs_out)


def resample_table(fs_in, fs_out=TARGET_FS, device=None):
    """The polyphase Table of a rate pair, built once per pair (host fp64 -> fp32); with `device`, its
    device copies are made (once per device) as well."""
    t = _table(int(fs_in), int(fs_out))
    if device is not None:
        t.on(device)
    return t


class Resample:
    """fs_in -> fs_out Hz.  frames(audio (B, stride) fp32 on the device | list of 1-D tensors, lens=None)
    -> (out (B, max out_len) fp32, out_lens): row b holds out_len(lens[b]) samples and 0.0 after them.
    fs_in == fs_out returns the input rows unchanged, with no launch."""

    def __init__(self, fs_in, fs_out=TARGET_FS):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M = rate_pair(fs_in, fs_out)
        self.bypass = self.L == self.M
        self.table = None if self.bypass else resample_table(fs_in, fs_out)
        self._lens = None

    def out_len(self, N):
        return out_len(N, self.fs_in, self.fs_out)

    @torch.no_grad()
    def frames(self, audio, lens=None):
        if isinstance(audio, (list, tuple)):
            if lens is not None:
                raise ValueError("Resample.frames: a list of utterances carries its own lengths")
            if not audio:
                raise ValueError("Resample.frames: an empty list")
            lens = [int(a.numel()) for a in audio]
            buf = torch.zeros(len(audio), max(max(lens), 1), device=audio[0].device)
            for b, a in enumerate(audio):
                buf[b, :lens[b]] = a.reshape(-1)
            audio = buf
        if audio.dim() != 2 or audio.dtype != torch.float32:
            raise ValueError(f"Resample: expected fp32 audio (B, stride), got {tuple(audio.shape)} {audio.dtype}")
        B, stride = audio.shape
        lens = [stride] * B if lens is None else [int(v) for v in lens]
        if len(lens) != B:
            raise ValueError(f"Resample: lens must hold B={B} values")
        if B < 1 or min(lens) < 1:
            raise ValueError("Resample: an utterance has at least one sample")
        if max(lens) > stride:
            raise ValueError(f"Resample: lens {max(lens)} exceeds the {stride} samples of a row")
        if self.bypass:
            return audio, lens
        K._dev(audio)
        audio = audio.contiguous()
        out_lens = [self.out_len(n) for n in lens]
        host, tab, wts = self.table.on(audio.device)
        lkey = (tuple(lens), str(audio.device))
        if self._lens is None or self._lens[0] != lkey:  # the same lengths again: no second upload
            self._lens = (lkey, (L.c_int * B)(*lens), torch.tensor(lens, dtype=torch.int32, device=audio.device))
        _, lens_host, lens_dev = self._lens
        out = torch.empty(B, max(out_lens), device=audio.device)
        L.call("avc_resample", audio.data_ptr(), stride, lens_host, lens_dev.data_ptr(), B, wts.data_ptr(),
               self.table.n_weights, host, tab.data_ptr(), self.L, self.M, self.table.taps, out.data_ptr(),
               out.shape[1], K.stream())
        return out, out_lens
