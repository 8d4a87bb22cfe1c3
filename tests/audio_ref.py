"""fp64 numpy restatement of the waveform -> log-mel chain (reference melgan/modules.py:26-69 and the
mel_gan_handler cell of make_data/make_spec.ipynb), and the test signals of the audio tests.

Nothing here comes from autoformer_amd: the filterbank below is written on its own (a loop over
triangles on the Slaney scale, not the product's vectorised form), so that the two can be held
against each other and against the closed-form invariants of tests/test_audio.py.  Those invariants
pin the FORMULA (Slaney scale, triangles, area normalisation); they are not librosa's bits: librosa
is not available where this suite runs, and neither is the reference's own Audio2Mel (its
`torch.stft` call without `return_complex` no longer exists), so no fixture comes from either.
"""
import math

import numpy as np

N_FFT, HOP, N_BINS, PAD, CLAMP = 1024, 256, 513, 384, 1e-5


def hz_to_mel(hz):
    if hz < 1000.0:
        return hz / (200.0 / 3.0)
    return 15.0 + math.log(hz / 1000.0) * 27.0 / math.log(6.4)


def mel_to_hz(mel):
    if mel < 15.0:
        return mel * (200.0 / 3.0)
    return 1000.0 * math.exp((mel - 15.0) * math.log(6.4) / 27.0)


def mel_basis(sr=22050, n_fft=1024, n_mels=80, fmin=0.0, fmax=None, dtype=np.float32):
    fmax = sr / 2.0 if fmax is None else fmax
    lo, hi = hz_to_mel(fmin), hz_to_mel(fmax)
    pts = [mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    W = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        for k in range(n_fft // 2 + 1):
            fk = k * sr / n_fft
            if left < fk <= centre:
                W[m, k] = (fk - left) / (centre - left)
            elif centre < fk < right:
                W[m, k] = (right - fk) / (right - centre)
        W[m] *= 2.0 / (right - left)
    return W.astype(dtype)


def n_frames(L):
    return (L + 2 * PAD - N_FFT) // HOP + 1


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def magnitudes(x, window=None):
    """(T, 513) fp64 |rfft| of the windowed frames of the reflect-padded x."""
    x = np.asarray(x, dtype=np.float64)
    window = hann_periodic() if window is None else np.asarray(window, dtype=np.float64)
    xp = np.pad(x, (PAD, PAD), mode="reflect")
    T = n_frames(x.shape[0])
    frames = np.stack([xp[HOP * t:HOP * t + N_FFT] * window for t in range(T)])
    return np.abs(np.fft.rfft(frames, axis=1))


def linear_mel(x, basis=None, window=None):
    """(T, n_mel) fp64 mel, before the clamp and the log."""
    basis = mel_basis(dtype=np.float64) if basis is None else np.asarray(basis, dtype=np.float64)
    return magnitudes(x, window) @ basis.T


def log_mel(x, basis=None, window=None):
    return np.log10(np.maximum(linear_mel(x, basis, window), CLAMP))


def peak_normalise(x):
    """librosa.util.normalize's default (norm=inf) on a 1-D signal: x / max|x|, zeros left as they are."""
    x = np.asarray(x, dtype=np.float64)
    peak = np.abs(x).max()
    return x / peak if peak > 0 else x


def frame_error(out_log, r):
    """The audio tests' metric: per frame, max_m |max(10^out, 1e-5) - max(r, 1e-5)| / max(max_m r, 1e-5),
    linear and relative to the frame's peak.  out_log (T, n_mel) log10 mel, r (T, n_mel) fp64 linear mel."""
    lin = np.maximum(np.power(10.0, np.asarray(out_log, dtype=np.float64)), CLAMP)
    rr = np.maximum(r, CLAMP)
    return np.abs(lin - rr).max(axis=1) / np.maximum(r.max(axis=1), CLAMP)


def signals():
    """name -> fp32 waveform: the smallest inputs at which the chain can still go wrong."""
    rng = np.random.RandomState(7)
    n = np.arange(4096, dtype=np.float64)
    sr = 22050.0
    imp = np.zeros(4096)
    imp[1000] = 1.0
    s = {
        "one_frame": 0.1 * rng.randn(385),                      # both reflections inside the one frame
        "ragged": 0.1 * rng.randn(3 * 256 + 17),                # the tail is dropped, T = 3
        "noise": 0.1 * rng.randn(4096),
        "sine440": np.sin(2 * np.pi * 440.0 * n / sr),
        "two_tone": np.sin(2 * np.pi * 300.0 * n / sr) + 1e-3 * np.sin(2 * np.pi * 5000.0 * n / sr),
        "impulse": imp,
        "zeros": np.zeros(4096),
        "const": np.full(4096, 0.5),
        "odd_groups": 0.1 * rng.randn(11 * 256 + 5),            # T = 11: one full group of 8 frames and 3 more
    }
    return {k: v.astype(np.float32) for k, v in s.items()}
