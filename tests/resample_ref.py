"""fp64 numpy restatement of the band-limited sample-rate converter (librosa.resample with the
notebook-era res_type='kaiser_best', i.e. resampy's windowed-sinc interpolator), written from the
operator's text and from nothing in autoformer_amd: one loop per OUTPUT sample over the right half of
the filter table with the `eta` interpolation, no polyphase table.

Neither librosa nor resampy runs where this suite does, so the FORMULA is pinned, not a library's
bits.

  table   num_zeros = 64, 512 samples per zero crossing, n = 512 * 64
          win[i]   = rolloff * sinc(rolloff * i / 512) * kaiser(2n + 1, beta)[n + i],  i = 0 .. n
          delta[i] = win[i + 1] - win[i], delta[n] = 0;  both times ratio when ratio < 1
  setup   L / M = fs_out / fs_in reduced, scale = min(1, L / M), step = int(scale * 512) (truncated)
  y[t]    n = (t M) div L, frac = scale * ((t M) mod L) / L
          left  wing: off = int(frac * 512), eta = frac * 512 - off,
                      i < min(n + 1, (32769 - off) div step):        (win + eta delta)[off + i step] * x[n - i]
          right wing: the same from frac' = scale - frac,
                      k < min(N - n - 1, (32769 - off) div step):    (win + eta delta)[off + k step] * x[n + 1 + k]
  length  ceil(N L / M); resampy fills floor(N L / M) samples, so the last one is 0.0 when M does not
          divide N L.

The wing bound is resampy's integer form `(nwin - off) // step`: a tap is taken while
off + (i + 1) step <= 32769, one tap per wing fewer than `off + i step < 32769` would take.  It is what
gives 277 taps at 48000 -> 22050 (127 at 16000, 255 at 44100, 559 at 96000).
"""
import math

import numpy as np

NUM_ZEROS, NUM_TABLE = 64, 512
BETA, ROLLOFF = 14.769656459379492, 0.9475937167399596
NWIN = NUM_ZEROS * NUM_TABLE + 1


def half_table():
    """(win, delta) fp64, NWIN = 32769 entries each, before the ratio factor."""
    n = NUM_ZEROS * NUM_TABLE
    i = np.arange(n + 1, dtype=np.float64)
    win = ROLLOFF * np.sinc(ROLLOFF * i / NUM_TABLE) * np.kaiser(2 * n + 1, BETA)[n:]
    delta = np.zeros(n + 1, dtype=np.float64)
    delta[:-1] = win[1:] - win[:-1]
    return win, delta


def setup(fs_in, fs_out):
    g = math.gcd(int(fs_in), int(fs_out))
    L, M = int(fs_out) // g, int(fs_in) // g
    scale = min(1.0, L / M)
    return L, M, scale, int(scale * NUM_TABLE)


def out_len(N, fs_in, fs_out):
    L, M, _, _ = setup(fs_in, fs_out)
    return -((-N * L) // M)


def resample(x, fs_in, fs_out):
    """x (N,) -> fp64 (ceil(N L / M),)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    L, M, scale, step = setup(fs_in, fs_out)
    win, delta = half_table()
    if L < M:
        win, delta = win * (L / M), delta * (L / M)
    y = np.zeros(out_len(N, fs_in, fs_out), dtype=np.float64)
    for t in range((N * L) // M):
        n, p = divmod(t * M, L)
        frac = scale * (p / L)
        off = int(frac * NUM_TABLE)
        eta = frac * NUM_TABLE - off
        idx = off + step * np.arange(min(n + 1, (NWIN - off) // step))
        acc = np.dot(win[idx] + eta * delta[idx], x[n - np.arange(idx.size)]) if idx.size else 0.0
        frac = scale - frac
        off = int(frac * NUM_TABLE)
        eta = frac * NUM_TABLE - off
        idx = off + step * np.arange(max(0, min(N - n - 1, (NWIN - off) // step)))
        if idx.size:
            acc += np.dot(win[idx] + eta * delta[idx], x[n + 1 + np.arange(idx.size)])
        y[t] = acc
    return y


def kaiser_sinc(u):
    """The continuous filter the table samples, at u in zero crossings: rolloff sinc(rolloff u) times the
    Kaiser window I0(beta sqrt(1 - (u/64)^2)) / I0(beta), 0 outside |u| <= 64."""
    u = np.abs(np.asarray(u, dtype=np.float64))
    inside = u <= NUM_ZEROS
    w = np.i0(BETA * np.sqrt(np.clip(1.0 - (u / NUM_ZEROS) ** 2, 0.0, None))) / np.i0(BETA)
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * u) * w, 0.0)


def closed_form(x, fs_in, fs_out):
    """y[t] = min(1, ratio) * sum_m x[m] h(scale (t M / L - m)), h the continuous filter: no table, no
    interpolation.  Every sample with |u| <= 64 is taken, so the last tap of a wing, which the table form
    drops, is in: |h| < 3e-8 there."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    L, M, scale, step = setup(fs_in, fs_out)
    assert scale * NUM_TABLE == step, "the closed form equals the table form only where the step is not truncated"
    y = np.zeros(out_len(N, fs_in, fs_out), dtype=np.float64)
    m = np.arange(N)
    for t in range((N * L) // M):
        n, p = divmod(t * M, L)
        y[t] = scale * np.dot(kaiser_sinc(scale * (n + p / L - m)), x)
    return y


def signals(N, fs_in):
    """name -> fp32 input of N samples: the inputs of the resampler's tests."""
    rng = np.random.RandomState(1000 + N)
    s = {"zeros": np.zeros(N), "const": np.full(N, 0.5), "noise": 0.1 * rng.randn(N),
         "sine1k": np.sin(2 * np.pi * 1000.0 * np.arange(N) / fs_in)}
    for name, at in (("imp_first", 0), ("imp_last", N - 1), ("imp_mid", N // 2)):
        s[name] = np.zeros(N)
        s[name][at] = 1.0
    return {k: v.astype(np.float32) for k, v in s.items()}
