"""MelGAN vocoder generator on the HIP path (the conversion path's mel ->
waveform step, reference melgan/modules.py:88-131 `Generator`, melgan/interface.py:23-53
`MelVocoder.inverse`, called by util/evaluate.py:96-98 `get_wavs`).

Drop-in: `Generator(input_size, ngf, n_residual_layers)` builds the reference's module tree
(ReflectionPad1d / weight-normed Conv1d / LeakyReLU / weight-normed ConvTranspose1d /
ResnetBlock, modules.py:72-86,88-131) only as the parameter container, so `state_dict()` keys
and shapes are the reference's (`model.1.weight_g`, `model.4.block.2.weight_v`,
`model.21.shortcut.bias`, ...) and a reference checkpoint loads unchanged.  `forward(mel)`
never runs those submodules: it runs frame-major HIP kernels (melgan.hip + avc_gemm):

  conv_in     mg_gather (reflect 3, 7 taps) -> GEMM 80*7 -> 512
  upsample r  LeakyReLU twin -> ONE GEMM over the zero-padded 3-tap window, N = r*Cout
              (polyphase ConvTranspose1d, avc_mg_wn_pack): its [B*L][r*Cout] output is the
              upsampled [B*L*r][Cout] sequence
  ResnetBlock mg_gather (reflect d, dilation d = 1, 3, 9, LeakyReLU) -> GEMM 3C -> C ->
              LeakyReLU twin; shortcut GEMM C -> C, then the 1x1 GEMM accumulated onto it
  conv_out    mg_conv_out (LeakyReLU, reflect 3, 7 taps, 32 -> 1, tanh)

Weight norm (g v / ||v||) is folded into the packed GEMM operands once per parameter version
(inference weights do not change between calls).  There is no CPU or torch fallback: the
kernels raise on host tensors.

`Generator.frames_ragged` / `MelVocoder.inverse_ragged` run the same sequence over utterances of
different lengths in one batch: mg_gather, the LeakyReLU twin in front of each upsampler and
mg_conv_out take the length-aware forms of melgan_ragged.hip (include/autovc_hip_vocoder.h), the
GEMMs are the same calls.

The other direction, waveform -> log-mel (reference modules.py:26-69 `Audio2Mel`, interface.py:33-41
`MelVocoder.__call__`), is `Audio2Mel` below: one fused fp32 kernel (audio.hip) behind the
reference's constructor and buffers, with the Slaney filterbank as a closed form.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from .layers import _transpose_batched

SLOPE = 0.2  # nn.LeakyReLU(0.2), modules.py:75,78,108,123
RATIOS = (8, 8, 2, 2)  # modules.py:91


def _wn(mod):
    # torch.nn.utils.weight_norm gives the reference's weight_g / weight_v keys (the
    # parametrizations API would rename them); its deprecation warning is noise here
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nn.utils.weight_norm(mod)


def WNConv1d(*args, **kwargs):
    return _wn(nn.Conv1d(*args, **kwargs))


def WNConvTranspose1d(*args, **kwargs):
    return _wn(nn.ConvTranspose1d(*args, **kwargs))


class ResnetBlock(nn.Module):
    """modules.py:72-86: shortcut(x) + [LeakyReLU, ReflectionPad(d), WNConv(k3, dilation d),
    LeakyReLU, WNConv(k1)](x) -- parameters only (see module docstring)."""

    def __init__(self, dim, dilation=1):
        super().__init__()
        self.dilation = dilation
        self.block = nn.Sequential(
            nn.LeakyReLU(SLOPE),
            nn.ReflectionPad1d(dilation),
            WNConv1d(dim, dim, kernel_size=3, dilation=dilation),
            nn.LeakyReLU(SLOPE),
            WNConv1d(dim, dim, kernel_size=1),
        )
        self.shortcut = WNConv1d(dim, dim, kernel_size=1)


def _pack(conv, stride=0, pad=0):
    """weight_norm + GEMM pack of one (transposed) conv: (W [N][K] in the compute dtype, bias)."""
    v, g = conv.weight_v.detach(), conv.weight_g.detach()
    d0, d1, k = v.shape
    dev = v.device
    tdt = K.compute_torch_dtype()
    if stride:
        w = torch.empty(stride * d1, 3 * d0, device=dev, dtype=tdt)
        bias = torch.empty(stride * d1, device=dev)
    else:
        w = torch.empty(d0, k * d1, device=dev, dtype=tdt)
        bias = None
    norms = torch.empty(d0, device=dev)
    b = conv.bias.detach() if conv.bias is not None else None
    L.call("avc_mg_wn_pack", v.contiguous().data_ptr(), g.contiguous().data_ptr(), K._ptr(b), d0, d1, k, int(stride),
           int(pad), norms.data_ptr(), w.data_ptr(), K._dt(w), K._ptr(bias), K.stream())
    return w, (bias if stride else b)


def _pack_f32(conv):
    """fp32 [taps][C] weight of the output conv (mg_conv_out reads it directly)."""
    v, g = conv.weight_v.detach(), conv.weight_g.detach()
    d0, d1, k = v.shape
    w = torch.empty(d0, k * d1, device=v.device)
    norms = torch.empty(d0, device=v.device)
    L.call("avc_mg_wn_pack", v.contiguous().data_ptr(), g.contiguous().data_ptr(), None, d0, d1, k, 0, 0,
           norms.data_ptr(), w.data_ptr(), K.F32, None, K.stream())
    return w


class Generator(nn.Module):
    """modules.py:88-131 with the reference's constructor and state_dict; forward on HIP."""

    def __init__(self, input_size, ngf, n_residual_layers):
        super().__init__()
        self.hop_length = int(np.prod(RATIOS))
        mult = int(2 ** len(RATIOS))
        model = [nn.ReflectionPad1d(3), WNConv1d(input_size, mult * ngf, kernel_size=7, padding=0)]
        self._stages = []  # (ratio, index of the ConvTranspose1d, [indices of its ResnetBlocks])
        for r in RATIOS:
            model += [nn.LeakyReLU(SLOPE),
                      WNConvTranspose1d(mult * ngf, mult * ngf // 2, kernel_size=r * 2, stride=r,
                                        padding=r // 2 + r % 2, output_padding=r % 2)]
            ct = len(model) - 1
            blocks = []
            for j in range(n_residual_layers):
                model += [ResnetBlock(mult * ngf // 2, dilation=3 ** j)]
                blocks.append(len(model) - 1)
            self._stages.append((r, ct, blocks))
            mult //= 2
        model += [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), WNConv1d(ngf, 1, kernel_size=7, padding=0), nn.Tanh()]
        self._out = len(model) - 2
        self.model = nn.Sequential(*model)
        self.input_size, self.ngf = input_size, ngf
        self._packs = None
        self._pack_key = None

    # ------------------------------------------------------------------ weight packs
    def _key(self):
        return (K.compute(),) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def packs(self):
        key = self._key()
        if self._packs is None or self._pack_key != key:
            m = self.model
            P = {"in": _pack(m[1])}
            for r, ct, blocks in self._stages:
                P[ct] = _pack(m[ct], stride=r, pad=r // 2 + r % 2)
                for bi in blocks:
                    blk = m[bi]
                    P[bi] = (_pack(blk.block[2]), _pack(blk.block[4]), _pack(blk.shortcut))
            conv = m[self._out]
            P["out"] = (_pack_f32(conv), conv.bias.detach())
            self._packs, self._pack_key = P, key
        return self._packs

    # ------------------------------------------------------------------ forward
    def _gemm(self, M, N, Kd, a, w, bias, out=None, accumulate=False):
        bf = K.compute() == K.BF16
        y = torch.empty(M, N, device=w.device) if out is None else out
        y16 = getattr(y, "_bf16", None) if out is not None else None
        if bf and y16 is None:
            y16 = torch.empty(M, N, device=w.device, dtype=torch.bfloat16)
        K.gemm(M, N, Kd, a, K.operand(w, Kd), y, bias=bias, accumulate=accumulate, c_bf16=y16 if bf else None)
        return K.attach_twin(y, y16) if bf and out is None else y

    # The three kernels that look across rows.  lens None: the rectangular forms (melgan.hip), every row
    # of the (B, Lf) block an utterance's own.  lens a kernels.Lens of MEL-frame counts: the length-aware
    # forms (melgan_ragged.hip) at this stage's cumulative upsampling `scale` (Lf = lens.T * scale).
    def _gather(self, x, B, Lf, C, taps, dil, pad, act, lens=None, scale=1):
        src = getattr(x, "_bf16", None)
        src = x if src is None else src
        Lo = Lf + 2 * pad - dil * (taps - 1)
        out = torch.empty(B * Lo, taps * C, device=x.device, dtype=K.compute_torch_dtype())
        if lens is None:
            L.call("avc_mg_gather", src.data_ptr(), K._dt(src), B, Lf, C, taps, dil, pad, 1, int(act), SLOPE,
                   out.data_ptr(), K._dt(out), K.stream())
        else:
            L.call("avc_mg_gather_ragged", src.data_ptr(), K._dt(src), B, lens.T, C, taps, dil, pad, int(act), SLOPE,
                   lens.host, lens.dev.data_ptr(), scale, out.data_ptr(), K._dt(out), K.stream())
        return out

    def _act(self, x, B=None, C=None, lens=None, scale=1):
        out = torch.empty(x.shape, device=x.device, dtype=K.compute_torch_dtype())
        bf = out.dtype == torch.bfloat16
        o32, o16 = (None, out.data_ptr()) if bf else (out.data_ptr(), None)
        if lens is None:
            L.call("avc_mg_act", x.data_ptr(), x.numel(), SLOPE, o32, o16, K.stream())
        else:
            L.call("avc_mg_act_ragged", x.data_ptr(), B, lens.T, C, SLOPE, lens.host, lens.dev.data_ptr(), scale, o32,
                   o16, K.stream())
        return out

    def _run(self, x, B, T, lens):
        """The launch sequence of frames (lens None) and frames_ragged (lens a kernels.Lens, T = lens.T)."""
        P = self.packs()
        m = self.model
        Lf, u = T, 1  # rows per utterance block at this stage, cumulative upsampling
        C = m[1].weight_v.shape[0]
        w, b = P["in"]
        g = self._gather(x.contiguous(), B, Lf, self.input_size, 7, 1, 3, act=False, lens=lens, scale=u)
        y = self._gemm(B * Lf, C, 7 * self.input_size, K.operand(g, 7 * self.input_size), w, b)
        for r, ct, blocks in self._stages:
            Cin, Cout = C, m[ct].weight_v.shape[1]
            w, b = P[ct]
            # LeakyReLU before the upsampler (modules.py:99).  Ragged: zeros past each utterance's last row, so
            # the zero-padded 3-tap window below reads after it what it reads at the block edge (and at B = 1)
            a = self._act(y, B, Cin, lens, u)
            y = self._gemm(B * Lf, r * Cout, 3 * Cin, K.operand(a, Cin, window=(3, 1, Lf, Lf, Cin)), w, b)
            Lf, C, u = Lf * r, Cout, u * r
            y16 = getattr(y, "_bf16", None)  # a view is a new tensor: carry the twin over
            y = K.attach_twin(y.view(B * Lf, C), None if y16 is None else y16.view(B * Lf, C))
            for bi in blocks:
                (w1, b1), (w2, b2), (ws, bs) = P[bi]
                d = m[bi].dilation
                h = self._gather(y, B, Lf, C, 3, d, d, act=True, lens=lens, scale=u)
                h1 = self._gemm(B * Lf, C, 3 * C, K.operand(h, 3 * C), w1, b1)
                # the rectangular twin in the ragged case too: it feeds the 1x1 GEMM, which is row-wise, so a
                # padding row of h2 reaches padding rows only (finite there: GEMM outputs of zeros and biases)
                h2 = self._act(h1)
                out = self._gemm(B * Lf, C, C, K.operand(y, C), ws, bs)  # shortcut (modules.py:83-86)
                y = self._gemm(B * Lf, C, C, K.operand(h2, C), w2, b2, out=out, accumulate=True)
        wo, bo = P["out"]
        audio = torch.empty(B * Lf, device=x.device)
        if lens is None:
            L.call("avc_mg_conv_out", y.data_ptr(), B, Lf, C, 7, wo.data_ptr(), bo.data_ptr(), SLOPE,
                   audio.data_ptr(), K.stream())
        else:
            L.call("avc_mg_conv_out_ragged", y.data_ptr(), B, lens.T, C, 7, wo.data_ptr(), bo.data_ptr(), SLOPE,
                   lens.host, lens.dev.data_ptr(), u, audio.data_ptr(), K.stream())
        return audio.view(B, Lf)

    @torch.no_grad()
    def frames(self, x, B, T):
        """x: frame-major mel (B*T, input_size) fp32 on the device -> audio (B, T*hop) fp32."""
        K._dev(x)
        if x.dtype != torch.float32 or x.shape != (B * T, self.input_size):
            raise ValueError(f"Generator.frames: expected fp32 ({B * T}, {self.input_size}), got "
                             f"{tuple(x.shape)} {x.dtype}")
        if T <= 3:
            raise ValueError("Generator: ReflectionPad1d(3) needs at least 4 mel frames (modules.py:95)")
        return self._run(x, B, T, None)

    @torch.no_grad()
    def frames_ragged(self, x, lens):
        """A batch of utterances of different lengths.  x: frame-major mel (B*Tmax, input_size) fp32 on the
        device, utterance b in rows b*Tmax .. b*Tmax + lens[b] - 1; lens: a kernels.Lens (B lengths, T =
        Tmax).  -> audio (B, Tmax*hop) fp32: audio[b, :lens[b]*hop] is frames(mel_b, 1, lens[b]), the samples
        after it are exactly 0.0.  The rows of x past an utterance's end are never read."""
        K._dev(x)
        if not isinstance(lens, K.Lens):
            raise TypeError("Generator.frames_ragged: lens must be a kernels.Lens")
        B, T = lens.B, lens.T
        if x.dtype != torch.float32 or x.shape != (B * T, self.input_size):
            raise ValueError(f"Generator.frames_ragged: expected fp32 ({B * T}, {self.input_size}), got "
                             f"{tuple(x.shape)} {x.dtype}")
        lens.check("Generator.frames_ragged", B, T, x)
        if min(lens.vals) <= 3:
            raise ValueError(f"Generator: ReflectionPad1d(3) needs at least 4 mel frames per utterance "
                             f"(modules.py:95), got lengths {list(lens.vals)}")
        return self._run(x, B, T, lens)

    @torch.no_grad()
    def forward(self, x):
        """x: (B, input_size, T) mel -> (B, 1, T*hop) audio (modules.py:130-131)."""
        B, C, T = x.shape
        xf = _transpose_batched(x.float().contiguous(), B, C, T).view(B * T, C)
        return self.frames(xf, B, T).unsqueeze(1)


# ----------------------------------------------------------------------------- audio -> mel
N_FFT, HOP, N_BINS = 1024, 256, 513
PAD = (N_FFT - HOP) // 2  # reflect padding on either side (modules.py:55)
CLAMP = 1e-5  # modules.py:68


def hz_to_mel(f):
    """Slaney's mel scale (librosa's htk=False) in fp64: 200/3 Hz per mel below 1 kHz, then
    ln(6.4)/27 per mel in log frequency."""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


def slaney_mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """The (n_mels, n_fft//2 + 1) fp32 filterbank the reference takes from librosa
    (htk=False, norm="slaney"), as a closed form in fp64: triangles between n_mels + 2 points equally
    spaced on the Slaney mel scale, each scaled by 2 / (f[m+2] - f[m]); cast to fp32 at the end."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    bins = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    ramps = f[:, None] - bins[None, :]
    fd = np.diff(f)
    lower = -ramps[:-2] / fd[:-1, None]
    upper = ramps[2:] / fd[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


def n_frames(L):
    """Frames of an L-sample utterance: (L + 2*384 - 1024) // 256 + 1; L <= 384 is refused (the
    reflection needs pad < length)."""
    L = int(L)
    if L <= PAD:
        raise ValueError(f"Audio2Mel: an utterance of {L} samples is too short: the reflect padding of {PAD} "
                         f"needs at least {PAD + 1}")
    return (L + 2 * PAD - N_FFT) // HOP + 1


def compact_basis(basis):
    """(table int32 [n_mel][3] = start, count, offset; weights fp32) of a (n_mel, 513) basis: each
    filter's span from its first to its last non-zero bin, spans laid end to end."""
    basis = np.asarray(basis, dtype=np.float32)
    table = np.zeros((basis.shape[0], 3), dtype=np.int32)
    chunks, off = [], 0
    for m, row in enumerate(basis):
        nz = np.flatnonzero(row)
        if nz.size:
            st, cnt = int(nz[0]), int(nz[-1] - nz[0] + 1)
            table[m] = (st, cnt, off)
            chunks.append(row[st:st + cnt])
            off += cnt
        else:
            table[m] = (0, 0, off)
    weights = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.float32)
    if weights.size == 0:
        weights = np.zeros(1, dtype=np.float32)
    return table, weights


class Audio2Mel(nn.Module):
    """modules.py:26-69 with the reference's constructor and its two buffers (`mel_basis`, `window`);
    the whole chain -- reflect pad, STFT, magnitude, mel, log10 of the clamp -- is one HIP kernel
    (audio.hip).  The kernel reads the filterbank from the `mel_basis` BUFFER (compacted on the host,
    cached per buffer version), so a loaded state_dict's basis is the one applied.

      forward(audio (B, 1, L))                      -> (B, n_mel, T)      the reference's contract
      frames(audio (B, L) or list, lens, scale)     -> (B, Tmax, n_mel)   frame-major, per-utterance
                                                       lengths, frames past an utterance's end 0.0
    """

    def __init__(self, n_fft=1024, hop_length=256, win_length=1024, sampling_rate=22050, n_mel_channels=80,
                 mel_fmin=0.0, mel_fmax=None):
        super().__init__()
        if (n_fft, hop_length, win_length) != (N_FFT, HOP, N_FFT):
            raise ValueError(f"Audio2Mel: n_fft={n_fft} hop_length={hop_length} win_length={win_length}: the kernel "
                             f"is built for n_fft = win_length = {N_FFT}, hop_length = {HOP} (the reference's values)")
        if not 1 <= n_mel_channels <= 128:
            raise ValueError(f"Audio2Mel: n_mel_channels = {n_mel_channels} outside 1..128")
        window = torch.hann_window(win_length).float()
        mel_basis = torch.from_numpy(slaney_mel_basis(sampling_rate, n_fft, n_mel_channels, mel_fmin, mel_fmax))
        self.register_buffer("mel_basis", mel_basis)
        self.register_buffer("window", window)
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.sampling_rate, self.n_mel_channels = sampling_rate, n_mel_channels
        self._tables = None
        self._table_key = None
        self._lens = None

    n_frames = staticmethod(n_frames)

    def tables(self):
        """(host table, device table, device weights, n_weights, device twiddles) for the current buffers."""
        mb, win = self.mel_basis, self.window
        key = (mb.data_ptr(), mb._version, win.data_ptr(), win._version, str(mb.device))
        if self._tables is None or self._table_key != key:
            if tuple(mb.shape) != (self.n_mel_channels, N_BINS) or tuple(win.shape) != (N_FFT,):
                raise ValueError(f"Audio2Mel: mel_basis {tuple(mb.shape)} / window {tuple(win.shape)}, expected "
                                 f"({self.n_mel_channels}, {N_BINS}) / ({N_FFT},)")
            table, weights = compact_basis(mb.detach().float().cpu().numpy())
            if weights.size > L.MEL_MAX_WEIGHTS:
                raise ValueError(f"Audio2Mel: the compact form of mel_basis has {weights.size} weights; at most "
                                 f"{L.MEL_MAX_WEIGHTS} fit the kernel's LDS budget")
            ang = 2.0 * np.pi * np.arange(N_BINS, dtype=np.float64) / N_FFT
            tw = np.stack((np.cos(ang), -np.sin(ang)), axis=1).astype(np.float32)
            host = (L.c_int * table.size)(*[int(v) for v in table.reshape(-1)])
            dev = mb.device
            self._tables = (host, torch.from_numpy(table.reshape(-1).copy()).to(dev), torch.from_numpy(weights).to(dev),
                            int(weights.size), torch.from_numpy(tw).to(dev))
            self._table_key = key
        return self._tables

    @torch.no_grad()
    def _run(self, audio, lens, scale, layout):
        K._dev(audio, self.mel_basis, self.window, scale)
        if audio.dim() != 2 or audio.dtype != torch.float32:
            raise ValueError(f"Audio2Mel: expected fp32 audio (B, L), got {tuple(audio.shape)} {audio.dtype}")
        audio = audio.contiguous()
        B, stride = audio.shape
        lens = [stride] * B if lens is None else [int(v) for v in lens]
        if len(lens) != B:
            raise ValueError(f"Audio2Mel: lens must hold B={B} values")
        if max(lens) > stride:
            raise ValueError(f"Audio2Mel: lens {max(lens)} exceeds the {stride} samples of a row")
        Tmax = max(n_frames(v) for v in lens)
        if scale is not None:
            scale = scale.to(device=audio.device, dtype=torch.float32).contiguous()
            if scale.shape != (B,):
                raise ValueError(f"Audio2Mel: scale must hold B={B} values")
        host, tab, wts, nw, tw = self.tables()
        n_mel = self.n_mel_channels
        win = self.window if self.window.dtype == torch.float32 else self.window.float()
        lkey = (tuple(lens), str(audio.device))
        if self._lens is None or self._lens[0] != lkey:  # the same lengths again: no second upload
            self._lens = (lkey, (L.c_int * B)(*lens), torch.tensor(lens, dtype=torch.int32, device=audio.device))
        _, lens_host, lens_dev = self._lens
        shape = (B, Tmax, n_mel) if layout == L.MEL_FRAME_MAJOR else (B, n_mel, Tmax)
        out = torch.empty(shape, device=audio.device)
        L.call("avc_audio2mel", audio.data_ptr(), stride, lens_host, lens_dev.data_ptr(), K._ptr(scale), B,
               win.contiguous().data_ptr(), tw.data_ptr(), host, tab.data_ptr(), wts.data_ptr(), nw, n_mel, N_FFT,
               N_FFT, HOP, CLAMP, out.data_ptr(), Tmax, layout, K.stream())
        return out

    def frames(self, audio, lens=None, scale=None):
        """audio: (B, L) fp32 on the device, rows valid up to lens[b] (default L), or a list of 1-D
        tensors of any lengths.  scale: (B,) device factors applied to the samples (the magnitude is
        linear in them).  -> (B, Tmax, n_mel) frame-major log-mel, 0.0 in frames t >= T_b."""
        if isinstance(audio, (list, tuple)):
            if lens is not None:
                raise ValueError("Audio2Mel.frames: a list of utterances carries its own lengths")
            lens = [int(a.numel()) for a in audio]
            buf = torch.zeros(len(audio), max(lens), device=self.mel_basis.device)
            for b, a in enumerate(audio):
                buf[b, :lens[b]] = a.reshape(-1)
            audio = buf
        return self._run(audio, lens, scale, L.MEL_FRAME_MAJOR)

    def forward(self, audio):
        """audio (B, 1, L) -> log-mel (B, n_mel, T) (modules.py:54-69)."""
        if audio.dim() != 3 or audio.shape[1] != 1:
            raise ValueError(f"Audio2Mel.forward: expected audio (B, 1, L), got {tuple(audio.shape)}")
        return self._run(audio.float().squeeze(1), None, None, L.MEL_CHANNEL_MAJOR)


# Mel frames (B * Tmax) one ragged vocoder batch may hold.  Per mel frame a stage of cumulative upsampling u
# and width C holds u*C elements per tensor: 2048 after the first upsampler (8 x 256), then 8192 at each of
# the three widest stages (64 x 128, 128 x 64, 256 x 32).  Inside a residual block of those stages five tensors
# are alive at once -- y, the 3-tap gather h (3 C wide), h1, its LeakyReLU twin h2 and the shortcut / sum -- at
# 6 + 6 + 6 + 2 + 6 = 26 B per element in bf16 mode (fp32 plus bf16 twin for the GEMM outputs, bf16 operands)
# and 4 + 12 + 4 + 4 + 4 = 28 B in fp32 mode: 28 x 8192 = 224 KiB per mel frame.  8192 frames keep the live
# set at 1.75 GiB (64 utterances of 128 frames, or 12 of the longest the bench draws); the GEMMs are past
# filling the chip long before that (B = 16 x 176 frames already is).
VOCODER_MAX_FRAMES = 8192
VOCODER_MAX_BATCH = 32


class MelVocoder:
    """melgan/interface.py:23-53: `inverse(mel (B, 80, T)) -> (B, T*256)` on the HIP generator and
    `__call__(audio (B, L)) -> (B, 80, T)` on the HIP Audio2Mel.  The checkpoint is read with
    torch.load(weights_only=True)."""

    def __init__(self, device="cuda:0", model_name="multi_speaker", generator=None):
        self.device = torch.device(device)
        self.fft = Audio2Mel().to(self.device)
        if generator is None:
            generator = Generator(80, 32, 3)
            sd = torch.load(f"{model_name}.pt", map_location="cpu", weights_only=True)
            generator.load_state_dict(sd)
        self.mel2wav = generator.to(self.device)

    def __call__(self, audio):
        """audio (B, L) -> log-mel (B, 80, T) (interface.py:33-41)."""
        return self.fft(audio.unsqueeze(1).to(self.device))

    def inverse(self, mel):
        return self.mel2wav(mel.to(self.device)).squeeze(1)

    def inverse_frames(self, mel_frames):
        """(B, T, 80) frame-major mel (the Converter's output layout) -> (B, T*256): no transpose."""
        B, T, C = mel_frames.shape
        return self.mel2wav.frames(mel_frames.reshape(B * T, C).float().contiguous(), B, T)

    def inverse_batch_ragged(self, mel_frames, lens):
        """One ragged batch that is already on the device: (B, Tmax, 80) frame-major mel, utterance b valid in
        its first lens[b] frames (the rest is never read) -> (B, Tmax*256), zeros after sample lens[b]*256."""
        B, T, C = mel_frames.shape
        return self.mel2wav.frames_ragged(mel_frames.reshape(B * T, C).float().contiguous(),
                                          K.Lens(lens, T, mel_frames.device))

    def inverse_ragged(self, mels, max_batch=VOCODER_MAX_BATCH, max_frames=VOCODER_MAX_FRAMES):
        """Mels of any lengths -> their waveforms, in input order.  mels: a list of (T_i >= 4, 80) host arrays
        or device tensors; returns a list of 1-D fp32 device tensors of T_i * 256 samples, each the B = 1
        forward of its mel at its own length.  Batches: convert.plan_whole with freq = 1 (sorted by length, cut
        at B <= max_batch and B * Tmax <= max_frames)."""
        from .convert import plan_whole

        mels = list(mels)
        for i, m in enumerate(mels):
            if len(m.shape) != 2 or m.shape[1] != 80:
                raise ValueError(f"inverse_ragged: mels[{i}] must be (T, 80), got {tuple(m.shape)}")
            if m.shape[0] <= 3:  # before any launch: a later batch must not run ahead of the refusal
                raise ValueError(f"inverse_ragged: mels[{i}] has {m.shape[0]} frames; ReflectionPad1d(3) needs at "
                                 "least 4 (modules.py:95)")
        lens = [int(m.shape[0]) for m in mels]
        out = [None] * len(mels)
        for idx, Tmax in plan_whole(lens, 1, max_batch, max_frames):
            if all(isinstance(mels[i], np.ndarray) for i in idx):  # one upload per batch
                host = np.zeros((len(idx), Tmax, 80), dtype=np.float32)
                for r, i in enumerate(idx):
                    host[r, :lens[i]] = mels[i]
                x = torch.from_numpy(host).to(self.device)
            else:
                x = torch.zeros(len(idx), Tmax, 80, device=self.device)
                for r, i in enumerate(idx):
                    x[r, :lens[i]] = torch.as_tensor(mels[i]).to(self.device, torch.float32)
            audio = self.inverse_batch_ragged(x, [lens[i] for i in idx])
            for r, i in enumerate(idx):
                out[i] = audio[r, :lens[i] * self.mel2wav.hop_length]
        return out


def load_model(mel2wav_path, device="cuda:0"):
    """interface.py:12-20 (which ignores its path argument and reads linda_johnson.pt)."""
    g = Generator(80, 32, 3)
    g.load_state_dict(torch.load("linda_johnson.pt", map_location="cpu", weights_only=True))
    return g.to(device)
