"""Voice conversion with a trained plugin model (reference util/evaluate.py:36-94,
Evaluator.crop_mel / get_trans_mel): crop or zero-pad the source (and target) mel to
`len_crop`, run the model with the source and target speaker embeddings -- dispatched like
get_trans_mel over the three model families (plain: model(x, e_org, e_trg); isAdjust:
model(x, e_org, e_trg, True, mel_target), 4 outputs; isAdain: features of the source first,
model(x, e_org, None, None), then model(x, e_org, e_trg, feature)) -- and cut the converted mel
back to the source's real length when it was padded (the `isPlay` branch).

Same kernels as training, forward only under `torch.no_grad()`; the model stays in whatever
BatchNorm mode the caller left it in (the reference converts with the model in train mode, so
BN uses the statistics of the one utterance).  `get_wavs` (evaluate.py:96-98) turns a converted
mel into a waveform with the HIP MelGAN generator (autoformer_amd.melgan.MelVocoder) when the
Converter was given one.

Everything above works on one window of `len_crop` frames (the reference's evaluation protocol: a longer
utterance is converted as a random crop).  convert_whole converts recordings of any length whole, many of
different lengths to a batch, and

    python -m autoformer_amd.convert --ckpt F --src a.wav [b.wav ...] --ref t1.wav [t2.wav ...]
        --embedder_ckpt F --vocoder_ckpt F --out_dir O

goes from wavs to wavs with it (AutoVC).
"""
from __future__ import annotations

import numpy as np
import torch


def crop_mel(mel: np.ndarray, len_crop: int, rng=np.random):
    """evaluate.py:36-50: (T, 80) -> ((len_crop, 80), pad_size): zero padding at the end when
    T < len_crop, a uniform crop offset in [0, T - len_crop) when longer (one rng draw)."""
    T = mel.shape[0]
    if T < len_crop:
        out = np.zeros((len_crop,) + mel.shape[1:], dtype=mel.dtype)
        out[:T] = mel
        return out, len_crop - T
    if T == len_crop:
        return mel, 0
    left = rng.randint(0, T - len_crop)
    return mel[left:left + len_crop], 0


class Converter:
    """convert(mel_source, emb_org, emb_trg) -> converted mel (T', 80) on the host."""

    def __init__(self, model, len_crop: int, device="cuda:0", vocoder=None, embedder=None):
        self.model = model
        self.len_crop = len_crop
        self.device = torch.device(device)
        self.vocoder = vocoder  # autoformer_amd.melgan.MelVocoder (evaluate.py:24) or None
        self.embedder = embedder  # an LstmDV (evaluate.py:25), a MetaDV or None: convert_between

    @torch.no_grad()
    def get_wavs(self, mel, frames: bool = False):
        """evaluate.py:96-98: (1, 80, T) mel -> (1, T*256) waveform (the reference contract).
        frames=True: a frame-major (1, T, 80) mel, the layout get_trans_mel returns, goes straight
        in without the transpose.  The layout is stated, never guessed from the shape (T may be 80)."""
        if self.vocoder is None:
            raise RuntimeError("Converter was built without a vocoder (pass vocoder=MelVocoder(...))")
        if mel.dim() != 3 or mel.shape[2 if frames else 1] != 80:
            raise ValueError(f"get_wavs: expected a {'(1, T, 80)' if frames else '(1, 80, T)'} mel, got "
                             f"{tuple(mel.shape)}")
        return self.vocoder.inverse_frames(mel) if frames else self.vocoder.inverse(mel)

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).unsqueeze(0).to(self.device)

    @torch.no_grad()
    def get_trans_mel(self, mel_source: np.ndarray, mel_target, emb_org: np.ndarray, emb_trg: np.ndarray,
                      isAdjust: bool = False, isAdain: bool = False, isPlay: bool = False):
        """util/evaluate.py:56-94 on host mels: returns (mel_source, mel_target, mel_trans) device
        tensors (1, T, 80) exactly as the reference does; the source is cropped before the target
        (the reference's rng order).  mel_target may be None unless isAdjust."""
        src, pad_s = crop_mel(mel_source, self.len_crop)
        x = self._dev(src)
        y, pad_t = (None, 0)
        if mel_target is not None:
            tgt, pad_t = crop_mel(mel_target, self.len_crop)
            y = self._dev(tgt)
        eo, et = self._dev(emb_org), self._dev(emb_trg)
        if isAdjust:
            if y is None:
                raise ValueError("isAdjust conversion needs the target mel (evaluate.py:79)")
            _, _, mel_trans, _ = self.model(x, eo, et, True, y)
        elif isAdain:
            _, feature = self.model(x, eo, None, None)
            _, mel_trans, _ = self.model(x, eo, et, feature)
        else:
            _, mel_trans, _ = self.model(x, eo, et)
        mel_trans = mel_trans.squeeze(1)
        if isPlay:
            if pad_s > 0:
                x = x[:, : self.len_crop - pad_s, :]
                mel_trans = mel_trans[:, : self.len_crop - pad_s, :]
            if y is not None and pad_t > 0:
                y = y[:, : self.len_crop - pad_t, :]
        return x, y, mel_trans

    @torch.no_grad()
    def convert(self, mel_source: np.ndarray, emb_org: np.ndarray, emb_trg: np.ndarray, trim: bool = True,
                mel_target=None, isAdjust: bool = False, isAdain: bool = False):
        """The converted mel (T', 80) on the host (trimmed to the source length when padded)."""
        _, _, mel_trans = self.get_trans_mel(mel_source, mel_target, emb_org, emb_trg, isAdjust, isAdain,
                                             isPlay=trim)
        return mel_trans[0].float().cpu().numpy()

    @torch.no_grad()
    def convert_between(self, mel_source: np.ndarray, src_mels, trg_mels, trim: bool = True, **kw):
        """Conversion between two speakers given only recordings of them: the d-vectors of src_mels and
        trg_mels (lists of (T, 80) mels; autoformer_amd.embed.speaker_dvector, evaluate.py:100-106) are
        emb_org / emb_trg of convert()."""
        if self.embedder is None:
            raise RuntimeError("Converter was built without an embedder (pass embedder=LstmDV(...))")
        from .embed import speaker_dvector

        e_org = speaker_dvector(self.embedder, src_mels, self.len_crop)
        e_trg = speaker_dvector(self.embedder, trg_mels, self.len_crop)
        return self.convert(mel_source, e_org, e_trg, trim=trim, **kw)

    @torch.no_grad()
    def convert_whole(self, mel_source: np.ndarray, emb_org: np.ndarray, emb_trg: np.ndarray):
        """The whole utterance converted, (T, 80) on the host, T = mel_source.shape[0]: no crop, no
        len_crop (convert_whole below, a batch of one)."""
        return convert_whole(self.model, [mel_source], emb_org, emb_trg, device=self.device)[0]


# ----------------------------------------------------------------------------- whole utterances
# Frames (B * Tmax) one ragged batch may hold.  The largest tensors of the forward are the decoder
# recurrences': the training-path LSTM entry points keep, per frame and layer, the (4H) fp32 gates next
# to the (H) fp32 h and c.  lstm2 is two layers of H = 1024: 2 x (16 KB gates + 4 KB h + 4 KB c) plus
# layer 0's 16 KB input projection and the two 2 KB bf16 h twins = 68 KB per frame, all alive at once
# in its one-launch pair forward; lstm1 (H = 512, 20 KB) and the conv activations (<= 2 KB fp32 per
# frame and layer, freed as the next layer runs) stay below that.  16384 frames x 68 KB = 1.1 GB at the
# peak -- 64 utterances of 256 frames (3 s), or 25 of the longest the bench draws (640).
MAX_FRAMES = 16384


def padded_len(T, freq):
    """P = ceil(T / freq) * freq: the frames an utterance of T occupies (crop_mel's padding rule)."""
    T, freq = int(T), int(freq)
    if T < 1 or freq < 1:
        raise ValueError(f"an utterance has T >= 1 frames and freq >= 1, got T = {T}, freq = {freq}")
    return -(-T // freq) * freq


def plan_whole(lens, freq, max_batch=64, max_frames=MAX_FRAMES):
    """Batches for convert_whole, host only and deterministic: [(indices, Tmax)] over the utterances sorted
    by padded length (ties by index), cut so that every batch has B <= max_batch rows and B * Tmax <=
    max_frames frames (Tmax: its longest padded length).  An utterance longer than max_frames on its own
    forms a batch of one."""
    if int(max_batch) < 1 or int(max_frames) < 1:
        raise ValueError(f"max_batch and max_frames must be >= 1, got {max_batch}, {max_frames}")
    P = [padded_len(T, freq) for T in lens]
    order = sorted(range(len(P)), key=lambda i: (P[i], i))
    plan, cur = [], []
    for i in order:
        if cur and (len(cur) + 1 > int(max_batch) or (len(cur) + 1) * P[i] > int(max_frames)):
            plan.append((cur, P[cur[-1]]))
            cur = []
        cur.append(i)
    if cur:
        plan.append((cur, P[cur[-1]]))
    return plan


def whole_family(model):
    """Raises NotImplementedError unless convert_whole takes this model: `type(model) is AutoVC`."""
    from .factory.AutoVC import AutoVC

    if type(model) is AutoVC:
        return
    name = type(model).__name__
    if name.endswith("_Adjust"):
        why = "an *_Adjust variant: its Adjust pass over the target mel is left out of whole-utterance conversion"
    elif name.endswith("2"):
        why = "an AdaIN variant: its per-utterance feature statistics are left out of whole-utterance conversion"
    elif name.startswith("Meta"):
        why = "a Meta model: its token mixers fix the length at 176 frames"
    else:
        why = "not an AutoVC"
    raise NotImplementedError(f"convert_whole converts AutoVC alone; {name} is {why}")


def _emb_rows(e, n, what):
    e = np.asarray(e, dtype=np.float32)
    if e.ndim == 1:
        e = np.broadcast_to(e, (n, e.shape[0]))
    if e.ndim != 2 or e.shape[0] != n:
        raise ValueError(f"{what} must be (E,) or (N = {n}, E), got {e.shape}")
    return np.ascontiguousarray(e)


@torch.no_grad()
def convert_whole(model, mels, emb_org, emb_trg, max_batch=64, max_frames=MAX_FRAMES, device=None, vocoder=None):
    """Whole-utterance conversion of N utterances of any lengths: [(T_i, 80) float32 host mels] in input
    order.  mels: N host mels (T_i, 80); emb_org / emb_trg: (N, E), or (E,) for all of them.

    vocoder (a melgan.MelVocoder): every batch's mel_postnet goes on to the generator where it lies, on the
    device, as one ragged batch with the TRUE lengths T_i (MelVocoder.inverse_batch_ragged: the pad frames
    up to P_i are not vocoded); the result is then (mels, wavs), wavs[i] a float32 host array of T_i * 256
    samples.  Every T_i must be >= 4 then (the generator's ReflectionPad1d(3)); a batch of more than
    melgan.VOCODER_MAX_FRAMES frames is vocoded in slices of it.

    Utterance i is zero-padded at the end to P_i = ceil(T_i / freq) * freq frames (crop_mel's rule); its
    result is mel_postnet of the model's B = 1 forward at T = P_i, cut back to T_i rows.  The pad frames
    up to P_i are part of that forward (they count in the BatchNorm statistics), nothing beyond P_i is.
    Utterances of different lengths share a batch (plan_whole) under layers.per_utterance_bn(lens=...):
    a train-mode model takes BatchNorm statistics over each utterance's own P_i frames and its buffers
    stay as they were; an eval-mode model uses its running statistics.  AutoVC only (whole_family)."""
    whole_family(model)
    from . import kernels as K
    from . import layers as Lyr

    mels = [np.asarray(m, dtype=np.float32) for m in mels]
    for i, m in enumerate(mels):
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] != 80:
            raise ValueError(f"mels[{i}] must be a (T >= 1, 80) array, got {m.shape}")
    n = len(mels)
    eo, et = _emb_rows(emb_org, n, "emb_org"), _emb_rows(emb_trg, n, "emb_trg")
    freq = int(model.encoder.freq)
    if freq < 2:
        raise ValueError(f"convert_whole needs freq >= 2 (per-utterance statistics need two frames), got {freq}")
    plan = plan_whole([m.shape[0] for m in mels], freq, max_batch, max_frames)
    if vocoder is not None:
        from .melgan import VOCODER_MAX_FRAMES

        short = [i for i, m in enumerate(mels) if m.shape[0] <= 3]
        if short:  # before any launch
            raise ValueError(f"convert_whole(vocoder=...): mels{short} have fewer than 4 frames; the generator's "
                             "ReflectionPad1d(3) needs at least 4")
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    out, wavs = [None] * n, [None] * n
    for idx, Tmax in plan:
        x = np.zeros((len(idx), Tmax, 80), dtype=np.float32)
        for r, i in enumerate(idx):
            x[r, :mels[i].shape[0]] = mels[i]
        lens = K.Lens([padded_len(mels[i].shape[0], freq) for i in idx], Tmax, device)
        xd = torch.from_numpy(x).to(device)
        with Lyr.per_utterance_bn(lens=lens):
            _, psnt, _ = model(xd, torch.from_numpy(eo[idx]).to(device), torch.from_numpy(et[idx]).to(device))
        psnt = psnt.squeeze(1).float()
        if vocoder is not None:
            # rows are sorted by padded length: slices of them, each cut to its own longest TRUE length
            true = [mels[i].shape[0] for i in idx]
            r0 = 0
            while r0 < len(idx):
                r1, Tm = r0 + 1, true[r0]
                while r1 < len(idx) and (r1 + 1 - r0) * max(Tm, true[r1]) <= VOCODER_MAX_FRAMES:
                    Tm = max(Tm, true[r1])
                    r1 += 1
                wav = vocoder.inverse_batch_ragged(psnt[r0:r1, :Tm], true[r0:r1]).float().cpu().numpy()
                for r in range(r0, r1):
                    wavs[idx[r]] = np.ascontiguousarray(wav[r - r0, :true[r] * 256])
                r0 = r1
        psnt = psnt.cpu().numpy()
        for r, i in enumerate(idx):
            out[i] = np.ascontiguousarray(psnt[r, :mels[i].shape[0]])
    if device.type == "cuda":
        K.check_faults(device)
    return out if vocoder is None else (out, wavs)


# ----------------------------------------------------------------------------- CLI
def _parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m autoformer_amd.convert",
                                description="wav to wav: convert whole recordings to the voice of a target speaker "
                                            "given a few reference recordings of that speaker (AutoVC, any lengths, "
                                            "batched)")
    p.add_argument("--model", default="AutoVC", help="a factory plugin name (whole-utterance conversion takes AutoVC)")
    p.add_argument("--ckpt", help="the model's state_dict (torch.save); required unless --det_init")
    p.add_argument("--dim_neck", type=int, default=44)
    p.add_argument("--dim_emb", type=int, default=256)
    p.add_argument("--dim_pre", type=int, default=512)
    p.add_argument("--freq", type=int, default=22)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--src", nargs="+", metavar="WAV", help="recordings to convert")
    src.add_argument("--src_dir", metavar="DIR", help="convert every *.wav of this folder (sorted)")
    p.add_argument("--src_ref", nargs="+", metavar="WAV",
                   help="recordings of the source speaker (default: the source recordings themselves)")
    p.add_argument("--ref", nargs="+", metavar="WAV", required=True, help="recordings of the target speaker")
    p.add_argument("--embedder", choices=["LstmDV", "MetaDV"], default="LstmDV", help="the speaker embedder")
    p.add_argument("--embedder_ckpt", help="the embedder's state_dict; required unless --det_init")
    p.add_argument("--num_classes", type=int, default=256, help="MetaDV: classes of its checkpoint's head")
    p.add_argument("--vocoder_ckpt", help="MelGAN generator state_dict; required unless --det_init")
    p.add_argument("--out_dir", required=True, help="<out_dir>/<name>.wav per source recording (22050 Hz, 16-bit)")
    p.add_argument("--resample", action="store_true",
                   help="convert wavs at another rate to 22050 Hz on the device instead of refusing them")
    p.add_argument("--max_batch", type=int, default=64, help="utterances per batch")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--det_init", action="store_true", help="closed-form weights instead of checkpoints (smoke runs)")
    p.add_argument("--save_mel", action="store_true", help="also write the converted mel as <name>.npy")
    return p


def _wav_mels(paths, a2m, device, resample):
    """Peak-normalised log-mels of wav files, in input order (make_spec's chain)."""
    from .make_spec import check_rate, first_channel, mels_of, read_wav, resample_waves
    from .resample import TARGET_FS

    out = [None] * len(paths)
    by_rate = {}
    for i, path in enumerate(paths):
        x, fs = read_wav(path)
        if not resample:
            check_rate(fs, path)
        by_rate.setdefault(int(fs), []).append((i, np.ascontiguousarray(first_channel(x), dtype=np.float32)))
    for fs, group in sorted(by_rate.items()):
        waves = [w for _, w in group]
        if fs == TARGET_FS:
            mels = mels_of(a2m, waves)
        else:
            mels = mels_of(a2m, *resample_waves(fs, waves, device))
        for (i, _), m in zip(group, mels):
            out[i] = m
    return out


def main(argv=None):
    import os

    args = _parser().parse_args(argv)
    if not str(args.device).startswith("cuda"):
        raise SystemExit(f"--device {args.device}: the HIP kernels need a GPU")
    for flag, what in (("ckpt", "the model's state_dict"), ("embedder_ckpt", f"an {args.embedder} state_dict"),
                       ("vocoder_ckpt", "a MelGAN generator state_dict")):
        if not getattr(args, flag) and not args.det_init:
            raise SystemExit(f"--{flag} FILE ({what}) is required unless --det_init is given")
    if args.src_dir:
        srcs = [os.path.join(args.src_dir, f) for f in sorted(os.listdir(args.src_dir)) if f.lower().endswith(".wav")]
        if not srcs:
            raise SystemExit(f"--src_dir {args.src_dir}: no *.wav files")
    else:
        srcs = list(args.src)
    names = [os.path.splitext(os.path.basename(p))[0] for p in srcs]
    if len(set(names)) != len(names):
        raise SystemExit("two source recordings share a file name: their outputs would overwrite each other")
    import autoformer_amd as A

    from .embed import speaker_dvector
    from .evaluate import _load_module, write_wav
    from .melgan import Audio2Mel, Generator, MelVocoder

    A.set_compute(args.dtype)
    # the reference converts in train mode: BatchNorm on the utterance's own statistics
    model = _load_module(args.model, (args.dim_neck, args.dim_emb, args.dim_pre, args.freq), args.ckpt, args.det_init,
                         args.device).train()
    whole_family(model)
    ctor = (args.num_classes,) if args.embedder == "MetaDV" else ()
    embedder = _load_module(args.embedder, ctor, args.embedder_ckpt, args.det_init, args.device).eval()
    g = Generator(80, 32, 3)
    if args.vocoder_ckpt:
        g.load_state_dict(torch.load(args.vocoder_ckpt, map_location="cpu", weights_only=True))
    else:
        from .detinit import det_melgan_state

        g.load_state_dict({k: torch.from_numpy(v) for k, v in
                           det_melgan_state([(k, tuple(v.shape)) for k, v in g.state_dict().items()]).items()})
    vocoder = MelVocoder(device=args.device, generator=g)
    a2m = Audio2Mel().to(args.device)
    src_mels = _wav_mels(srcs, a2m, args.device, args.resample)
    ref_mels = _wav_mels(list(args.ref), a2m, args.device, args.resample)
    org_mels = _wav_mels(list(args.src_ref), a2m, args.device, args.resample) if args.src_ref else src_mels
    e_trg = speaker_dvector(embedder, ref_mels)
    e_org = speaker_dvector(embedder, org_mels)
    # conversion and vocoder batch by batch on the device: each batch's mels go on to the generator as a ragged batch
    trans, wavs = convert_whole(model, src_mels, e_org, e_trg, args.max_batch, device=args.device, vocoder=vocoder)
    os.makedirs(args.out_dir, exist_ok=True)
    for name, mel, wav in zip(names, trans, wavs):
        write_wav(os.path.join(args.out_dir, name + ".wav"), wav)
        if args.save_mel:
            np.save(os.path.join(args.out_dir, name + ".npy"), mel)
    print(f"{args.out_dir}: {len(trans)} wavs, {sum(m.shape[0] for m in trans)} frames")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
