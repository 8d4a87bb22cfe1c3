"""MetaDV (reference factory/MetaDV.py:8-70): the MLP-Mixer speaker classifier the GAN / StarGAN
trainers use as their classifier C -- LSTM(80 -> 768) -> e1 = the last frame; four random 128-frame
windows of the LSTM output, each read as a Conv1d input with THE WINDOW FRAMES AS CHANNELS and the
768 hidden units as the length axis -> ConvNorm(128 -> 768, k3) -> MLPMixer(image 768, patch 32,
dim 768, out conv 576 -> 88 k3) -> output channel 87 only; e2 = their mean; embedding =
Linear(1536 -> 256)(cat(e1, e2)); returns (Linear(256 -> num_classes)(embedding),
embedding / ||embedding||).  No BN and no dropout: train and eval are the same function.

The four crops of all B utterances go through the conv and the mixer as one batch of S*B rows
(`crop_chunk` crops at a time if memory asks for it; rows are independent, so the result does not
depend on it).  Two HIP paths:
  * autograd enabled -- the training composition: LSTM layer, crop_windows (the conv operand of all
    crops in one launch, and e1), conv, mlp_mixer, chan_mean, the two linears, row normalisation.
    Gradients reach every parameter and x.
  * torch.no_grad() in bf16 compute, where avc_lstm_infer_persistent admits the batch -- the
    forward-only recurrence (bf16 h of every frame + the fp32 h of each utterance's own last
    frame), crop_windows from the bf16 h, conv, mixer, and the fused head (avc_metadv_head).
Any other no_grad call (fp32 parity mode, another emb, a batch whose grid is not resident,
`infer_path = False`) runs the training composition.

The windows: without `lefts` the module draws random.randint(0, T - crop_len) sample_count times,
in the reference's order, from Python's `random` module, so random.seed(k) reproduces the
reference's crops.  With `lens` (no_grad only) row b is embedded as x[b, :lens[b]], as the reference
would embed it alone: e1 from frame lens[b] - 1, crops drawn inside [0, lens[b] - crop_len], row by
row.  `lefts` (sample_count starts, or sample_count rows of B) fixes the windows.
"""
import random

import torch
import torch.nn as nn

from .. import kernels as K
from .. import layers as Lyr
from .. import metadv as MD
from .. import metaformer as MF
from .. import variants as V
from .AutoVC import _frames
from .MLPMixer import MLPMixer
from .Norm import ConvNorm, LSTMParams

MAX_INFER_BATCH = 64  # S * 64 = 256 crops per pass through the mixer (about 6 GB of activations)


class MetaBlock(nn.Module):
    def __init__(self, num_classes, dim_emb=256, emb=768, crop_len=128, patch_size=32, mlp_depth=1, kernel_size=3,
                 channels=1, sample_count=4):
        super().__init__()
        self.token_mixer = LSTMParams(80, hidden_size=emb, num_layers=1, batch_first=True)
        self.conv_1 = ConvNorm(crop_len, emb, kernel_size=kernel_size)
        self.mlp = MLPMixer(image_size=emb, channels=channels, patch_size=patch_size, kernel_size=kernel_size,
                            dim=emb, out_dim=88, padding=1, depth=mlp_depth)
        self.dv = nn.Linear(emb * 2, dim_emb)
        self.output = nn.Linear(dim_emb, num_classes)
        self.crop_len = crop_len
        self.sample_count = sample_count
        self.emb = emb
        self._lstm = [Lyr.LSTMLayerCore(self.token_mixer, 0)]
        self._c1, self._dv, self._out = Lyr.PackCache(), Lyr.PackCache(), Lyr.PackCache()
        self.infer_rows = 0     # utterances per workgroup group of the inference recurrence (0: default)
        self.infer_path = True  # no_grad + bf16: the forward-only path (False: the training composition)
        self.crop_chunk = 0     # crops per pass through conv + mixer (0: all sample_count at once)

    # ------------------------------------------------------------------ windows
    def draw_lefts(self, T, lens=None):
        """The window starts of one call, from Python's `random`: sample_count draws of
        randint(0, T - crop_len) (MetaDV.py:46-47) -- with lens, sample_count draws per row inside
        the row's own length, row by row (each row as the reference embeds it alone), returned as
        sample_count rows of B."""
        W, S = self.crop_len, self.sample_count
        if lens is None:
            if T < W:
                raise ValueError(f"MetaDV: T = {T} frames is shorter than crop_len = {W}")
            return [random.randint(0, T - W) for _ in range(S)]
        if min(lens) < W:
            raise ValueError(f"MetaDV: an utterance of {min(lens)} frames is shorter than crop_len = {W}")
        rows = [[random.randint(0, n - W) for _ in range(S)] for n in lens]
        return [[rows[b][s] for b in range(len(lens))] for s in range(S)]

    def _lens(self, lens, B, T):
        if lens is None:
            return None
        lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"MetaDV: lens must hold B={B} lengths in 1..T={T}, got {lens}")
        return lens

    def _lefts(self, lefts, B, T, lens):
        """sample_count rows of B checked starts (a flat list of sample_count starts serves every row)."""
        W, S = self.crop_len, self.sample_count
        lefts = lefts.tolist() if hasattr(lefts, "tolist") else list(lefts)
        if len(lefts) != S:
            raise ValueError(f"MetaDV: lefts must hold sample_count = {S} entries, got {len(lefts)}")
        rows = [[int(v)] * B if not hasattr(v, "__len__") else [int(u) for u in v] for v in lefts]
        for row in rows:
            if len(row) != B:
                raise ValueError(f"MetaDV: a row of lefts must hold B = {B} starts")
            for b, v in enumerate(row):
                n = T if lens is None else lens[b]
                if n < W:
                    raise ValueError(f"MetaDV: {n} frames are shorter than crop_len = {W}")
                if v < 0 or v > n - W:
                    raise ValueError(f"MetaDV: window start {v} of row {b} outside 0..{n - W}")
        return rows

    # ------------------------------------------------------------------ the two paths
    def _mix(self, X, B):
        """Conv operand X (S*B*E, W) -> mixer output (S*B*E, 88), crop_chunk whole crops at a time."""
        S, E = self.sample_count, self.emb
        n = self.crop_chunk if 0 < self.crop_chunk < S else S
        ys = []
        for s0 in range(0, S, n):
            s1 = min(S, s0 + n)
            xs = X if n == S else X[s0 * B * E:s1 * B * E]
            a = MF.conv(xs, self.conv_1.conv, self._c1, (s1 - s0) * B, E)
            ys.append(MF.mlp_mixer(a, self.mlp, (s1 - s0) * B, E))
        return ys[0] if len(ys) == 1 else torch.cat(ys)

    def _train_form(self, mel, B, T, lf, lens):
        S = self.sample_count
        h = Lyr.lstm(self.token_mixer, self._lstm, mel, B, T)
        X, e1 = MD.crop_windows(h, lf, B, T, self.crop_len, lens)
        e2 = MD.chan_mean(self._mix(X, B), S, B)
        emb = Lyr.linear(torch.cat((e1, e2), dim=1), self.dv.weight, self.dv.bias, self._dv)
        d_vec = V.rownorm(emb)
        return Lyr.linear(emb, self.output.weight, self.output.bias, self._out), d_vec

    def _infer_form(self, mel, B, T, lf, lens):
        H = self.emb
        wih, bsum, whh, _, _ = self._lstm[0].packs()
        x = K.twin(mel)  # bf16 operand copy of the mel, as the training form makes it
        In = x.shape[1]
        xproj = torch.empty(B * T, 4 * H, device=mel.device)
        K.gemm(B * T, 4 * H, In, K.operand(x, In), K.operand(wih, In), xproj, bias=bsum)
        h16, last = K.lstm_infer(xproj, whh, B, T, H, lens=lens, rows=self.infer_rows, want_h16=True, want_last=True)
        X = K.crop_windows(h16, lf, B, T, self.crop_len, lens=lens)
        Y = self._mix(X, B)
        return K.metadv_head(last, Y, self.sample_count, self.dv.weight, self.dv.bias, self.output.weight,
                             self.output.bias)

    def max_infer_batch(self, limit=MAX_INFER_BATCH):
        """The largest batch (<= limit) the forward-only path admits in one call, 0 if none (fp32
        mode, another emb, no device): what embed_utterances sizes its batches by."""
        H = self.emb
        if K.compute() != K.BF16 or not K.lstm_infer_persistent(1, H, self.infer_rows):
            return 0
        lo, hi = 1, limit  # admitted batches form a prefix 1..n: bisect for n
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if K.lstm_infer_persistent(mid, H, self.infer_rows):
                lo = mid
            else:
                hi = mid - 1
        return lo

    def forward(self, x, lens=None, lefts=None):
        """(B, T, 80) -> (predictions (B, num_classes), d_vec (B, dim_emb)).  lens (no_grad only):
        per-utterance frame counts of a batch padded at the end.  lefts: the window starts
        (sample_count values, or sample_count rows of B); None draws them (draw_lefts)."""
        B, T = (x.shape[0], x.shape[-2]) if x.dim() in (3, 4) else (0, 0)
        grad = torch.is_grad_enabled()
        if grad and lens is not None:
            raise ValueError("MetaDV: lens is an inference argument (call under torch.no_grad())")
        lens = self._lens(lens, B, T)
        # the windows are settled (and a too-short input refused) on the host, before any launch
        rows = self._lefts(self.draw_lefts(T, lens) if lefts is None else lefts, B, T, lens)
        K.require_device(x)
        mel, B, T = _frames(x)
        lf = K.Lefts(rows, self.sample_count, B, mel.device, last=None if lens is None else [n - 1 for n in lens])
        if (not grad and self.infer_path and K.compute() == K.BF16
                and K.lstm_infer_persistent(B, self.emb, self.infer_rows)):
            return self._infer_form(mel, B, T, lf, lens)
        return self._train_form(mel, B, T, lf, lens)


class MetaDV(nn.Module):
    """For Gan Training Use (MetaDV.py:60-70)."""

    def __init__(self, num_classes=256):
        super().__init__()
        self.metablock = MetaBlock(num_classes)

    @property
    def crop_len(self):
        return self.metablock.crop_len

    def draw_lefts(self, T, lens=None):
        return self.metablock.draw_lefts(T, lens)

    def max_infer_batch(self, limit=MAX_INFER_BATCH):
        return self.metablock.max_infer_batch(limit)

    def forward(self, x, lens=None, lefts=None):
        return self.metablock(x, lens, lefts)
