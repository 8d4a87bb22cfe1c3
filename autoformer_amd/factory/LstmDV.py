"""LstmDV (reference factory/LstmDV.py:4-24): the d-vector speaker embedder --
LSTM(80, 768, 3 layers) -> last step -> Linear(768 -> 256) -> L2 normalise.  It produces the 256-d
speaker embeddings the models train and convert with (emb_org / emb_trg, the second entry of every
train.pkl speaker; make_data/make_metadata.ipynb cell 5) and the d-vectors behind the reference's
cosine-similarity metric (util/evaluate.py:100-121).

Two HIP paths:
  * autograd enabled -- the training composition of Adjust.py: three LSTM layers (input projection
    GEMM + persistent recurrence, everything kept for the backward), step select, linear, row
    normalisation.  Gradients reach every parameter and x (the GAN trainers' classifier loss).
  * torch.no_grad() in bf16 compute, where avc_lstm_infer_persistent admits the batch -- per layer
    the input projection GEMM and the forward-only recurrence (lstm_infer.hip): layers 0 and 1
    write only the bf16 h the next GEMM reads, the top layer only the fp32 h of each utterance's
    own last frame (`lens`), then the fused d-vector head (avc_dvec_head).
Any other no_grad call (fp32 parity mode, another dim_cell, a batch whose grid is not resident) runs
the training composition and gathers the per-length rows by indexing.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from .. import layers as Lyr
from .. import variants as V
from .AutoVC import _frames
from .Norm import LSTMParams


class LstmDV(nn.Module):
    def __init__(self, num_layers=3, dim_input=80, dim_cell=768, dim_emb=256):
        super().__init__()
        self.lstm = LSTMParams(dim_input, hidden_size=dim_cell, num_layers=num_layers, batch_first=True)
        self.embedding = nn.Linear(dim_cell, dim_emb)
        self._lstm = [Lyr.LSTMLayerCore(self.lstm, layer) for layer in range(num_layers)]
        self._lin = Lyr.PackCache()
        self.infer_rows = 0  # utterances per workgroup group of the inference recurrence (0: default)

    def max_infer_batch(self, limit=512):
        """The largest batch (<= limit) the forward-only recurrence admits in one launch, 0 if none
        (fp32 mode, another dim_cell, no device): what embed_utterances sizes its batches by."""
        H = self.lstm.hidden_size
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

    def _lens(self, lens, B, T):
        if lens is None:
            return None
        lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"LstmDV: lens must hold B={B} lengths in 1..T={T}, got {lens}")
        return lens

    def _train_form(self, mel, B, T, lens):
        h = Lyr.lstm(self.lstm, self._lstm, mel, B, T)
        if lens is None:
            last = V.step_select(h, B, T, T - 1)
        else:
            idx = torch.tensor([b * T + n - 1 for b, n in enumerate(lens)], device=h.device)
            last = h.index_select(0, idx)
        return V.rownorm(Lyr.linear(last, self.embedding.weight, self.embedding.bias, self._lin))

    def _infer_form(self, mel, B, T, lens):
        H = self.lstm.hidden_size
        x, last = K.twin(mel), None  # bf16 operand copy of the mel, as the training form makes it
        hbuf = K.lstm_infer_scratch(B, H, mel.device, self.infer_rows)  # the launches are stream-ordered
        for n, core in enumerate(self._lstm):
            top = n == len(self._lstm) - 1
            wih, bsum, whh, _, _ = core.packs()
            In = x.shape[1]
            xproj = torch.empty(B * T, 4 * H, device=mel.device)
            K.gemm(B * T, 4 * H, In, K.operand(x, In), K.operand(wih, In), xproj, bias=bsum)
            x, last = K.lstm_infer(xproj, whh, B, T, H, lens=lens if top else None, rows=self.infer_rows,
                                   want_h16=not top, want_last=top, hbuf=hbuf)
        return K.dvec_head(last, self.embedding.weight, self.embedding.bias)

    def forward(self, x, lens=None):
        """(B, T, 80) -> (B, 256) unit-norm d-vectors.  lens (no_grad only): per-utterance frame
        counts in 1..T of a batch padded at the end; row b is then the embedding of x[b, :lens[b]]."""
        K.require_device(x)
        mel, B, T = _frames(x)
        if torch.is_grad_enabled():
            if lens is not None:
                raise ValueError("LstmDV: lens is an inference argument (call under torch.no_grad())")
            return self._train_form(mel, B, T, None)
        lens = self._lens(lens, B, T)
        if K.compute() == K.BF16 and K.lstm_infer_persistent(B, self.lstm.hidden_size, self.infer_rows):
            return self._infer_form(mel, B, T, lens)
        return self._train_form(mel, B, T, lens)
