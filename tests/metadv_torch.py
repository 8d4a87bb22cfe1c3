"""The MetaDV speaker classifier in plain torch, as functions of a state_dict (name -> tensor):
what the fixture tests/golden/metadv.npz is checked against on the CPU, and the emulation of the
bf16 compute mode's rounding points that the GPU bar is built from.

  LSTM(80 -> E) -> e1 = h at the last frame; S windows h[b, left:left+W, :] taken as Conv1d inputs
  with the W frames as channels and the E hidden units as the length axis -> Conv1d(W -> E, k3, pad 1)
  -> MLP-Mixer on the (E x E) map (patches ps x ps, dim E, token + channel feed-forward, output
  Conv1d(patches -> 88, k3, pad 1)) -> output channel 87 -> mean over the windows = e2;
  emb = Linear(cat(e1, e2)); returns (Linear(emb), emb / ||emb||).

`r` is applied wherever the bf16 path rounds: the bf16 weights, the mel, h_{t-1} before the recurrent
product, the h the crops read, the conv / mixer GEMM operands (patches, LayerNorm outputs, GELU
outputs, the output conv's input).  e1, every accumulation, the biases and the head stay fp32."""
import torch
import torch.nn.functional as F

PRE = "metablock."


def _ident(t):
    return t


def bf16_round(t):
    return t.bfloat16().to(t.dtype)


def lefts_rows(lefts, B):
    """S starts (one per crop, every row) or S rows of B -> S rows of B ints."""
    rows = []
    for v in (lefts.tolist() if hasattr(lefts, "tolist") else lefts):
        rows.append([int(v)] * B if not isinstance(v, (list, tuple)) else [int(u) for u in v])
    return rows


def lstm(sd, x, r=_ident):
    if r is _ident:  # the unrounded function: torch's own LSTM (the explicit loop below is the same recurrence)
        H = sd[PRE + "token_mixer.weight_hh_l0"].shape[1]
        mod = torch.nn.LSTM(x.shape[-1], H, 1, batch_first=True).to(x.dtype)
        names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
        return torch.func.functional_call(mod, {n: sd[PRE + "token_mixer." + n] for n in names}, (x,))[0]
    wih, whh = r(sd[PRE + "token_mixer.weight_ih_l0"]), r(sd[PRE + "token_mixer.weight_hh_l0"])
    bias = sd[PRE + "token_mixer.bias_ih_l0"] + sd[PRE + "token_mixer.bias_hh_l0"]
    B, T, _ = x.shape
    H = whh.shape[1]
    xp = r(x) @ wih.t() + bias
    h = torch.zeros(B, H, dtype=x.dtype)
    c = torch.zeros(B, H, dtype=x.dtype)
    outs = []
    for t in range(T):
        i, f, g, o = (xp[:, t] + r(h) @ whh.t()).chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs, 1)


def mixer(sd, img, ps, r=_ident):
    """img (N, H, W) -> (N, 88, dim)."""
    m = PRE + "mlp."
    N, Hh, Ww = img.shape
    P = img.reshape(N, Hh // ps, ps, Ww // ps, ps).permute(0, 1, 3, 2, 4).reshape(N, -1, ps * ps)
    Z = r(P) @ r(sd[m + "1.weight"]).t() + sd[m + "1.bias"]
    D = Z.shape[-1]
    Y1 = r(F.layer_norm(Z, (D,), sd[m + "2.0.norm.weight"], sd[m + "2.0.norm.bias"]))
    w1, w2 = r(sd[m + "2.0.fn.0.weight"][:, :, 0]), r(sd[m + "2.0.fn.3.weight"][:, :, 0])
    U = torch.einsum("on,bnd->bod", w1, Y1) + sd[m + "2.0.fn.0.bias"][:, None]
    Z1 = Z + torch.einsum("no,bod->bnd", w2, r(F.gelu(U))) + sd[m + "2.0.fn.3.bias"][:, None]
    Y2 = r(F.layer_norm(Z1, (D,), sd[m + "2.1.norm.weight"], sd[m + "2.1.norm.bias"]))
    U2 = Y2 @ r(sd[m + "2.1.fn.0.weight"]).t() + sd[m + "2.1.fn.0.bias"]
    Z2 = Z1 + r(F.gelu(U2)) @ r(sd[m + "2.1.fn.3.weight"]).t() + sd[m + "2.1.fn.3.bias"]
    return F.conv1d(r(Z2), r(sd[m + "3.weight"]), sd[m + "3.bias"], padding=1)


def forward(sd, x, lefts, lens=None, r=_ident, crop_len=128, ps=32):
    """(pred (B, classes), d_vec (B, dim_emb)); row b is x[b, :lens[b]] when lens is given."""
    B, T, _ = x.shape
    rows = lefts_rows(lefts, B)
    h = lstm(sd, x, r)
    e1 = torch.stack([h[b, (lens[b] if lens is not None else T) - 1] for b in range(B)])
    h16 = r(h)
    e2 = 0
    for row in rows:
        win = torch.stack([h16[b, lf:lf + crop_len] for b, lf in enumerate(row)])  # (B, W, E): W channels
        a = F.conv1d(win, r(sd[PRE + "conv_1.conv.weight"]), sd[PRE + "conv_1.conv.bias"], padding=1)
        e2 = e2 + mixer(sd, a, ps, r)[:, -1, :]
    e2 = e2 / len(rows)
    emb = torch.cat((e1, e2), 1) @ sd[PRE + "dv.weight"].t() + sd[PRE + "dv.bias"]
    d_vec = emb / emb.norm(p=2, dim=-1, keepdim=True)
    return emb @ sd[PRE + "output.weight"].t() + sd[PRE + "output.bias"], d_vec


def emulate_bf16(sd, x, lefts, lens=None):
    """The forward-only bf16 path's rounding points on the CPU (fp32 state and accumulation)."""
    with torch.no_grad():
        return forward({k: v.float() for k, v in sd.items()}, x.float(), lefts, lens, r=bf16_round)


def step_loss(pred, d_vec, e, labels):
    return F.cosine_embedding_loss(d_vec, e, torch.ones(d_vec.shape[0], dtype=d_vec.dtype)) + F.cross_entropy(pred, labels)
