"""Shared comparison helpers for the GPU parity tests (SURVEY.md §8(c) bars)."""
import numpy as np
import torch


def rel_inf(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _bf16_round(x):
    return x.bfloat16().double()


def ref_fwd(xp, w, B, T, H, dirs, round_rec=False):
    """The LSTM recurrence (h0 = c0 = 0, direction 1 in reversed time) in float64.
    xp (B, T, dirs*4H), w (dirs*4H, H): h, c, activated gates, all (B, T, dirs*.) float64.
    round_rec rounds h_{t-1} to bf16 before the recurrent product, as the bf16 large-H kernels do."""
    G = 4 * H
    h = torch.zeros(B, T, dirs * H, dtype=torch.float64)
    c = torch.zeros_like(h)
    g = torch.zeros(B, T, dirs * G, dtype=torch.float64)
    for d in range(dirs):
        W = w[d * G:(d + 1) * G]
        hp = torch.zeros(B, H, dtype=torch.float64)
        cp = torch.zeros_like(hp)
        for s in range(T):
            t = T - 1 - s if d else s
            pre = xp[:, t, d * G:(d + 1) * G] + (_bf16_round(hp) if round_rec else hp) @ W.t()
            i, f, gg, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(
                pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            cp = f * cp + i * gg
            hp = o * torch.tanh(cp)
            h[:, t, d * H:(d + 1) * H] = hp
            c[:, t, d * H:(d + 1) * H] = cp
            g[:, t, d * G:(d + 1) * G] = torch.cat([i, f, gg, o], 1)
    return h, c, g


def ref_bwd(dh_out, c, g, w, B, T, H, dirs, round_rec=False, c0=None):
    """dL/d(pre-activation gates) (B, T, dirs*4H) float64 from the forward's c and activated gates.
    round_rec rounds the previous backward step's dG to bf16 before the recurrent product; c0 (B, dirs*H)
    is the cell state before each direction's first step (default: zeros, as the kernels have it)."""
    G = 4 * H
    dg = torch.zeros(B, T, dirs * G, dtype=torch.float64)
    for d in range(dirs):
        W = w[d * G:(d + 1) * G]
        dgn = torch.zeros(B, G, dtype=torch.float64)
        dc = torch.zeros(B, H, dtype=torch.float64)
        for s in range(T):
            t = s if d else T - 1 - s  # opposite to the forward
            tp = t + 1 if d else t - 1
            gt = g[:, t, d * G:(d + 1) * G]
            i, f, gg, o = gt[:, :H], gt[:, H:2 * H], gt[:, 2 * H:3 * H], gt[:, 3 * H:]
            ct = c[:, t, d * H:(d + 1) * H]
            c_first = torch.zeros_like(ct) if c0 is None else c0[:, d * H:(d + 1) * H]
            cp = c[:, tp, d * H:(d + 1) * H] if 0 <= tp < T else c_first
            dh = dh_out[:, t, d * H:(d + 1) * H] + (_bf16_round(dgn) if round_rec else dgn) @ W
            tc = torch.tanh(ct)
            dcs = dc + dh * o * (1 - tc * tc)
            dgn = torch.cat([dcs * gg * i * (1 - i), dcs * cp * f * (1 - f), dcs * i * (1 - gg * gg),
                             dh * tc * o * (1 - o)], 1)
            dc = dcs * f
            dg[:, t, d * G:(d + 1) * G] = dgn
    return dg


def grad_mismatches(model, g, tol=1e-2, head_tol=1e-2,
                    bn_fed_bias=lambda n: "conv.bias" in n and "postnet.convolutions.4" not in n):
    """Per-parameter check against the golden gradient norm (rel <= tol) and first-64-element
    head (max abs error <= head_tol * max(max|head|, rms of the whole golden tensor)): a head
    whose 64 elements happen to be far below the tensor's typical magnitude is held to the
    tensor's scale, not to its own (fp32 reassociation moves every element by ~1e-7 x rms).
    Parameters whose true gradient is analytically zero (conv biases feeding a training-mode
    BatchNorm; `bn_fed_bias`) get an absolute floor only: their golden values are fp32
    rounding noise."""
    bad = {}
    for name, p in model.named_parameters():
        ref_n = float(g["gnorm/" + name])
        got = p.grad.detach().cpu().double()
        head = g["ghead/" + name].astype(np.float64)
        err = np.abs(got.reshape(-1)[:64].numpy() - head).max()
        if bn_fed_bias(name):
            ok = err < 1e-6 + head_tol * np.abs(head).max()
        else:
            scale = max(np.abs(head).max(), ref_n / np.sqrt(max(p.numel(), 1)), 1e-6)
            ok = abs(got.norm().item() - ref_n) <= tol * ref_n + 1e-6 and err <= head_tol * scale
        if not ok:
            bad[name] = (got.norm().item(), ref_n, err)
    return bad


def bn_state_mismatches(model, g):
    bad = []
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            if not np.allclose(v.detach().cpu().numpy(), g["bn/" + k], rtol=1e-4, atol=1e-6):
                bad.append(k)
    return bad


def to_dev(g, dev, *keys):
    return [torch.from_numpy(g[k]).to(dev) for k in keys]


# ---------------------------------------------------------------- direct-kernel bars (fp64 references)
# Every helper returns error / bar, the worst element's: a test asserts `<= 1`, and the printed figure
# says how far inside (or outside) its bar a kernel is.
EPS32 = 2.0 ** -24   # unit roundoff of fp32 (round to nearest)
BF16_ULP = 2.0 ** -8  # bf16 keeps 8 significand bits: round-to-nearest is within 2^-8, relative


def f64(t):
    return t.detach().cpu().double()


def bits_equal(got, ref):
    """Bit-for-bit equality (so -0.0 != 0.0 and equal NaNs compare equal); same dtype and shape."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    return bool(torch.equal(got.view(it), ref.view(it)))


def _ratio(err, bar):
    """max err / bar with 0 / 0 = 0 and x / 0 = inf."""
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                      torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def roundings_ratio(got, ref, k):
    """Elementwise result of k fp32 roundings: |err| <= k * 2^-24 * |ref|."""
    ref = ref.double()
    return _ratio((f64(got).reshape(ref.shape) - ref).abs(), k * EPS32 * ref.abs())


def sum_ratio(got, ref, sum_abs, d):
    """fp32 sum whose terms pass through at most d dependent additions: |err| <= d * 2^-24 * sum|terms|."""
    ref = ref.double()
    return _ratio((f64(got).reshape(ref.shape) - ref).abs(), d * EPS32 * sum_abs.double().reshape(ref.shape))


def close_ratio(got, ref, rtol, atol):
    """torch.testing.assert_close's bar against a float64 reference: |err| <= atol + rtol * |ref|."""
    ref = ref.double()
    return _ratio((f64(got).reshape(ref.shape) - ref).abs(), atol + rtol * ref.abs())


def rinf_ratio(got, ref, bar):
    """max|err| / max|ref| over the bar (the rel-inf measure of the older direct tests)."""
    return rel_inf(f64(got).reshape(ref.shape).numpy(), ref.double().numpy()) / bar


def report(family, what, ratio):
    """One line per check (pytest -s shows it): the measured error as a fraction of its bar."""
    print(f"[direct] {family:10s} {what}: {ratio:.3g} of bar")
    return ratio
