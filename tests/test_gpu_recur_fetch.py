"""The decoder recurrences and what queues in front of their flag poll: the lstm2 backward selects its
layer's pointers instead of loading them on every tick, reads its quit word by inline asm, and its
cell-phase barriers wait for LDS alone (profiles/r7_recur_fetch_ab.txt).  The lstm2 forward and the
single-layer kernels are as they were and are covered all the same: the hand-off protocol is shared.
None of this changes a summation order, so besides the references (fp32 / fp64 loops with the kernels'
roundings, and the two single-layer launches for the lstm2 backward) every output is compared bit for
bit with the outputs recorded from the kernels of the commit before (tests/golden/recur_fetch.json:
SHA-256 of each output's bytes; the inputs come from an integer generator, so they are the same bytes
on every machine).  Every case asserts that the spin-timeout word is 0.

Shapes: H = 1024 groups are 16 utterances, H = 512 groups are 8.  T = 1 has no hand-off, T = 2 the first
fill (layer 1's tile absent), T = 3 both parity slots; B = 17 / 9 a group with one live row (zero rows),
B = 20 a ragged last group."""
import functools
import hashlib
import json
import os

import pytest
import torch

from .helpers import ref_bwd, ref_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recur_fetch.json")
FWD2_BAR = 3e-3  # test_lstm2_wavefront_forward's
STEP_BAR = 2e-3  # test_gpu_lstm_paths.STEP_BAR, test_lstm_persistent_forward / backward's
PAIR_BAR = 2e-3  # test_gpu_lstm2_bwd's
DB_BAR = 1e-5    # test_lstm2_wavefront_bias_partials_and_bf16_only_outputs'


def relf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def _kr():
    import autoformer_amd as A
    from autoformer_amd import kernels as Kr

    A.set_compute("bf16")
    return Kr


def _u(shape, seed, lo=-1.0, hi=1.0):
    """Uniform values in [lo, hi) from a 32-bit integer hash of the element index: exact in fp32, the same
    bytes on every machine and torch version."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    x = (i * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 2246822519) & 0xFFFFFFFF
    x = ((x ^ (x >> 13)) * 3266489917) & 0xFFFFFFFF
    x = (x ^ (x >> 16)) >> 8  # 24 bits
    return (x.to(torch.float32) / 16777216.0 * (hi - lo) + lo).reshape(shape)


def _gates(B, T, H, seed):
    g = _u((B * T, 4, H), seed, 0.05, 0.95)
    g[:, 2] = g[:, 2] * 2 - 1  # g gate in (-1, 1)
    return g.reshape(B * T, 4 * H)


# ------------------------------------------------------------------ lstm2 forward
@functools.lru_cache(maxsize=None)
def _fwd2_inputs(B, T):
    H = 1024
    G = 4 * H
    xproj = _u((B * T, G), 1) * 0.9
    ws = tuple((_u((G, H), 2 + i) * (1.7 / H ** 0.5)).bfloat16() for i in range(3))
    bias1 = _u((G,), 7) * 0.2
    return xproj, ws, bias1


def _fwd2_run(B, T):
    Kr = _kr()
    H = 1024
    assert Kr.lstm2_persistent(B, H, H)
    xproj, ws, bias1 = _fwd2_inputs(B, T)
    out = Kr.lstm2_fwd(xproj.to(DEV), *[w.to(DEV) for w in ws], bias1.to(DEV), B, T, H)
    torch.cuda.synchronize()
    assert int(Kr._CACHE["lstm2_buf"].view(torch.int32)[0].item()) == 0
    Kr.check_faults()
    return out


@functools.lru_cache(maxsize=None)
def _fwd2_ref(B, T):
    """test_lstm2_wavefront_forward's fp32 CPU loop: bf16 weights, h of both layers rounded to bf16 for
    the products.  Computed once per shape; read-only."""
    H = 1024
    G = 4 * H
    xproj, ws, bias1 = _fwd2_inputs(B, T)
    w0, wi1, w1 = [w.float() for w in ws]
    xp = xproj.view(B, T, G)
    hs = [torch.zeros(B, H), torch.zeros(B, H)]
    cs = [torch.zeros(B, H), torch.zeros(B, H)]
    outs, gts = [[], []], [[], []]
    for t in range(T):
        for L in range(2):
            if L == 0:
                pre = xp[:, t] + hs[0].bfloat16().float() @ w0.t()
            else:
                pre = bias1 + outs[0][t].bfloat16().float() @ wi1.t() + hs[1].bfloat16().float() @ w1.t()
            i, f, gg, o = pre.chunk(4, 1)
            i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
            cs[L] = f * cs[L] + i * gg
            hs[L] = o * torch.tanh(cs[L])
            outs[L].append(hs[L])
            gts[L].append(torch.cat([i, f, gg, o], 1))
    return ([torch.stack(outs[L], 1).reshape(B * T, H) for L in range(2)], cs,
            [torch.stack(gts[L], 1).reshape(B * T, G) for L in range(2)])


@pytest.mark.parametrize("B,T", [(16, 1), (16, 2), (17, 3), (20, 5), (64, 4)])
def test_lstm2_forward_against_cpu_loop(B, T):
    H = 1024
    h0, c0, g0, h1, c1, g1 = _fwd2_run(B, T)
    href, cref, gref = _fwd2_ref(B, T)
    for L, (h, c, g) in enumerate(((h0, c0, g0), (h1, c1, g1))):
        errs = (relf(h, href[L]), relf(c.cpu().view(B, T, H)[:, -1], cref[L]), relf(g, gref[L]))
        print(f"lstm2 fwd B{B} T{T} layer {L}: h {errs[0]:.2e} last c {errs[1]:.2e} gates {errs[2]:.2e}")
        assert max(errs) < FWD2_BAR, (L, errs)
        assert torch.equal(h._bf16, h.to(torch.bfloat16)), L


# ------------------------------------------------------------------ lstm2 backward
@functools.lru_cache(maxsize=None)
def _bwd2_inputs(B, T):
    H = 1024
    dh = _u((B * T, H), 11) * 0.2
    cs = tuple(_u((B * T, H), 12 + i) * 1.2 for i in range(2))
    gs = tuple(_gates(B, T, H, 14 + i) for i in range(2))
    ws = tuple((_u((H, 4 * H), 16 + i) * (1.7 / H ** 0.5)).bfloat16() for i in range(3))  # W_hh0^T, W_ih1^T, W_hh1^T
    return dh, cs, gs, ws


def _bwd2_run(B, T, db, fp32=True):
    Kr = _kr()
    H = 1024
    assert Kr.lstm2_bwd_persistent(B, H)
    dh, cs, gs, ws = _bwd2_inputs(B, T)
    out = Kr.lstm2_bwd(dh.to(DEV), cs[0].to(DEV), gs[0].to(DEV), cs[1].to(DEV), gs[1].to(DEV),
                       *[w.to(DEV) for w in ws], B, T, H, fp32=fp32, db=db)
    torch.cuda.synchronize()
    assert int(Kr._CACHE["lstm2_bwd_buf"].view(torch.int32)[0].item()) == 0
    Kr.check_faults()
    return out


@functools.lru_cache(maxsize=None)
def _bwd2_two_launches(B, T):
    """The path the wavefront replaces: layer 1's single-layer persistent backward, dX1 = dG1 W_ih1 from its
    bf16 dG (an fp32 product of the same bf16 values), layer 0's launch on that.  Once per shape; read-only."""
    Kr = _kr()
    H = 1024
    dh, cs, gs, ws = _bwd2_inputs(B, T)
    wt0, wti1, wt1 = [w.to(DEV) for w in ws]
    dhd = dh.to(DEV)
    gb = Kr.lstm_bwd_scratch(B, H, 1, DEV)
    dg1 = Kr.lstm_bwd(dhd, dhd, cs[1].to(DEV), gs[1].to(DEV), None, wt1, B, T, H, 1, gbuf=gb)
    torch.cuda.synchronize()
    assert Kr.lstm_bwd_timeout_flag(gb, B, H) == 0
    dx1 = (dg1._bf16.double() @ wti1.double().t()).float()
    dg0 = Kr.lstm_bwd(dx1, dx1, cs[0].to(DEV), gs[0].to(DEV), None, wt0, B, T, H, 1, gbuf=gb)
    torch.cuda.synchronize()
    assert Kr.lstm_bwd_timeout_flag(gb, B, H) == 0
    return dg0.cpu(), dg1.cpu()


@pytest.mark.parametrize("db", [False, True])
@pytest.mark.parametrize("B,T", [(16, 1), (17, 3), (64, 4)])
def test_lstm2_backward_against_two_launches(B, T, db):
    H = 1024
    out = _bwd2_run(B, T, db)
    r0, r1 = _bwd2_two_launches(B, T)
    e0, e1 = relf(out[0], r0), relf(out[1], r1)
    print(f"lstm2 bwd B{B} T{T} db={db}: dG0 {e0:.2e} dG1 {e1:.2e}")
    assert e0 < PAIR_BAR and e1 < PAIR_BAR, (e0, e1)
    for d in out[:2]:
        assert torch.equal(d._bf16, d.to(torch.bfloat16))
    if db:
        ng = -(-B // 16)
        for layer in range(2):
            ref = torch.zeros(ng * 16, T, 4 * H, dtype=torch.float64)
            ref[:B] = out[layer].double().cpu().view(B, T, 4 * H)
            e = relf(out[2][layer], ref.view(ng, 16 * T, 4 * H).sum(1))
            print(f"  bias partials layer {layer}: {e:.2e}")
            assert e < DB_BAR, (layer, e)


# ------------------------------------------------------------------ determinism, uneven load
def _all_equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        if getattr(x, "_bf16", None) is not None:
            assert torch.equal(x._bf16, y._bf16)


def test_two_launches_are_identical():
    _all_equal(_fwd2_run(20, 5), _fwd2_run(20, 5))
    _all_equal(_bwd2_run(17, 3, True), _bwd2_run(17, 3, True))


def test_lstm2_forward_handoff_under_uneven_load():
    """The wavefront forward's hand-off beside a stream of large GEMMs on a second stream, started 0, 1 and 3
    GEMMs ahead, as test_lstm_persistent_backward_under_load loads the chip: members start and run at different
    times and the payload lines compete with streaming traffic.  The arithmetic order is fixed, so a payload
    consumed before it landed, a stale line or a row that should have read as zero shows as a differing word."""
    B, T = 64, 8
    quiet = _fwd2_run(B, T)
    Kr = _kr()
    xproj, ws, bias1 = _fwd2_inputs(B, T)
    args = [xproj.to(DEV)] + [w.to(DEV) for w in ws] + [bias1.to(DEV)]
    side = torch.cuda.Stream()
    x = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    for lead in (0, 1, 3):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(lead):
                x = (x @ x).clamp_(-1, 1)
        loaded = Kr.lstm2_fwd(*args, B, T, 1024)
        with torch.cuda.stream(side):
            for _ in range(4):
                x = (x @ x).clamp_(-1, 1)
        torch.cuda.synchronize()
        assert int(Kr._CACHE["lstm2_buf"].view(torch.int32)[0].item()) == 0
        Kr.check_faults()
        _all_equal(loaded, quiet)


# ------------------------------------------------------------------ single-layer kernels
@functools.lru_cache(maxsize=None)
def _one_inputs(B, T, H):
    G = 4 * H
    xp = _u((B * T, G), 21) * 0.9
    whh = (_u((G, H), 22) * (1.7 / H ** 0.5)).bfloat16()
    dh = _u((B * T, H), 23) * 0.2
    c = _u((B * T, H), 24) * 1.2
    gates = _gates(B, T, H, 25)
    return xp, whh, dh, c, gates


def _one_fwd(B, T, H):
    Kr = _kr()
    assert Kr.lstm_persistent_fwd(B, H, 1)
    xp, whh, _, _, _ = _one_inputs(B, T, H)
    hb = Kr.lstm_scratch(B, H, 1, DEV)
    out = Kr.lstm_fwd(xp.to(DEV), whh.to(DEV), B, T, H, 1, hb)
    torch.cuda.synchronize()
    assert Kr.lstm_timeout_flag(hb, B, H) == 0
    Kr.check_faults()
    return out


def _one_bwd(B, T, H):
    Kr = _kr()
    assert Kr.lstm_persistent_bwd(B, H, 1)
    _, whh, dh, c, gates = _one_inputs(B, T, H)
    gb = Kr.lstm_bwd_scratch(B, H, 1, DEV)
    dhd = dh.to(DEV)
    dg = Kr.lstm_bwd(dhd, dhd, c.to(DEV), gates.to(DEV), None, whh.t().contiguous().to(DEV), B, T, H, 1, gbuf=gb)
    torch.cuda.synchronize()
    assert Kr.lstm_bwd_timeout_flag(gb, B, H) == 0
    Kr.check_faults()
    return dg


ONE_CASES = [(B, T, 512) for B in (8, 9, 64) for T in (1, 2, 3, 5)] + [(9, 3, 1024)]


@pytest.mark.parametrize("B,T,H", ONE_CASES)
def test_single_layer_forward(B, T, H):
    """lstm_persist_fwd against the float64 recurrence the per-step kernels are held to (bf16 weights, h_{t-1}
    rounded to bf16), at their bar."""
    xp, whh, _, _, _ = _one_inputs(B, T, H)
    h, c, g = _one_fwd(B, T, H)
    hr, cr, gr = ref_fwd(xp.view(B, T, -1).double(), whh.double(), B, T, H, 1, round_rec=True)
    errs = (relf(h, hr.reshape(h.shape)), relf(c, cr.reshape(c.shape)), relf(g, gr.reshape(g.shape)))
    print(f"lstm fwd B{B} T{T} H{H}: h {errs[0]:.2e} c {errs[1]:.2e} gates {errs[2]:.2e}")
    assert max(errs) < STEP_BAR, errs
    assert torch.equal(h._bf16, h.to(torch.bfloat16))


@pytest.mark.parametrize("B,T,H", ONE_CASES)
def test_single_layer_backward(B, T, H):
    _, whh, dh, c, gates = _one_inputs(B, T, H)
    dg = _one_bwd(B, T, H)
    ref = ref_bwd(dh.view(B, T, -1).double(), c.view(B, T, -1).double(), gates.view(B, T, -1).double(), whh.double(),
                  B, T, H, 1, round_rec=True)
    e = relf(dg, ref.reshape(dg.shape))
    print(f"lstm bwd B{B} T{T} H{H}: dG {e:.2e}")
    assert e < STEP_BAR, e
    assert torch.equal(dg._bf16, dg.to(torch.bfloat16))


@pytest.mark.parametrize("T,nc", [(4, 2), (6, 3)])
def test_fold_kernels(T, nc):
    """The lstm1 code fold (H = 512): step t reads row t / (T / nc) of the per-code projection and the backward
    sums dG over each code's frames.
    Forward bit-identical to the ordinary launch on the expanded rows; the backward's bf16 dG likewise, its
    segment sums against fp64 sums of that launch's fp32 dG."""
    Kr = _kr()
    B, H = 9, 512
    G = 4 * H
    pcode = (_u((B * nc, G), 31) * 0.9).to(DEV)
    whh = (_u((G, H), 32) * (1.7 / H ** 0.5)).bfloat16().to(DEV)
    hb = Kr.lstm_scratch(B, H, 1, DEV)
    h1, c1, g1 = Kr.lstm_fwd_fold(pcode, nc, whh, B, T, H, hb)
    xproj = pcode.view(B, nc, 1, G).expand(B, nc, T // nc, G).reshape(B * T, G).contiguous()
    hb0 = Kr.lstm_scratch(B, H, 1, DEV)
    h0, c0, g0 = Kr.lstm_fwd(xproj, whh, B, T, H, 1, hb0)
    torch.cuda.synchronize()
    assert Kr.lstm_timeout_flag(hb, B, H) == 0 and Kr.lstm_timeout_flag(hb0, B, H) == 0
    hr, _, _ = ref_fwd(xproj.cpu().view(B, T, G).double(), whh.cpu().double(), B, T, H, 1, round_rec=True)
    assert relf(h0, hr.reshape(h0.shape)) < STEP_BAR
    assert torch.equal(h1, h0) and torch.equal(c1, c0) and torch.equal(g1, g0) and torch.equal(h1._bf16, h0._bf16)
    dh = (_u((B * T, H), 33) * 0.2).to(DEV)
    wt = whh.t().contiguous()
    gb = Kr.lstm_bwd_scratch(B, H, 1, DEV)
    dg16, sc = Kr.lstm_bwd_fold(dh, c0, g0, wt, B, T, H, nc, gbuf=gb)
    torch.cuda.synchronize()
    assert Kr.lstm_bwd_timeout_flag(gb, B, H) == 0
    dg = Kr.lstm_bwd(dh, h0, c0, g0, None, wt, B, T, H, 1)
    torch.cuda.synchronize()
    Kr.check_faults()
    assert torch.equal(dg16, dg._bf16)
    ref = dg.double().view(B, nc, T // nc, G).sum(2).reshape(B * nc, G)
    e = relf(sc, ref)
    print(f"fold T{T} nc{nc}: segment sums {e:.2e}")
    assert e < 1e-6, e  # test_lstm_fold_kernels_match_expanded_launch's bar
    assert torch.equal(sc._bf16, sc.bfloat16())


# ------------------------------------------------------------------ bit-identity to the parent commit
def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def golden_digests():
    """{output name: SHA-256 of its bytes} of the four kernels at the recorded shapes."""
    d = {}
    names = ("h0", "c0", "g0", "h1", "c1", "g1")
    for n, t in zip(names, _fwd2_run(20, 5)):
        d[f"lstm2_fwd_B20_T5/{n}"] = _sha(t)
        if n[0] == "h":
            d[f"lstm2_fwd_B20_T5/{n}_bf16"] = _sha(t._bf16)
    dg0, dg1, dbp = _bwd2_run(17, 3, True)
    for n, t in (("dg0", dg0), ("dg1", dg1), ("dg0_bf16", dg0._bf16), ("dg1_bf16", dg1._bf16), ("db_part", dbp)):
        d[f"lstm2_bwd_B17_T3/{n}"] = _sha(t)
    for H in (512, 1024):
        h, c, g = _one_fwd(20, 5, H)
        for n, t in (("h", h), ("c", c), ("g", g), ("h_bf16", h._bf16)):
            d[f"lstm_fwd_B20_T5_H{H}/{n}"] = _sha(t)
        dg = _one_bwd(17, 3, H)
        d[f"lstm_bwd_B17_T3_H{H}/dg"] = _sha(dg)
        d[f"lstm_bwd_B17_T3_H{H}/dg_bf16"] = _sha(dg._bf16)
    return d


def test_outputs_bit_identical_to_parent_commit():
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    got = golden_digests()
    assert set(got) == set(want)
    diff = sorted(k for k in want if got[k] != want[k])
    assert not diff, diff
