"""The decoder lstm2 wavefront kernels (lstm2.hip) after the work on what stands in front of wave 0's flag
poll (profiles/lstm2_poll_ab.txt): in the backward wave 0 issues its cells' inputs behind the poll and hands
its cells' dG to wave 1 through LDS, the A fragments are read at immediate offsets (no scratch), and the
compiler's own vmcnt(0) waits at the head of the tick and in chunk 0 are gone.  None of it changes the order
of a floating-point operation (tests/test_gpu_recur_fetch.py holds the outputs to the parent's bit for bit).

Here: every element of both kernels' outputs against the float64 per-step recurrences of tests/helpers.py,
the backward's hand-off beside a loaded second stream, and (no GPU needed) the two kernels' register and
scratch figures read from the compiler's metadata.

Shapes (H = 1024 is the only size the kernels take; groups are 16 utterances):
  (16, 1)  ticks 0 and T only: each runs with one layer idle, no hand-off is consumed twice
  (17, 3)  a second group with one live row (15 rows read the zero source), both payload parities
  (20, 5)  a ragged last group
  (33, 2)  three groups, the first fill only (layer 1's tile absent in tick 1)
Every tick with an exchange walks all four K-chunks of the backward.

Bars.  The kernels round the recurrent operand (h, dG) to bf16 and accumulate in fp32; the references round
the same operand to bf16 and work in float64.  What is left is fp32 accumulation (4096 terms, ~1e-6), the
v_exp / v_rcp activations (~1e-6) and, the largest, operand elements that round to the other bf16 neighbour
because the fp32 value differs from the float64 one in its last bits: each moves one of up to 4096 products by
2^-8 of that term.  The project holds these kernels to 2e-3 (tests/test_gpu_recur_fetch.py STEP_BAR / PAIR_BAR)
for dG and the states; here that bar is applied to every element, as |err| <= 2e-3 * max|ref| of the tensor
(a bar relative to each element's own magnitude is not meaningful for a sum of thousands of signed terms).
A bf16 output adds the format's own rounding, half an ulp = 2^-9 of the element.  The bias partials are sums of
the kernel's own fp32 dG over a group's utterances and steps and are held to those sums in float64: 1e-5 as
in tests/test_gpu_lstm2_bwd.py (norm-relative), and per element to the bound of a (T + 16)-deep fp32 sum."""
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch

from .helpers import ref_bwd, ref_fwd, sum_ratio
from .test_gpu_recur_fetch import _all_equal, _bwd2_inputs, _bwd2_run, _fwd2_inputs, _fwd2_run, _kr, relf

DEV = "cuda:0"
H = 1024
G = 4 * H
SHAPES = [(16, 1), (17, 3), (20, 5), (33, 2)]
BAR = 2e-3       # dG and the states
DB_BAR = 1e-5    # the bias partials
BF16_HALF_ULP = 2.0 ** -9


def _worst(got, ref, extra_rel=0.0):
    """max over the elements of |got - ref| / (BAR * max|ref| + extra_rel * |ref|): <= 1 passes."""
    got, ref = got.detach().cpu().double().reshape(ref.shape), ref.double()
    bar = BAR * ref.abs().max() + extra_rel * ref.abs()
    return float(((got - ref).abs() / bar).max())


# ------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def _bwd2_ref(B, T):
    """float64 dG of both layers (B, T, 4H): layer 1 from the upstream gradient, layer 0 from dX1 = dG1 W_ih1
    with dG1 rounded to bf16 (the payload the kernel multiplies).  Once per shape; read-only."""
    dh, cs, gs, ws = _bwd2_inputs(B, T)
    w0, wi1, w1 = [w.double().t().contiguous() for w in ws]  # (4H, H)
    v = lambda x, n: x.double().view(B, T, n)  # noqa: E731
    dg1 = ref_bwd(v(dh, H), v(cs[1], H), v(gs[1], G), w1, B, T, H, 1, round_rec=True)
    dx1 = dg1.bfloat16().double() @ wi1
    dg0 = ref_bwd(dx1, v(cs[0], H), v(gs[0], G), w0, B, T, H, 1, round_rec=True)
    return dg0, dg1


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
def test_lstm2_backward_every_element_against_fp64(B, T):
    r0, r1 = _bwd2_ref(B, T)
    d0, d1 = _bwd2_run(B, T, False)[:2]                # fp32 dG (+ its bf16 twin)
    e0, e1, dbp = _bwd2_run(B, T, True, fp32=False)    # the step's form: bf16 dG + bias partials
    for layer, (d, e, r) in enumerate(((d0, e0, r0), (d1, e1, r1))):
        w32, w16 = _worst(d, r), _worst(e.float(), r, BF16_HALF_ULP)
        print(f"lstm2 bwd B{B} T{T} layer {layer}: fp32 dG {w32:.3f} of bar, bf16 dG {w16:.3f} of bar, "
              f"norm-relative {relf(d, r.reshape(d.shape)):.2e}")
        assert w32 <= 1, (layer, w32)
        assert w16 <= 1, (layer, w16)
        assert e.dtype == torch.bfloat16 and torch.equal(e, d._bf16) and torch.equal(e, d.to(torch.bfloat16)), layer
        # bias partials: the kernel's own fp32 dG summed over each group's utterances and steps
        ng = -(-B // 16)
        full = torch.zeros(ng * 16, T, G, dtype=torch.float64)
        full[:B] = d.double().cpu().view(B, T, G)
        sums = full.view(ng, 16 * T, G).sum(1)
        sabs = full.abs().view(ng, 16 * T, G).sum(1)
        en, es = relf(dbp[layer], sums.reshape(dbp[layer].shape)), sum_ratio(dbp[layer], sums, sabs, T + 16)
        print(f"  bias partials: norm-relative {en:.2e}, worst element {es:.3f} of the ({T} + 16) * 2^-24 sum bound")
        assert en < DB_BAR, (layer, en)
        assert es <= 1, (layer, es)


# ------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=None)
def _fwd2_ref64(B, T):
    """float64 h, c, gates of both layers, h_{t-1} (and layer 1's input h0_t) rounded to bf16 for the products."""
    xproj, ws, bias1 = _fwd2_inputs(B, T)
    w0, wi1, w1 = [w.double() for w in ws]  # (4H, H)
    h0, c0, g0 = ref_fwd(xproj.double().view(B, T, G), w0, B, T, H, 1, round_rec=True)
    xp1 = bias1.double() + h0.bfloat16().double() @ wi1.t()
    h1, c1, g1 = ref_fwd(xp1, w1, B, T, H, 1, round_rec=True)
    return (h0, c0, g0), (h1, c1, g1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
def test_lstm2_forward_every_element_against_fp64(B, T):
    h0, c0, g0, h1, c1, g1 = _fwd2_run(B, T)
    refs = _fwd2_ref64(B, T)
    for layer, (h, c, g) in enumerate(((h0, c0, g0), (h1, c1, g1))):
        hr, cr, gr = refs[layer]
        ws = (_worst(h, hr), _worst(c, cr), _worst(g, gr), _worst(h._bf16.float(), hr, BF16_HALF_ULP))
        print(f"lstm2 fwd B{B} T{T} layer {layer}: h {ws[0]:.3f} c {ws[1]:.3f} gates {ws[2]:.3f} "
              f"bf16 h {ws[3]:.3f} of bar")
        assert max(ws) <= 1, (layer, ws)
        assert torch.equal(h._bf16, h.to(torch.bfloat16)), layer


# ------------------------------------------------------------------ hand-off under uneven load
@pytest.mark.gpu
def test_lstm2_backward_handoff_under_uneven_load():
    """test_lstm2_forward_handoff_under_uneven_load's mirror: the wavefront backward beside large GEMMs on a
    second stream, started 0, 1 and 3 GEMMs ahead, so members start and run at different times and the payload
    lines compete with streaming traffic.  Wave 0 now has its inputs and the fills in flight together under
    counted waits and another wave stores its cells: a tile read before it landed, a stale line or a store of
    the wrong tick shows as a differing word (the arithmetic order is fixed), a lost hand-off as the timeout
    word."""
    B, T = 64, 16
    Kr = _kr()
    dh, cs, gs, ws = _bwd2_inputs(B, T)
    args = [dh.to(DEV), cs[0].to(DEV), gs[0].to(DEV), cs[1].to(DEV), gs[1].to(DEV)] + [w.to(DEV) for w in ws]
    side = torch.cuda.Stream()
    x = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    for fp32, db in ((True, False), (False, True)):
        quiet = _bwd2_run(B, T, db, fp32=fp32)
        for lead in (0, 1, 3):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(lead):
                    x = (x @ x).clamp_(-1, 1)
            loaded = Kr.lstm2_bwd(*args, B, T, H, fp32=fp32, db=db)
            with torch.cuda.stream(side):
                for _ in range(4):
                    x = (x @ x).clamp_(-1, 1)
            torch.cuda.synchronize()
            assert int(Kr._CACHE["lstm2_bwd_buf"].view(torch.int32)[0].item()) == 0
            Kr.check_faults()
            _all_equal(loaded, quiet)


# ------------------------------------------------------------------ kernel resources (no GPU)
def _kernel_records(asm_text):
    """{kernel name: {field: int}} from the .amdgpu_metadata note of a gfx950 assembly file: the records
    between `amdhsa.kernels:` and the next top-level key, nothing of the instruction stream."""
    meta = asm_text[asm_text.index(".amdgpu_metadata"):asm_text.index(".end_amdgpu_metadata")]
    body = meta[meta.index("amdhsa.kernels:"):]
    recs = {}
    for rec in re.split(r"\n  - ", body)[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if not name:
            continue
        recs[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)",
            rec)}
    return recs


def test_lstm2_kernels_use_no_scratch(tmp_path):
    """Both wavefront kernels keep three H x 4H slices of weights in registers, one workgroup per CU: a spilled
    weight fragment is reloaded inside the tick, behind a wait for everything in flight.  Compiled for gfx950
    to assembly, each must report no private segment, no spilled VGPR and at most 256 VGPRs."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoformer_amd", "csrc")
    out = tmp_path / "lstm2.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                    os.path.join(csrc, "lstm2.hip"), "-o", str(out)], check=True, cwd=csrc,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    recs = _kernel_records(out.read_text())
    found = {}
    for kernel in ("lstm2_persist_fwd", "lstm2_persist_bwd"):
        names = [n for n in recs if kernel in n]
        assert len(names) == 1, (kernel, sorted(recs))
        r = recs[names[0]]
        found[kernel] = r
        print(f"{kernel}: {r}")
        assert r["private_segment_fixed_size"] == 0, (kernel, r)
        assert r["vgpr_spill_count"] == 0, (kernel, r)
        assert r["vgpr_count"] <= 256, (kernel, r)
    assert len(found) == 2
