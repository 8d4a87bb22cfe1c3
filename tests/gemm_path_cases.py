"""The table behind tests/test_gpu_gemm_paths.py: one row per avc_gemm kernel path and epilogue form
(pure data, importable without a GPU: tests/test_gemm_path_table.py checks that every kernel family and
variant avc_gemm_last_path can name is the expected value of some row).

A row is (descriptor recipe, expected witness).  Shapes are the smallest that cross a tile edge in
every dimension (row tiles of 128, column tiles of 64 or 128, K tiles of 32 / 64) and land on the
listed kernel by the predicates of gemm_impl, gemm_ring_launch, gemm_conv_launch, gemm_nt_launch,
gemm_tt_launch and make_op (gemm*.hip); the reason is noted per group.
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

from autoformer_amd._lib import (PATH_BNB, PATH_CONV, PATH_FAST, PATH_GENERIC, PATH_NT, PATH_POST_PASS, PATH_RING,
                                 PATH_SPLITK_WS, PATH_TT, PATH_VARIANT_SHIFT, PATH_WINDOW)

# the variants avc_gemm_last_path can name per family (include/autovc_hip.h)
PATH_FAMILY_VARIANTS = {PATH_GENERIC: (0,), PATH_FAST: (1, 2), PATH_NT: (1, 2), PATH_CONV: (0,), PATH_TT: (1, 2, 3),
                        PATH_RING: (1, 2, 3)}


def gemm_path(family: int, variant: int = 0, flags: int = 0) -> int:
    """The avc_gemm_last_path value of (family, variant, flag bits)."""
    return family | (variant << PATH_VARIANT_SHIFT) | flags


def op(ks=False, dt="bf16", win=None, batched=False):
    """Operand recipe: K-strided?, storage dtype, frame window (taps, pad, t_out, t_in, chans), own batch."""
    return {"ks": ks, "dt": dt, "win": win, "batched": batched}


@dataclass
class Case:
    name: str
    family: str            # report label
    M: int
    N: int
    K: int
    expect: int            # avc_gemm_last_path
    comp: str = "bf16"
    a: dict = field(default_factory=op)
    b: dict = field(default_factory=op)
    ring: int = -1         # avc_gemm_set_ring mode: -1 default policy, 0 off, 1 forced to the 128 x 128 x 4 tile
    batch: int = 1
    bsum: bool = False     # the batch summed into one C (c_batch_stride == 0)
    fold: bool = False     # contiguous A / C batches sharing B: gemm_impl folds them into one product
    split: int = 1
    bias: bool = False
    res: bool = False
    acc: bool = False
    # guard columns: ldc = N + ldc_pad.  None = every row has them: 3 on the generic and fast kernels (scalar
    # stores, rows not 16-B aligned), 8 elsewhere (a multiple of 8 keeps the 16-B vector stores of the ring,
    # the tt halo cperm epilogue and the bf16-only C on their paths); 0 only where the descriptor needs
    # ldc == N: avc_gemm_bnb, whose y shares C's ldc
    ldc_pad: Optional[int] = None
    cperm: int = 0
    row_bias: Optional[Tuple[int, int]] = None  # (T, pad)
    twin: bool = False     # bf16 twin beside the fp32 C
    c16only: bool = False  # bf16-only C
    bn: Optional[int] = None   # 0: bn_partial + separate finalize; n >= 1: avc_gemm_bn with nupd = n
    bnb: Optional[int] = None  # avc_gemm_bnb with this activation (1 ReLU, 2 tanh)
    col_sum: bool = False  # col_sum[n] += column sums of the stored C
    shared: Optional[str] = None  # key of operand values / reference shared by several rows
    tags: Tuple[str, ...] = ()

    def __post_init__(self):
        if self.ldc_pad is None:
            self.ldc_pad = 0 if self.bnb is not None else 3 if self.family in ("generic", "fast64", "fast128") else 8


CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


LAYOUTS = [("nn", False, False), ("nt", False, True), ("tn", True, False), ("tt", True, True)]
DTYPES = [("bf16", "bf16"), ("f32", "bf16"), ("bf16", "f32"), ("f32", "f32")]
GEN, F64, F128 = gemm_path(PATH_GENERIC), gemm_path(PATH_FAST, 1), gemm_path(PATH_FAST, 2)

# ------------------------------------------------------------------ generic kernel, (131, 70, 37)
# fp32 compute never takes the bf16 fast path; under bf16 compute no operand is vectorisable (make_op:
# K = 37 and the K-strided contiguous dimensions 131 and 70 are not multiples of 4)
for comp in ("fp32", "bf16"):
    dt = "f32" if comp == "fp32" else "bf16"
    g = dict(comp=comp, a=op(dt=dt), b=op(dt=dt))
    for ln, aks, bks in LAYOUTS:
        add(f"generic-{comp}-{ln}", "generic", 131, 70, 37, GEN, comp=comp, a=op(aks, dt), b=op(bks, dt))
    add(f"generic-{comp}-bias-res", "generic", 131, 70, 37, GEN, bias=True, res=True, **g)
    add(f"generic-{comp}-acc", "generic", 131, 70, 37, GEN, acc=True, **g)
    add(f"generic-{comp}-ldc", "generic", 131, 70, 37, GEN, ldc_pad=3, **g)
    add(f"generic-{comp}-split3", "generic", 131, 70, 37, GEN, split=3, ldc_pad=3, **g)
    add(f"generic-{comp}-split3-acc", "generic", 131, 70, 37, GEN, split=3, acc=True, **g)
    add(f"generic-{comp}-batch3", "generic", 131, 70, 37, GEN, comp=comp, a=op(dt=dt, batched=True),
        b=op(dt=dt, batched=True), batch=3, ldc_pad=3)
    add(f"generic-{comp}-batchsum", "generic", 131, 70, 37, GEN, comp=comp, a=op(dt=dt, batched=True),
        b=op(dt=dt, batched=True), batch=3, bsum=True)
    add(f"generic-{comp}-cperm5", "generic", 131, 70, 37, GEN, cperm=5, **g)
    # row_bias needs M % rb_t == 0 (131 is prime): 12 utterances of 11 frames
    add(f"generic-{comp}-rowbias", "generic", 132, 70, 37, GEN, row_bias=(11, 2), bias=True, **g)
    # windows: 5 channels (not vectorisable), 4 utterances of 11 frames
    add(f"generic-{comp}-win-same", "generic", 44, 70, 15, GEN, comp=comp, a=op(dt=dt, win=(3, 1, 11, 11, 5)), b=op(dt=dt))
    add(f"generic-{comp}-win-valid", "generic", 36, 70, 15, GEN, comp=comp, a=op(dt=dt, win=(3, 0, 9, 11, 5)), b=op(dt=dt))
    # the data gradient of that valid conv: pad = Kw - 1 - pad = 2 over its 9-frame output gradient
    add(f"generic-{comp}-win-dgrad", "generic", 44, 70, 15, GEN, comp=comp, a=op(dt=dt, win=(3, 2, 11, 9, 5)), b=op(dt=dt))
    # the weight gradient: K-strided B window over the frames (K = 4 x 11), A = dy K-strided
    add(f"generic-{comp}-win-wgrad", "generic", 70, 15, 44, GEN, comp=comp, a=op(True, dt),
        b=op(True, dt, win=(3, 1, 11, 11, 5)), split=2)
    for sh in (1, -1):  # the LSTM h_{t-1} / h_{t+1} time shift
        add(f"generic-{comp}-shift{sh:+d}", "generic", 70, 5, 44, GEN, comp=comp, a=op(True, dt),
            b=op(True, dt, win=(1, sh, 11, 11, 5)))

# ------------------------------------------------------------------ fast kernel, every instance
# 64-wide, (132, 68, 100): vectorisable (every contiguous dimension % 4 == 0); bf16/bf16 NN stays off the
# ring and gemm_nt.hip because K % 8 == 4, bf16/bf16 TT off gemm_tt.hip because M % 8 == 4; mixed layouts
# and fp32-stored operands have no other kernel.  2 x 1 128-wide tiles < 384 -> the narrow rule.
# 128-wide, (2500, 2500, 68): 20 x 20 = 400 tiles >= 384; K % 8 == 4 and M % 8 == 4 as above.
for (M, N, K, w, exp, sh) in ((132, 68, 100, 64, F64, "f64"), (2500, 2500, 68, 128, F128, "f128")):
    for ln, aks, bks in LAYOUTS:
        for adt, bdt in DTYPES:
            add(f"fast{w}-{ln}-{adt}-{bdt}", f"fast{w}", M, N, K, exp, a=op(aks, adt), b=op(bks, bdt), shared=sh,
                tags=(f"fast{w}-instance",))

# epilogue forms on the 64-wide NN instance with A stored as fp32
fa = dict(a=op(dt="f32"), b=op())
add("fast-bias-res-twin", "fast64", 132, 68, 100, F64, bias=True, res=True, twin=True, ldc_pad=4, **fa)
add("fast-c16only", "fast64", 132, 68, 100, F64, c16only=True, bias=True, **fa)
add("fast-acc", "fast64", 132, 68, 100, F64, acc=True, ldc_pad=4, **fa)
# K = 200 in 3 splits: klen = 128, the third split owns no K tile
add("fast-split3-empty", "fast64", 132, 68, 200, F64, split=3, **fa)
add("fast-split3-acc", "fast64", 132, 68, 200, F64, split=3, acc=True, ldc_pad=4, **fa)
add("fast-batch3", "fast64", 132, 68, 100, F64, a=op(dt="f32", batched=True), b=op(batched=True), batch=3, bias=True)
add("fast-batch3-fold", "fast64", 132, 68, 100, F64, a=op(dt="f32", batched=True), b=op(), batch=3, fold=True, res=True)
add("fast-batchsum", "fast64", 132, 68, 100, F64, a=op(dt="f32", batched=True), b=op(batched=True), batch=3, bsum=True)
add("fast-cperm5", "fast64", 132, 60, 100, F64, cperm=5, **fa)
add("fast-rowbias", "fast64", 132, 68, 100, F64, row_bias=(11, 2), bias=True, **fa)
add("fast-bn-partial", "fast64", 132, 68, 100, F64, bn=0, bias=True, **fa)  # the last row tile holds 4 rows
add("fast-bn-fin1", "fast64", 132, 68, 100, F64, bn=1, bias=True, **fa)
add("fast-bn-fin2", "fast64", 132, 68, 100, F64, bn=2, bias=True, **fa)
add("fast-bnb", "fast64", 132, 68, 100, F64 | PATH_BNB, bnb=2, **fa)  # fused on this kernel for NN
add("fast-bnb-relu-c16", "fast64", 132, 68, 100, F64 | PATH_BNB, bnb=1, c16only=True, **fa)
# windows: 12 channels (vectorisable, not % 8), 12 utterances of 11 frames
add("fast-win-a", "fast64", 132, 68, 36, F64, a=op(dt="f32", win=(3, 1, 11, 11, 12)), b=op(), bias=True)
add("fast-win-b-kstrided", "fast64", 132, 36, 44, F64, a=op(dt="f32"), b=op(True, win=(3, 1, 11, 11, 12)))

# ------------------------------------------------------------------ gemm_nt.hip (bf16, both K-contiguous)
NT64, NT128 = gemm_path(PATH_NT, 1), gemm_path(PATH_NT, 2)
RING_GEMM, RING_HALO, RING_UTT = gemm_path(PATH_RING, 1), gemm_path(PATH_RING, 2), gemm_path(PATH_RING, 3)
add("nt64-ring-off", "nt", 130, 72, 72, NT64, ring=0, bias=True, res=True, twin=True)
# split-K is atomic, which the ring declines: default mode reaches gemm_nt.hip; klen 128, empty last split
add("nt64-split3-atomics", "nt", 130, 72, 200, NT64, split=3, bias=True)
# 128-wide: N >= 1024 and K >= 2048
add("nt128-ring-off", "nt", 130, 1032, 2048, NT128, ring=0, shared="nt128", bias=True)
add("nt128-split2", "nt", 130, 1032, 2048, NT128, split=2, shared="nt128")
WIN3 = (3, 1, 11, 11, 8)  # 4 utterances of 11 frames, 8 channels
add("nt-win-default-is-ring", "ring", 44, 72, 24, RING_GEMM, a=op(win=WIN3), bias=True)
add("nt-win-ring-off", "nt", 44, 72, 24, NT64 | PATH_WINDOW, ring=0, a=op(win=WIN3), bias=True)
add("nt64-bnb", "nt", 130, 72, 72, NT64 | PATH_BNB, ring=0, bnb=2)
add("nt128-bnb", "nt", 130, 1032, 2048, NT128 | PATH_BNB, ring=0, bnb=2, shared="nt128")
add("nt-win-bnb", "nt", 44, 72, 24, NT64 | PATH_WINDOW | PATH_BNB, ring=0, a=op(win=WIN3), bnb=1)
# col_sum is an epilogue of the ring kernels only: every other kernel stores C and a pass follows
add("nt64-colsum-pass-after", "nt", 130, 72, 72, NT64 | PATH_POST_PASS, ring=0, col_sum=True, bias=True)
add("generic-colsum-pass-after", "generic", 131, 70, 37, GEN | PATH_POST_PASS, col_sum=True)
add("fast-colsum-pass-after", "fast64", 132, 68, 100, F64 | PATH_POST_PASS, col_sum=True, **fa)

# ------------------------------------------------------------------ gemm_conv.hip: 5-tap 'same' convs, bf16
CONV = gemm_path(PATH_CONV)


def conv(name, B, T, Cin, Cout, expect, family="conv", **k):
    add(name, family, B * T, Cout, 5 * Cin, expect, a=op(win=(5, 2, T, T, Cin)), **k)


for bn in (None, 0):
    sfx = "" if bn is None else "-bn"
    conv("conv-straddle" + sfx, 3, 37, 32, 72, CONV, bn=bn, bias=True)      # tiles straddle utterances
    conv("conv-short" + sfx, 1, 3, 32, 64, CONV, bn=bn, bias=True)          # utterance shorter than the halo
    conv("conv-n72" + sfx, 2, 130, 64, 72, CONV, bn=bn, bias=True)          # N < 128: no ring, no utterance tile
    conv("conv-t128-default-is-ring" + sfx, 2, 128, 32, 128, RING_HALO, family="ring", bn=bn, bias=True)
    conv("conv-t128-ring-off" + sfx, 2, 128, 32, 128, CONV, ring=0, bn=bn, bias=True)
conv("conv-bn-fin", 3, 37, 32, 72, CONV, bn=1, bias=True)
conv("conv-bnb", 3, 37, 32, 72, CONV | PATH_BNB, bnb=2)  # the ring takes avc_gemm_bnb on its halo tile only
conv("ring-halo-bnb", 2, 128, 32, 128, RING_HALO | PATH_BNB, family="ring", bnb=2)  # ring_bnb_epilogue
# the straddling BN-backward instance, which only a forced configuration reaches (T % 128 != 0): M = 150 is two
# row tiles, the second partial, both spanning utterances; N % 8 == 0 and ldc == N as avc_gemm_bnb needs
conv("ring-halo-bnb-straddle", 3, 50, 32, 72, RING_HALO | PATH_BNB, family="ring", ring=1, bnb=2)

# ------------------------------------------------------------------ gemm_tt.hip (bf16, both K-strided)
TT, TTW, TTH = gemm_path(PATH_TT, 1), gemm_path(PATH_TT, 2), gemm_path(PATH_TT, 3)
tt = dict(a=op(True), b=op(True))
add("tt-plain", "tt", 136, 72, 100, TT, tags=("tt1-single",), **tt)
add("tt-split3-ws", "tt", 136, 72, 100, TT | PATH_SPLITK_WS, split=3, tags=("tt1-ws",), **tt)
add("tt-split3-bias-atomics", "tt", 136, 72, 100, TT, split=3, bias=True, tags=("tt1-atomics",), **tt)
add("tt-split9-atomics", "tt", 136, 72, 580, TT, split=9, tags=("tt1-atomics",), **tt)  # past the bound of 8
add("tt-split3-ws-acc", "tt", 136, 72, 100, TT | PATH_SPLITK_WS, split=3, acc=True, **tt)
WS3 = (3, 1, 11, 11, 8)
add("tt-win", "tt", 72, 24, 44, TTW, a=op(True), b=op(True, win=WS3), tags=("tt2-single",))
add("tt-win-split2-ws", "tt", 72, 24, 44, TTW | PATH_SPLITK_WS, a=op(True), b=op(True, win=WS3), split=2, tags=("tt2-ws",))
add("tt-win-split2-bias-atomics", "tt", 72, 24, 44, TTW, a=op(True), b=op(True, win=WS3), split=2, bias=True,
    tags=("tt2-atomics",))
add("tt-shift", "tt", 72, 72, 44, TTW, a=op(True), b=op(True, win=(1, 1, 11, 11, 72)))
add("tt-shift-back", "tt", 72, 72, 44, TTW, a=op(True), b=op(True, win=(1, -1, 11, 11, 72)))
# halo: 5 taps x 32 channels, 3 utterances of 37 frames (T % 64 != 0: a partial K tile per utterance)
HALO = dict(a=op(True), b=op(True, win=(5, 2, 37, 37, 32)))
add("tt-halo", "tt", 72, 160, 111, TTH, tags=("tt3-single",), **HALO)
add("tt-halo-split3-ws", "tt", 72, 160, 111, TTH | PATH_SPLITK_WS, split=3, tags=("tt3-ws",), **HALO)
add("tt-halo-split9-atomics", "tt", 72, 160, 111, TTH, split=9, tags=("tt3-atomics",), **HALO)
add("tt-halo-cperm5", "tt", 72, 160, 111, TTH, cperm=5, **HALO)
add("tt-halo-cperm5-split3-ws", "tt", 72, 160, 111, TTH | PATH_SPLITK_WS, cperm=5, split=3, acc=True, **HALO)
add("tt-halo-acc", "tt", 72, 160, 111, TTH, acc=True, **HALO)

# ------------------------------------------------------------------ the ring, default policy
add("ring-gemm", "ring", 130, 72, 72, RING_GEMM, bias=True, res=True, twin=True)
add("ring-gemm-c16only", "ring", 130, 72, 72, RING_GEMM, bias=True, c16only=True)
add("ring-gemm-acc", "ring", 130, 72, 72, RING_GEMM, acc=True)
add("ring-gemm-colsum", "ring", 130, 72, 72, RING_GEMM, col_sum=True, bias=True)  # in the ring's own epilogue
conv("ring-utt", 2, 176, 32, 128, RING_UTT, family="ring", bias=True)  # 128 < T <= 192: one utterance per tile

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
