"""The StarGAN trainer, the host side (no GPU): the ledger of the twelfth ABI header (include/autovc_hip_cycle.h)
and its refusals (every check precedes the launch), the iteration-kind schedule, the trainer's Config and command
line, and the fixtures of tests/test_gpu_train_stargan.py against its plain-torch twin."""
import ctypes
import os
import re

import pytest

from .conftest import ROOT

HEADER_CYCLE = os.path.join(ROOT, "include", "autovc_hip_cycle.h")


def test_the_modules_import():
    import autoformer_amd.cycle as cy
    import autoformer_amd.train_stargan as ts
    from autoformer_amd import kernels as K
    from autoformer_amd.train_gan import CriticStep, GanVer1Solver

    assert callable(cy.cycle_loss_block) and callable(K.cycle_loss) and callable(K.cycle_loss_grad)
    assert issubclass(ts.CycleStep, CriticStep) and issubclass(ts.StarGanSolver, GanVer1Solver)
    assert ts.CycleStep.vc_step is CriticStep.vc_step                           # inherited
    assert ts.LOG_KEYS == ["VC/loss_id", "VC/loss_id_psnt", "VC/loss_cd", "C/loss_trans", "C/loss_reconst", "D/loss",
                           "Cycle/loss"]                                       # train_with_stargan.py:51-59


# ----------------------------------------------------------------------- the twelfth header
def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_CYCLE).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\b(avc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_cycle_header_symbols():
    from autoformer_amd import _lib

    protos = _prototypes()
    assert protos == {"avc_cycle_loss_ws": 2, "avc_cycle_loss": 24, "avc_cycle_loss_grad": 35}
    assert set(protos) == set(_lib.exported_symbols_cycle())
    for name, n in protos.items():
        assert len(_lib._SIGS_CYCLE[name][1]) == n, (name, n)
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg()
               + _lib.exported_symbols_ragged() + _lib.exported_symbols_vocoder() + _lib.exported_symbols_ge2e()
               + _lib.exported_symbols_xent() + _lib.exported_symbols_critic())
    assert not set(protos) & set(earlier)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in protos if not hasattr(so, s)]                       # every declared symbol is built
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "cycle_loss.hip" in _lib.SOURCES
    src = open(HEADER_CYCLE).read()
    assert int(re.search(r"#define AVC_CYCLE_MAX_NX (\d+)LL", src).group(1)) == _lib.CYCLE_MAX_NX == 2 ** 31 - 1
    assert int(re.search(r"#define AVC_CYCLE_GRID (\d+)", src).group(1)) == _lib.CYCLE_GRID


def test_cycle_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(4096)

    def err():
        return Lb.avc_last_error().decode()

    def ins(a):
        return (a["e1"], a["lde1"], a["t1"], a["ldt1"], a["e2"], a["lde2"], a["t2"], a["ldt2"], a["B"], a["E"], a["pr"],
                a["n_r"], a["pf"], a["n_f"], a["x"], a["y"], a["n_x"])

    base = dict(e1=p, lde1=8, t1=p, ldt1=8, e2=p, lde2=8, t2=p, ldt2=8, B=4, E=8, pr=p, n_r=4, pf=p, n_f=4, x=p, y=p,
                n_x=64, out=p, ws=p, de1=p, ldde1=8, de2=p, ldde2=8, dr=p, df=p, dy=p)

    def fwd(**kw):
        a = dict(base, **kw)
        return Lb.avc_cycle_loss(*ins(a), None, 0.1, 1.0, 1.0, a["out"], a["ws"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return Lb.avc_cycle_loss_grad(*ins(a), 0.1, 1.0, 1.0, a["ws"], None, None, None, None, None, p, a["de1"],
                                      a["ldde1"], a["de2"], a["ldde2"], a["dr"], a["df"], a["dy"], None)

    for call, who in ((fwd, "avc_cycle_loss:"), (bwd, "avc_cycle_loss_grad:")):
        for name in ("e1", "t1", "e2", "t2", "pr", "pf", "x", "y", "ws"):
            assert call(**{name: None}) == -1 and who in err() and "null pointer" in err(), (who, name)
        assert call(B=0) == -1 and who in err() and "bad shape B = 0" in err()
        assert call(B=4097) == -1 and "bad shape B = 4097" in err()
        assert call(E=0) == -1 and "E = 0" in err()
        big = dict(E=4097, lde1=4097, ldt1=4097, lde2=4097, ldt2=4097, ldde1=4097, ldde2=4097)
        assert call(**big) == -1 and "E = 4097" in err()
        for ld in ("lde1", "ldt1", "lde2", "ldt2"):
            assert call(**{ld: 7}) == -1 and f"{ld} = 7 is below E = 8" in err(), ld
        for n in ("n_r", "n_f"):
            assert call(**{n: 0}) == -1 and f"{n} = 0" in err()
            assert call(**{n: 65537}) == -1 and f"{n} = 65537" in err()
        assert call(n_x=0) == -1 and "n_x = 0" in err()
        assert call(n_x=-5) == -1 and "n_x = -5" in err()
        assert call(n_x=2 ** 31) == -1 and "n_x = 2147483648" in err()
    assert fwd(out=None) == -1 and "out is required" in err()
    assert bwd(ldde1=7) == -1 and "ldde1 = 7 is below E = 8" in err()
    assert bwd(ldde2=7) == -1 and "ldde2 = 7 is below E = 8" in err()
    assert bwd(de1=None, ldde1=0, de2=None, ldde2=0, dr=None, df=None, dy=None) == 0   # nothing asked for: no launch
    for B, n_x in ((0, 8), (-1, 8), (4097, 8), (4, 0), (4, 2 ** 31)):
        assert Lb.avc_cycle_loss_ws(B, n_x) == 0, (B, n_x)
    for B in (1, 2, 5, 64, 4096):
        for n_x in (1, 28160, 2 ** 31 - 1):
            n = Lb.avc_cycle_loss_ws(B, n_x)
            assert n >= 4 * (6 * B + 3 + _lib.CYCLE_GRID) and n % 16 == 0, (B, n)


def test_wrappers_need_a_device():
    import torch

    from autoformer_amd import kernels as K
    from autoformer_amd.cycle import cycle_loss_block

    e, t, p, x = torch.randn(3, 8), torch.randn(3, 8), torch.rand(3), torch.randn(3, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cycle_loss_block(e, t, e, t, p, p, x, x, 0.1, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.cycle_loss(e, t, e, t, p, p, x, x, 0.1, 1.0, 1.0)


# ----------------------------------------------------------------------- the trainer
def test_the_iteration_kind_schedule():
    """A cycle iteration is train_with_stargan.py:138's condition; StarGanSolver's loop asks train_gan.critic_due,
    and takes a cycle_step exactly there (a stub step, no device)."""
    import torch

    from autoformer_amd.train_gan import critic_due
    from autoformer_amd.train_stargan import StarGanSolver

    class Step:
        def __init__(self):
            self.kinds = []

        def vc_step(self, x, emb):
            self.kinds.append("vc")
            return tuple(torch.tensor(float(v)) for v in (1, 2, 3))

        def cycle_step(self, x, emb, xt, et, lefts_trans, lefts_reconst):
            assert len(lefts_trans) == 4 and len(lefts_reconst) == 4
            self.kinds.append("cycle")
            n = float(len(self.kinds))
            return tuple(torch.tensor(v) for v in (1.0, 2.0, 3.0, n, n + 0.25, n + 0.5, n + 0.75))

        def check(self):
            pass

    class Mod:
        def train(self):
            return self

        def draw_lefts(self, T):
            return [0, 1, 2, T - 128]

    for n_critic in (1, 2, 3, 10):
        for pretrained_step in (0, 1, 5, 10):
            want = [(i + 1) % n_critic == 0 and (i + 1) > pretrained_step for i in range(24)]
            assert [critic_due(i, n_critic, pretrained_step) for i in range(24)] == want
            s = StarGanSolver.__new__(StarGanSolver)
            s.step, s.VC, s.C, s.D = Step(), Mod(), Mod(), Mod()
            s.n_critic, s.pretrained_step, s.num_iters, s.log_step, s.device = n_critic, pretrained_step, 24, 10 ** 6, "cpu"
            s.log_keys = list(__import__("autoformer_amd.train_stargan", fromlist=["LOG_KEYS"]).LOG_KEYS)
            s.vcc_loader = [(torch.zeros(2, 176, 80), torch.zeros(2, 256))]
            rows = s.train()
            assert s.step.kinds == ["cycle" if w else "vc" for w in want], (n_critic, pretrained_step)
            assert len(rows) == 24 and all(len(r) == 7 for r in rows)
            last = [0.0] * 4
            for k, (r, w) in enumerate(zip(rows, want)):                       # the latest cycle iteration's; 0.0 before
                if w:
                    last = [k + 1.0, k + 1.25, k + 1.5, k + 1.75]
                assert r == [1.0, 2.0, 3.0] + last, (k, r)


REFERENCE_CONFIG = dict(num_speaker=80, lambda_cd=1, lambda_cls=0.1, lambda_dis=1, lambda_cycle=1, n_critic=10,
                        batch_size=2, len_crop=176, dim_neck=44, dim_emb=256, dim_pre=512, freq=22, log_step=10)


def test_config_and_parser_defaults_equal_the_reference():
    from autoformer_amd.train_stargan import Config, build_parser, config_from_args

    c = Config("AutoVC", "d", False, 1000)
    assert {k: getattr(c, k) for k in REFERENCE_CONFIG} == REFERENCE_CONFIG       # train_with_stargan.py:246-265
    assert c.pretrained_step == 100 and Config("AutoVC", "d", False, 15).pretrained_step == 1
    a = build_parser().parse_args(["--data_dir", "d", "--classifier_ckpt", "f"])
    assert (a.model_name, a.use_adain, int(a.num_iters), a.save_model_name) == ("AutoVC", False, 10, None)
    assert (a.n_critic, a.lambda_cls, a.lambda_dis, a.lambda_cycle, a.batch_size, a.len_crop) == (10, 0.1, 1, 1, 2, 176)
    cfg = config_from_args(a)
    want = dict(REFERENCE_CONFIG, num_speaker=None)                            # the checkpoint's class count
    assert {k: getattr(cfg, k) for k in want} == want
    assert cfg.pretrained_step == 1 and cfg.classifier_ckpt == "f" and cfg.use_adain is False
    a = build_parser().parse_args(["--synthetic", "--det_init", "--num_iters", "40", "--pretrained_step", "0",
                                   "--n_critic", "2", "--use_adain", "1", "--model_name", "AutoVC2", "--lambda_cycle",
                                   "0.5"])
    cfg = config_from_args(a)
    assert (cfg.num_iters, cfg.pretrained_step, cfg.n_critic, cfg.use_adain, cfg.lambda_cycle) == (40, 0, 2, True, 0.5)


def test_cli_refusals():
    from autoformer_amd.train_stargan import main

    with pytest.raises(SystemExit, match="--len_crop 160: the Discriminator is hard-wired to 176 frames"):
        main(["--synthetic", "--det_init", "--len_crop", "160"])
    with pytest.raises(SystemExit, match="--len_crop 100: MetaDV crops windows of 128 frames"):
        main(["--synthetic", "--det_init", "--len_crop", "100"])
    with pytest.raises(SystemExit, match="--classifier_ckpt is required"):
        main(["--synthetic"])
    with pytest.raises(SystemExit, match="--data_dir or --synthetic"):
        main(["--det_init"])
    with pytest.raises(SystemExit, match="--n_critic 0: at least 1"):
        main(["--synthetic", "--det_init", "--n_critic", "0"])
    with pytest.raises(SystemExit, match="the \\*_Adjust models return four outputs"):
        main(["--synthetic", "--det_init", "--model_name", "AutoVC_Adjust"])
    with pytest.raises(SystemExit, match="--use_adain True with --model_name AutoVC: "):
        main(["--synthetic", "--det_init", "--use_adain", "1"])
    with pytest.raises(SystemExit, match="--use_adain False with --model_name MetaConv2: "):
        main(["--synthetic", "--det_init", "--model_name", "MetaConv2"])
    with pytest.raises(SystemExit, match="no such model"):
        main(["--synthetic", "--det_init", "--model_name", "NoSuchModel"])
    with pytest.raises(SystemExit, match="the HIP kernels need a GPU"):
        main(["--synthetic", "--det_init", "--device", "cpu"])


# ----------------------------------------------------------------------- the fixtures pin the twin
def test_the_fixture_pins_the_twin():
    from .test_gpu_train_stargan import check_fixture_pins_the_twin

    check_fixture_pins_the_twin()


def test_the_adain_fixture_pins_the_twin():
    from .test_gpu_train_stargan import check_adain_fixture_pins_the_twin

    check_adain_fixture_pins_the_twin()
