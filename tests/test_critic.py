"""The GAN trainer, the host side (no GPU): the ledger of the eleventh ABI header (include/autovc_hip_critic.h)
and its refusals (every check precedes the launch), critic_due, the trainer's Config and command line."""
import ctypes
import os
import re

import pytest

from .conftest import ROOT

HEADER_CRITIC = os.path.join(ROOT, "include", "autovc_hip_critic.h")


def _prototypes():
    """name -> argument count of every avc_* prototype of the header."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_CRITIC).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\b(avc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


# ----------------------------------------------------------------------- the eleventh header
def test_critic_header_symbols():
    from autoformer_amd import _lib

    from .test_abi import declared_symbols

    protos = _prototypes()
    assert sorted(protos) == ["avc_critic_loss", "avc_critic_loss_grad", "avc_critic_loss_ws"]
    assert set(protos) == set(_lib.exported_symbols_critic())
    for name, n in protos.items():                                             # argument counts agree
        assert len(_lib._SIGS_CRITIC[name][1]) == n, (name, n)
    assert protos == {"avc_critic_loss_ws": 1, "avc_critic_loss": 16, "avc_critic_loss_grad": 22}
    earlier = (_lib.exported_symbols() + _lib.exported_symbols_dv() + _lib.exported_symbols_audio()
               + _lib.exported_symbols_resample() + _lib.exported_symbols_eval() + _lib.exported_symbols_seg()
               + _lib.exported_symbols_ragged() + _lib.exported_symbols_vocoder() + _lib.exported_symbols_ge2e()
               + _lib.exported_symbols_xent())
    assert not set(protos) & set(earlier)
    assert set(_lib.exported_symbols()) == set(declared_symbols())             # the first table is as it was
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in protos if not hasattr(so, s)]                       # every declared symbol is built
    assert _lib.lib().avc_abi_version() == 31 and _lib.ABI_VERSION == 31       # added without an ABI bump
    assert "critic_loss.hip" in _lib.SOURCES
    src = open(HEADER_CRITIC).read()
    lim = {k: int(v) for k, v in re.findall(r"#define AVC_CRITIC_MAX_(\w+) (\d+)", src)}
    assert lim == {"B": _lib.CRITIC_MAX_B, "E": _lib.CRITIC_MAX_E, "N": _lib.CRITIC_MAX_N}
    assert lim == {"B": 4096, "E": 4096, "N": 65536}


def test_critic_host_refusals_without_a_gpu():
    """Every check precedes the launch: the pointers are never dereferenced."""
    from autoformer_amd import _lib

    Lb = _lib.lib()
    p = ctypes.c_void_p(4096)

    def err():
        return Lb.avc_last_error().decode()

    def fwd(e=p, lde=8, t=p, ldt=8, B=4, E=8, pr=p, n_r=4, pf=p, n_f=4, base=None, out=p, ws=p, **_):
        return Lb.avc_critic_loss(e, lde, t, ldt, B, E, pr, n_r, pf, n_f, base, 0.1, 1.0, out, ws, None)

    def bwd(e=p, lde=8, t=p, ldt=8, B=4, E=8, pr=p, n_r=4, pf=p, n_f=4, ws=p, de=p, ldde=8, dr=p, df=p, **_):
        return Lb.avc_critic_loss_grad(e, lde, t, ldt, B, E, pr, n_r, pf, n_f, 0.1, 1.0, ws, None, None, None, p, de,
                                       ldde, dr, df, None)

    for call, who in ((fwd, "avc_critic_loss:"), (bwd, "avc_critic_loss_grad:")):
        for name in ("e", "t", "pr", "pf", "ws"):
            assert call(**{name: None}) == -1 and who in err() and "null pointer" in err(), (who, name)
        assert call(B=0) == -1 and who in err() and "bad shape B = 0" in err()
        assert call(B=4097) == -1 and "bad shape B = 4097" in err()
        assert call(E=0, lde=0, ldt=0) == -1 and "E = 0" in err()
        assert call(E=4097, lde=4097, ldt=4097, ldde=4097) == -1 and "E = 4097" in err()
        assert call(lde=7) == -1 and "lde = 7 is below E = 8" in err()
        assert call(ldt=7) == -1 and "ldt = 7 is below E = 8" in err()
        assert call(n_r=0) == -1 and "n_r = 0" in err()
        assert call(n_f=0) == -1 and "n_f = 0" in err()
        assert call(n_r=65537) == -1 and "n_r = 65537" in err()
        assert call(n_f=65537) == -1 and "n_f = 65537" in err()
    assert fwd(out=None) == -1 and "out is required" in err()
    assert bwd(ldde=7) == -1 and "ldde = 7 is below E = 8" in err()
    assert bwd(de=None, dr=None, df=None) == 0                                 # nothing asked for: no launch
    for B in (0, -1, 4097):
        assert Lb.avc_critic_loss_ws(B) == 0, B
    for B in (1, 2, 5, 64, 4096):
        n = Lb.avc_critic_loss_ws(B)
        assert n >= 12 * B and n % 16 == 0, (B, n)


def test_wrappers_need_a_device():
    import torch

    from autoformer_amd import kernels as K
    from autoformer_amd.critic import critic_loss_block

    e, t, p = torch.randn(3, 8), torch.randn(3, 8), torch.rand(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        critic_loss_block(e, t, p, p, 0.1, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.critic_loss(e, t, p, p, 0.1, 1.0)


# ----------------------------------------------------------------------- the trainer
def test_critic_due_is_the_reference_condition():
    from autoformer_amd.train_gan import critic_due

    for n_critic in (1, 10):
        for pretrained_step in (0, 5, 10):
            for i in range(30):
                want = (i + 1) % n_critic == 0 and (i + 1) > pretrained_step   # train_with_gan_ver1.py:139
                assert critic_due(i, n_critic, pretrained_step) is want, (i, n_critic, pretrained_step)
    assert [i for i in range(30) if critic_due(i, 10, 10)] == [19, 29]
    assert [i for i in range(6) if critic_due(i, 2, 0)] == [1, 3, 5]


REFERENCE_CONFIG = dict(num_speaker=80, lambda_cd=1, lambda_ad=0.1, lambda_cls=0.1, lambda_dis=1, n_critic=10,
                        batch_size=2, len_crop=176, dim_neck=44, dim_emb=256, dim_pre=512, freq=22, log_step=10)


def test_config_and_parser_defaults_equal_the_reference():
    from autoformer_amd.train_gan import Config, build_parser, config_from_args

    c = Config("AutoVC", "d", False, 1000)
    assert {k: getattr(c, k) for k in REFERENCE_CONFIG} == REFERENCE_CONFIG
    assert c.pretrained_step == 100 and Config("AutoVC", "d", False, 15).pretrained_step == 1
    a = build_parser().parse_args(["--data_dir", "d", "--classifier_ckpt", "f"])
    assert (a.model_name, a.use_adain, int(a.num_iters), a.save_model_name) == ("AutoVC", False, 10, None)
    assert (a.n_critic, a.lambda_cls, a.lambda_dis, a.batch_size, a.len_crop, a.log_step) == (10, 0.1, 1, 2, 176, 10)
    assert (a.pretrained_step, a.dtype, a.synthetic, a.seed, a.det_init) == (None, "fp32", False, 1234, False)
    cfg = config_from_args(a)
    want = dict(REFERENCE_CONFIG, num_speaker=None)                            # the checkpoint's class count
    assert {k: getattr(cfg, k) for k in want} == want
    assert cfg.pretrained_step == 1 and cfg.classifier_ckpt == "f" and cfg.use_adain is False
    a = build_parser().parse_args(["--synthetic", "--det_init", "--num_iters", "40", "--pretrained_step", "0",
                                   "--n_critic", "2", "--use_adain", "1", "--num_speaker", "5"])
    cfg = config_from_args(a)
    assert (cfg.num_iters, cfg.pretrained_step, cfg.n_critic, cfg.use_adain, cfg.num_speaker) == (40, 0, 2, True, 5)


def test_cli_refusals():
    from autoformer_amd.train_gan import main

    with pytest.raises(SystemExit, match="--len_crop 160: the Discriminator is hard-wired to 176 frames"):
        main(["--synthetic", "--det_init", "--len_crop", "160"])
    with pytest.raises(SystemExit, match="--len_crop 100: MetaDV crops windows of 128 frames"):
        main(["--synthetic", "--det_init", "--len_crop", "100"])
    with pytest.raises(SystemExit, match="--classifier_ckpt is required"):
        main(["--synthetic"])
    with pytest.raises(SystemExit, match="--data_dir or --synthetic"):
        main(["--det_init"])
    with pytest.raises(SystemExit, match="the HIP kernels need a GPU"):
        main(["--synthetic", "--det_init", "--device", "cpu"])
