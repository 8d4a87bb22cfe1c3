"""bench.py's multi-GPU entry: --gpus N without a launcher starts N ranks
itself, and refuses (non-zero exit, clear message) when the node has fewer than N GPUs --
never a 1-GPU number labelled as N GPUs."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="node has >= 2 GPUs: the spawn would run the bench")
def test_bench_gpus2_refuses_without_two_gpus():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2 needs 2 visible GPUs" in r.stderr
    assert '"metric"' not in r.stdout


def test_bench_world_mismatch_is_an_error():
    """Launched by torchrun-like env with WORLD_SIZE=1 but --gpus 2: refuse."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "process group has 1 rank" in (r.stderr + r.stdout)


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs writes loss / loss_terms / mel_postnet and grad_norm (float32; grad_norm: whole, then
    per top-level module), and keeps to its byte bound by writing the leading utterances only."""
    import types

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    owner = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 2))
    grads = []
    for i, p in enumerate(owner.parameters()):
        p.grad = torch.full_like(p, float(i + 1))
        grads.append(p.grad.reshape(-1))
    tr = types.SimpleNamespace(gflat=torch.cat(grads), owner=owner)
    mel = torch.arange(4 * 1 * 8 * 80, dtype=torch.float32).reshape(4, 1, 8, 80)
    outs = types.SimpleNamespace(last=(None, (torch.tensor(0.5), torch.tensor(0.25), torch.tensor(2.0)), mel))
    bench.dump_outputs(str(tmp_path / "a"), torch.tensor(2.75), outs, tr)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["grad_norm", "loss", "loss_terms", "mel_postnet"]
    assert got["loss"].dtype == got["loss_terms"].dtype == got["mel_postnet"].dtype == np.float32
    assert got["loss"].tolist() == [2.75] and got["loss_terms"].tolist() == [0.5, 0.25, 2.0]
    assert np.array_equal(got["mel_postnet"], mel.numpy())
    assert got["grad_norm"].dtype == np.float32
    expect = [(6 * 1 + 2 * 4 + 4 * 9 + 2 * 16) ** 0.5, (6 * 1 + 2 * 4) ** 0.5, (4 * 9 + 2 * 16) ** 0.5]
    np.testing.assert_allclose(got["grad_norm"], expect, rtol=1e-6)
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 20) + 2 * 8 * 80 * 4)  # room for two utterances
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(2.75), outs, tr)
    assert np.array_equal(np.load(tmp_path / "b" / "mel_postnet.npy"), mel[:2].numpy())


def _bench(tmp_path, name, steps, warmup):
    import json

    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path / name)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    files = sorted(os.listdir(tmp_path / name))
    assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64 * 10**6
    return json.loads(lines[0]), {f[:-4]: np.load(tmp_path / name / f) for f in files}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("bench"), "first", 2, 1)


@pytest.mark.gpu
def test_bench_plain_run_is_lean(plain_run):
    """A plain run prints the headline fields only (roofline / cpu_baseline are behind --full) and times
    exactly --steps steps."""
    out, _ = plain_run
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["unit"] == "mel-frames/s"
    assert out["value"] == pytest.approx(64 * 128 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert out["higher_is_better"] is True and out["dtype"] == "bf16" and "metric" in out
    assert "roofline" not in out and "cpu_baseline" not in out


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_run_to_run(plain_run, tmp_path):
    """Two runs write the same outputs, whatever --steps and --warmup: loss, loss terms and mel_postnet
    bit for bit (same inputs, same initial state, bit-reproducible forward).  The gradient passes
    through bf16 tensors behind float-atomic sums, so single elements may move by a bf16 ulp between
    runs: its norms agree to within one bf16 ulp, 2^-8 relative."""
    import numpy as np

    _, a = plain_run
    _, b = _bench(tmp_path, "second", 1, 0)
    assert sorted(a) == sorted(b) == ["grad_norm", "loss", "loss_terms", "mel_postnet"]
    assert a["mel_postnet"].shape == (64, 1, 128, 80) and a["mel_postnet"].dtype == np.float32
    assert a["loss"].dtype == a["loss_terms"].dtype == a["grad_norm"].dtype == np.float32
    for k in ("loss", "loss_terms", "mel_postnet"):
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert float(a["loss"][0]) == pytest.approx(float(a["loss_terms"].sum()), rel=1e-6)
    assert a["grad_norm"].shape == (4,) and (a["grad_norm"] > 0).all()  # whole, encoder, decoder, postnet
    np.testing.assert_allclose(a["grad_norm"], b["grad_norm"], rtol=2.0 ** -8)
