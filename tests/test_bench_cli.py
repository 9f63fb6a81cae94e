"""bench.py's command line beside the launch decision: --full (everything but the headline is behind it) and
--dump-outputs (the last timed step's loss / parameters / gradients as float32 .npy files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

BENCH = os.path.join(ROOT, "bench.py")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_zero_steps_is_refused(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import torch
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.PReLU(), torch.nn.Linear(4, 1)).to(torch.float64)
    loss = model(torch.ones(2, 3, dtype=torch.float64)).sum()
    loss.backward()
    model[2].bias.grad = None            # a parameter the step gave no gradient: no grad file
    rec = bench.dump_outputs(str(tmp_path / "out"), loss, model)
    names = sorted(os.listdir(tmp_path / "out"))
    want = ["loss.npy"] + [f"param.{n}.npy" for n, _ in model.named_parameters()] + \
           [f"grad.{n}.npy" for n, p in model.named_parameters() if p.grad is not None]
    assert names == sorted(want) and "grad.2.bias.npy" not in names
    assert rec["files"] == len(names)
    total = 0
    for n, p in model.named_parameters():
        a = np.load(tmp_path / "out" / f"param.{n}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(p.shape)
        assert np.array_equal(a, p.detach().to(torch.float32).numpy())
        total += a.nbytes
    g = np.load(tmp_path / "out" / "grad.0.weight.npy")
    assert g.dtype == np.float32 and np.array_equal(g, model[0].weight.grad.to(torch.float32).numpy())
    l = np.load(tmp_path / "out" / "loss.npy")
    assert l.dtype == np.float32 and l.shape == (1,) and l[0] == np.float32(float(loss.detach()))
    assert total < rec["bytes"] <= bench.DUMP_LIMIT_BYTES


def test_dump_outputs_refuses_to_pass_the_limit(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64)
    model = torch.nn.Linear(8, 8)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), torch.zeros(()), model)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_them(tmp_path):
    """One plain run at cfg1 (1k nodes): the line carries the headline fields and nothing of --full, --steps is the
    number of timed steps, and the dump holds float32 arrays for the loss and every parameter."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "cfg1",
                          "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "edges/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["conv_edges"] / (line["ms_per_step"] / 1e3)) <= 1e-3 * line["value"]
    for k in ("roofline", "gemm", "gemm_dw", "gemm_dx", "csr_build", "extras", "cpu_baseline"):
        assert line[k] is None, k
    files = sorted(os.listdir(tmp_path / "dump"))
    assert line["dumped_outputs"]["files"] == len(files) and "loss.npy" in files
    assert any(f.startswith("param.") for f in files) and any(f.startswith("grad.") for f in files)
    for f in files:
        a = np.load(tmp_path / "dump" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert np.load(tmp_path / "dump" / "loss.npy")[0] == np.float32(line["final_loss"])
