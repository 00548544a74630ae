"""bench.py's launch contract, checked without a GPU: under torchrun, a WORLD_SIZE that differs
from --gpus is refused before anything touches the GPU (it used to warn and time one
rank), and the self-launch command is a fresh torch.distributed.run child."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert "WORLD_SIZE=1" in r.stderr
    assert r.stdout.strip() == ""


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    import pytest

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and (args.steps, args.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_files_are_exact(tmp_path):
    """--dump-outputs writes float64 files; the hi32 / lo32 halves restore every u64 bit."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench

    g = np.array([0, 1, 2**53 + 1, 2**64 - 1, 0x0123456789ABCDEF], dtype=np.uint64)
    p = np.arange(10, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    outs = [torch.from_numpy(a.view(np.int64).copy()) for a in (g, p)]
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), [("gcounter", None, 0), ("pncounter", None, 0)], outs)
    assert sorted(os.listdir(d)) == sorted(f"{k}{s}.npy" for k in ("gcounter", "pncounter")
                                           for s in ("", "_hi32", "_lo32"))
    for kind, a in (("gcounter", g), ("pncounter", p)):
        v, hi, lo = (np.load(d / f"{kind}{s}.npy") for s in ("", "_hi32", "_lo32"))
        assert v.dtype == hi.dtype == lo.dtype == np.float64 and v.shape == a.shape
        assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), a)
        assert np.array_equal(v, a.astype(np.float64))


def test_self_launch_command(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    class R:
        returncode = 0

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    args = bench.parse()
    assert bench.self_launch(args) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-3:] == ["--gpus", "4", "--steps", "3"][-3:]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    json.dumps(cmd)
