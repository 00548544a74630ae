"""bench.py --gpus 2 on the one-GPU box (VERDICT r2 "Done" criterion): started WITHOUT a torchrun
environment, the script launches its own 2-rank torch.distributed.run child (gloo: both ranks on
GPU 0), and rank 0 prints one JSON line with n_gpus 2 and (--full) the parity results and a config-5
block.  With --exchange
cabi-ops the step's exchange is the C ABI's own sharded code (crdt_lub_many_multi_sharded,
crdt_vclock_lub_many_sharded) over crdt_ctx_comm_init_ops host callbacks; with --exchange cabi the
RCCL communicator cannot form on one GPU, and every rank falls back to the torch exchange together."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_only_the_headline_and_dumps_its_result(tmp_path):
    """A plain run carries the headline figure alone (no c5 / c3 / c4 block, no CPU baseline, no
    parity verdict) with exactly --steps timed steps, and --dump-outputs writes the step's lubs:
    the elementwise u64 max over every row of the seeded synthetic input, restated on the CPU."""
    import numpy as np

    import bench
    import oracle as O

    R = 4099  # odd: the last block of the stream kernel is partial
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--replicas", str(R), "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["full"] is False and out["steps"] == 3 and out["n_gpus"] == 1
    assert not any(k in out for k in ("c5", "c3", "c4")) and out["cpu_baseline"] is None
    assert out["parity"].startswith("unchecked")
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(2 * R / (out["ms_per_step"] * 1e-3))
    for kind, seed, width in (("gcounter", bench.SEED_G, bench.A_ACTORS), ("pncounter", bench.SEED_P, 2 * bench.A_ACTORS)):
        exp = O.synth_matrix(seed, R, width, 0).max(axis=0)
        hi, lo = (np.load(tmp_path / "dump" / f"{kind}_{h}32.npy") for h in ("hi", "lo"))
        assert hi.dtype == lo.dtype == np.float64
        assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), exp)
        assert np.array_equal(np.load(tmp_path / "dump" / f"{kind}.npy"), exp.astype(np.float64))


@pytest.mark.parametrize("exchange", ["torch", "cabi-ops", "cabi"])
def test_bench_self_launches_two_ranks(exchange):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--exchange",
           exchange, "--replicas", "65536", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["parity"] == "ok"
    assert out["config"]["replica_merges_per_step"] == 2 * 2 * 65536
    assert out["c5"]["parity"] == "ok" and out["c5"]["config"]["replica_merges_per_step"] == 2 * 65536
    assert out["step_ms"]["min"] <= out["step_ms"]["median"] <= out["step_ms"]["max"]
    if exchange == "cabi-ops":
        assert "crdt_ctx_comm_init_ops" in out["config"]["exchange"]
    if exchange == "cabi":  # RCCL refuses two ranks on one GPU: every rank takes the torch exchange together
        assert "torch" in out["config"]["exchange"]
