"""bench.py's multi-rank path on the CPU: `bench.py --gpus 2` (no torch.distributed.run
environment) launches the two ranks itself; with the stub workload (CPU oracle, gloo,
codewords keyed by global index exactly like the GPU workloads' Philox streams, offsets
from mc.rank_offset) the summed counters of the two ranks must equal one process over
[0, 2B) -- the sharding contract of SURVEY.md section 8(e)."""
import json
import os
import subprocess
import sys

import pytest

from polarcub_amd import mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2])
def test_launcher_counters_equal_single_process(world):
    B = 48
    multi = _bench("--gpus", str(world), "--workload", "stub", "--batch", str(B), "--steps", "2", "--warmup", "1")
    single = _bench("--gpus", "1", "--workload", "stub", "--batch", str(world * B), "--steps", "1", "--warmup", "0")
    assert multi["n_gpus"] == world and single["n_gpus"] == 1
    assert multi["codewords_per_step"] == single["codewords_per_step"] == world * B
    assert multi["frame_errors"] == single["frame_errors"]
    assert multi["bit_errors"] == single["bit_errors"]
    assert multi["frame_errors"] > 0  # the comparison is not vacuous
    assert [p["codewords"] for p in multi["per_rank"]] == [B] * world
    assert multi["value"] > 0 and all(p["value"] > 0 for p in multi["per_rank"])


def test_dump_outputs_repeat_and_steps_are_honoured(tmp_path):
    """--dump-outputs writes the last timed step's decisions as float .npy files, the same from run
    to run with the same arguments (whatever --steps, --warmup and --full are); --steps sets the
    timed steps, and the line carries ms_per_step; a plain run has none of --full's legs."""
    import numpy as np
    B = 40
    common = ["--gpus", "1", "--workload", "stub", "--batch", str(B)]
    one = _bench(*common, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    two = _bench(*common, "--steps", "1", "--warmup", "0", "--full", "--dump-outputs", str(tmp_path / "b"))
    assert one["steps"] == 3 and two["steps"] == 1
    for rec in (one, two):
        assert rec["ms_per_step"] > 0
        assert abs(rec["value"] - rec["codewords_per_step"] / (rec["ms_per_step"] / 1e3)) <= 1e-6 * rec["value"]
    assert "cpu_baseline" not in one and "mc_end_to_end" not in one
    a, b = np.load(tmp_path / "a" / "info.npy"), np.load(tmp_path / "b" / "info.npy")
    assert a.dtype in (np.float32, np.float64) and a.shape == (B, 32)
    assert np.array_equal(a, b) and set(np.unique(a)) <= {0.0, 1.0}
    assert int((a.sum(axis=1) > 0).sum()) > 0  # decisions, not an empty buffer
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["info.npy"]


def test_rank_offsets_tile_the_global_batch():
    B = 1 << 20
    offs = [mc.rank_offset(r, B) for r in range(8)]
    assert offs == [r * B for r in range(8)]
    assert mc.gather_floats([1.0, 2.0]) == [[1.0, 2.0]]
