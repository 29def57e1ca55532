"""GPU (-m gpu): bench.py as the driver starts it.  (a) `bench.py --gpus 2` started as ONE process re-executes itself under torch.distributed.run and
rank 0 prints one compact line with n_gpus 2 - two ranks on the one device of the box (--oversubscribe; RCCL refuses two ranks on one device, so the
process group is gloo and the exchange the peer-copy form, shc_peer_*: the engine, the sharding, the timed region and the line are the N > 1 path's).
(b) BASELINE.json configs[3] at its stated size on one device: bench.py --workload config4full (eight shards of 131 072 octopods, the 335.5 MB gathered
buffer).  (c) The plain run: the headline figure alone, and the outputs --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = r.stdout.strip().splitlines()[-1]
    assert len(line.encode()) < 4096
    return json.loads(line)


@pytest.mark.timeout(1200)
def test_gpus_2_spawns_two_ranks_and_prints_one_line():
    out = run_bench("--gpus", "2", "--oversubscribe", "--backend", "gloo", "--gather", "peer", "--workload", "config4", "--instances", "8192", "--steps", "10", "--warmup", "3",
                    "--no-cpu-baseline", "--full")
    assert out["n_gpus"] == 2 and out["steps"] == 10 and out["warmup"] == 3 and out["scaling"] == "weak"
    cfg = out["config"]
    assert cfg["instances_per_gpu"] == 8192 and cfg["legs"] == 8 and cfg["dof"] == 5
    assert out["value"] > 0 and cfg["scale_reference"]["value"] > 0 and cfg["gather_ms"] > 0 and cfg["value_without_gather"] >= out["value"] * 0.5
    assert 0 < cfg["weak_scaling_efficiency"]["without_gather"] and cfg["gather_bytes_per_rank"] == 8192 * 40 * 8
    assert out["parity"]["max_abs_dq"] is not None and out["parity"]["max_abs_dq"] <= 1e-6


@pytest.mark.timeout(1800)
def test_config4_at_its_stated_size_on_one_device():
    out = run_bench("--workload", "config4full", "--steps", "20", "--warmup", "5", "--full")
    cfg = out["config"]
    assert cfg["instances_per_gpu"] == 1 << 20 and cfg["legs"] == 8 and cfg["dof"] == 5
    assert out["value"] > 1e8 and cfg["gather_ms"] > 0
    assert out["parity"]["instances"] == 512 and out["parity"]["max_abs_dq"] <= 1e-6
    det = json.load(open(os.path.join(ROOT, "bench_details.json")))["config"]
    assert det["gathered_buffer_bytes"] == (1 << 20) * 40 * 8 and det["gathered_buffer_matches_getter"] and det["finite"] and det["moving_fraction"] == 1.0


@pytest.mark.timeout(1200)
def test_rccl_path_keeps_the_json_line_last():
    """One rank with the process group up (--force-dist: RCCL's all-gather in the timed region).  RCCL prints a version banner through C stdio, which a pipe
    holds back until the process exits; bench.py flushes it before its own line, so the driver's "last line of stdout" is the JSON."""
    out = run_bench("--gpus", "1", "--force-dist", "--workload", "config4", "--instances", "8192", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--full")
    assert out["n_gpus"] == 1 and out["config"]["gather_ms"] > 0 and out["config"]["gather_form"].startswith("RCCL")


@pytest.mark.timeout(600)
def test_plain_run_is_the_headline_alone_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline figure only (no roofline / parity / cpu_baseline / also), `--steps` timed steps, and
    --dump-outputs writes the joint state of the last timed step - the same bits in two processes with the same arguments."""
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = run_bench("--gpus", "1", "--steps", "300", "--warmup", "20", "--dump-outputs", str(d))
        assert out["steps"] == 300 and out["warmup"] == 20 and out["dtype"] == "f64" and out["higher_is_better"] is True
        assert out["value"] == pytest.approx(4096 / (out["ms_per_step"] * 1e-3), rel=1e-4)
        assert out["roofline"] is None and out["parity"] is None and "cpu_baseline" not in out and out["also"] == []
        outs.append({name: np.load(str(d / f"{name}.npy")) for name in ("q", "qd")})
    for name in ("q", "qd"):
        a, b = outs[0][name], outs[1][name]
        assert a.dtype == np.float64 and a.shape == (4096, 18) and np.isfinite(a).all()
        assert np.array_equal(a, b), name
