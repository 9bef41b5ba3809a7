"""GPU: a plain `bench.py --gpus 1` run - the contract fields, --steps timed steps, none of the --full legs - and
--dump-outputs: the tables of the last timed step, in float32, equal the CPU oracle on sampled rows."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_last_one(built, tmp_path):
    from oracle import oracle

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SLAM_RDZV", "SLAM_BENCH_SINGLE_DEVICE", "SLAM_BENCH_COLLECTIVE"):
        env.pop(k, None)
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "pairs/s" and rec["higher_is_better"] is True
    assert abs(rec["value"] - 65536.0 * 65536 / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["parity_spot_check"] is None
    assert not any(k in rec for k in ("cpu_baseline", "pipelined", "reproj", "next_rows"))

    assert sorted(os.listdir(dump)) == ["distance.npy", "train_idx.npy"]
    idx, dist = np.load(dump / "train_idx.npy"), np.load(dump / "distance.npy")
    assert idx.dtype == dist.dtype == np.float32 and idx.shape == dist.shape == (65536, 2)
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    query, train = b.make_descriptors(b.N_QUERY, 228), b.make_descriptors(b.N_TRAIN, 229)
    sel = np.random.default_rng(7).choice(b.N_QUERY, 512, replace=False)
    ridx, rdist = oracle.bf_knn_c(query[sel], train, 2, threads=8)
    assert np.array_equal(idx[sel], ridx) and np.array_equal(dist[sel], rdist)
