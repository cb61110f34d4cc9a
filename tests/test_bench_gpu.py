"""bench.py as a plain run: one JSON line with the headline fields and, with --dump-outputs, the arrays of the last timed
generation - the same in every run of the same arguments (the settling steps run on an engine of their own)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*more):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + list(more), cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_bench_dumps_the_same_outputs_in_every_run(tmp_path):
    K, W = 3, 2
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        line = _bench("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(d))
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == K and line["ms_per_step"] > 0 and line["settle_steps"] > 0
        assert line["value"] == pytest.approx(line["gens_per_sec"] * line["config"]["agent_steps_per_generation"], rel=1e-3)
        for k in ("cpu_baseline", "cpu_baseline_all_cores", "extra", "cold_gens_per_sec"):
            assert line.get(k) is None, k   # (--full only)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"game_rewards.npy", "fitness.npy", "elite_ids.npy", "sigma.npy", "hof_weights_agent_0.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert x.dtype in (np.float32, np.float64) and x.size and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    # the timed engine played exactly W + K generations, whatever the settling took
    assert np.load(dirs[0] / "eval_reward_history.npy").shape == (3, W + K)
    ids = np.load(dirs[0] / "elite_ids.npy")
    assert ids.shape == (3, 2) and ((ids >= 0) & (ids < 200)).all()
    assert np.load(dirs[0] / "game_rewards.npy").shape == (3 * 200 * 5, 3)
