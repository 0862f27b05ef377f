"""A plain `bench.py` run (no --full): exactly --steps timed steps, once, and with --dump-outputs the top-k of the last timed
step on disk — the same files from two runs with the same arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tools.bench_line import parse_emitted

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_times_the_steps_once_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    got = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "200000", "--steps", "6", "--warmup", "2",
               "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=270, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        line, side = parse_emitted(r.stdout)
        assert line["steps"] == 6 and line["config"]["repeats"] == 1 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(64 * 1e3 / line["ms_per_step"], rel=1e-4)
        assert "extra" not in side and line["cpu_baseline"] is None and line["roofline"]["achieved"] is None
        ids, sc = np.load(tmp_path / run / "topk_ids.npy"), np.load(tmp_path / run / "topk_scores.npy")
        assert ids.dtype == np.float64 and sc.dtype == np.float32 and ids.shape == sc.shape == (64, 20)
        assert np.all(ids == np.round(ids)) and ids.min() >= 0 and ids.max() < 200000
        assert all(len(set(row.tolist())) == 20 for row in ids) and np.all(np.diff(sc, axis=1) <= 0)
        got.append((ids, sc))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
