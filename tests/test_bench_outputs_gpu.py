"""`bench.py --dump-outputs DIR` writes what the LAST timed step returned, and a plain run is the headline alone.

The inputs depend only on the arguments, so two runs whose last timed step covers the same global permutation range
(warm-up 1 + 2 timed steps, warm-up 2 + 1 timed step) must dump the same arrays, bit for bit."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--rows", "120", "--cols", "150", "--perms-per-step", "640"]
NAMES = ("moments_s1", "moments_s2", "zscore", "counts")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in NAMES}


def test_dump_outputs_is_the_last_timed_step_and_a_plain_run_is_the_headline(tmp_path):
    a = _bench(*SMALL, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*SMALL, "--steps", "1", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == 2 and b["steps"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    for line in (a, b):  # a plain run: no leg, baseline, projection or detail file
        assert not {"legs", "secondary", "cpu_baseline", "emulated_ranks", "geary_c"} & set(line) and line["detail"] is None
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    for name in NAMES:
        assert da[name].dtype == np.float64 and da[name].shape == (30, 30), name
        np.testing.assert_array_equal(da[name], db[name], err_msg=name)
    assert np.isfinite(da["zscore"]).all()
    from oracle import restate as O
    from squidpy_amd._synthetic import hex_grid_graph

    adj = hex_grid_graph(120, 150)  # bench.py's inputs: the hex grid and uniform labels of default_rng(0)
    labels = np.random.default_rng(0).integers(0, 30, adj.shape[0])
    np.testing.assert_array_equal(da["counts"], O.nhood_counts(adj.indices, adj.indptr, labels, 30))
