"""Timing of ``sq.gr.niche_leiden`` (csrc/sqgr_leiden.hip) on the device and of networkx's Louvain on the host.

    python tools/niche_leiden_time.py [--out profiles/niche_leiden_time.json] [--legs gpu_1e5,gpu_1e6,networkx_1e4,networkx_1e5]

The driver runs every leg as a process of its own under ``timeout -k 10 <seconds>`` sized to that leg, chained with ``&&`` (a leg that
fails or runs out of time ends the run; nothing starts on the device after it), and merges what the legs wrote.

- ``gpu_1e5`` / ``gpu_1e6``: rows x 30 columns drawn from 20 overlapping Gaussian blobs, ``niche_neighbors(n_neighbors=15)`` (not timed
  here: tools/niche_neighbors_time.py), then ``niche_leiden(graph, 1.0)``: the whole call (quantisation and symmetry check on the host,
  upload, every iteration, the canonical relabelling; wall clock), the HIP-event time of each kernel, sweeps, levels, iterations, the
  number of communities and Q.
- ``networkx_1e4`` / ``networkx_1e5``: ``networkx.community.louvain_communities(resolution=1, seed=0)`` on the quantised kNN-15 fuzzy
  graph of the same kind of cloud, built on the host (scipy's KD-tree and the numpy restatement of the fuzzy weights), one core, and its
  Q by the same helper.  No device."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_NEIGHBORS, COLUMNS, RESOLUTION = 15, 30, 1.0
LEG_SECONDS = {"gpu_1e5": 240, "gpu_1e6": 560, "networkx_1e4": 600, "networkx_1e5": 3000}


def cloud(n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + COLUMNS)
    centres = rng.normal(size=(20, COLUMNS)) * 1.5
    return centres[rng.integers(0, 20, size=n)] + rng.normal(size=(n, COLUMNS))


def leg_gpu(n: int) -> dict:
    import squidpy_amd as sq
    from squidpy_amd._lib import default_context

    ctx = default_context()
    sq.gr.niche_leiden(sq.gr.niche_neighbors(cloud(3000), N_NEIGHBORS), RESOLUTION)  # loads the code objects
    graph = sq.gr.niche_neighbors(cloud(n), N_NEIGHBORS)
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    res = sq.gr.niche_leiden(graph, RESOLUTION)
    wall = time.perf_counter() - t0
    rep = {name: v for name, v in ctx.timer_report().items() if name.startswith("leiden")}
    ctx.timer_enable(False)
    t0 = time.perf_counter()
    sq.gr.quantise_weights(graph.connectivities)
    host = time.perf_counter() - t0
    out = {"device": ctx.device_info(), "rows": n, "columns": COLUMNS, "n_neighbors": N_NEIGHBORS, "resolution": RESOLUTION,
           "connectivities_nnz": int(graph.connectivities.nnz), "whole_call_s": wall, "host_quantisation_s": host,
           "kernels_launches_ms": rep, "kernels_total_ms": sum(v[1] for v in rep.values()), "sweeps": res.sweeps, "levels": res.levels,
           "iterations": res.iterations, "n_communities": res.n_communities, "quality": res.quality}
    print(f"gpu n={n}", json.dumps(out), flush=True)
    return out


def leg_networkx(n: int) -> dict:
    import networkx as nx
    from scipy import sparse
    from scipy.spatial import cKDTree

    import squidpy_amd as sq
    from tests import niche_leiden_oracle as LO
    from tests import niche_neighbors_oracle as NO

    x = cloud(n)
    dist, idx = cKDTree(x).query(x, k=N_NEIGHBORS)
    dist, idx = dist[:, 1:], idx[:, 1:].astype(np.int32)
    conn = NO.connectivities(idx, NO.fuzzy(dist, float(dist.sum() / (n * N_NEIGHBORS))).vals).tocsr()
    conn.setdiag(0)
    conn.eliminate_zeros()
    q = sq.gr.quantise_weights(conn)
    g = nx.from_scipy_sparse_array(sparse.csr_matrix((q.data.astype(np.int64), q.indices, q.indptr), shape=q.shape))
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(g, weight="weight", resolution=RESOLUTION, seed=0)
    wall = time.perf_counter() - t0
    labels = np.empty(n, dtype=np.int64)
    for c, members in enumerate(parts):
        labels[list(members)] = c
    out = {"rows": n, "columns": COLUMNS, "n_neighbors": N_NEIGHBORS, "resolution": RESOLUTION, "connectivities_nnz": int(q.nnz), "threads": 1,
           "louvain_s": wall, "n_communities": len(parts), "quality": LO.quality(q.indptr, q.indices, q.data, labels, RESOLUTION)}
    print(f"networkx n={n}", json.dumps(out), flush=True)
    return out


def run_leg(name: str) -> dict:
    kind, size = name.split("_")
    n = int(float(size))
    return leg_gpu(n) if kind == "gpu" else leg_networkx(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=",".join(LEG_SECONDS))
    ap.add_argument("--leg", default=None, help="(internal) run one leg and write its part")
    ap.add_argument("--part", default=None)
    a = ap.parse_args()
    if a.leg:
        part = run_leg(a.leg)
        with open(a.part, "w") as fh:
            json.dump(part, fh)
        return
    legs = [s for s in a.legs.split(",") if s]
    with tempfile.TemporaryDirectory() as tmp:
        steps = [f"timeout -k 10 {LEG_SECONDS[leg]} {sys.executable} {os.path.abspath(__file__)} --leg {leg} --part {tmp}/{leg}.json" for leg in legs]
        rc = subprocess.run(" && ".join(steps), shell=True, cwd=ROOT).returncode
        report = {"exit_status": rc, "legs": {}}
        for leg in legs:
            if os.path.exists(f"{tmp}/{leg}.json"):
                with open(f"{tmp}/{leg}.json") as fh:
                    report["legs"][leg] = json.load(fh)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    sys.exit(rc)


if __name__ == "__main__":
    main()
