"""spatial_neighbors front ends on 3-D coordinates at 1e6 points: wall time and kernel time per call, next to sklearn's
KD-tree on one core and to the 2-D search at 1e6 hex spots from the same run (run on the GPU box).

    python tools/neighbors3d_time.py [--out profiles/neighbors3d_time.json] [--reps 3] [--z-step 100] [--skip-cpu]

Inputs: a 100 x 100 x 100 cubic lattice of pitch 100, and 10 stacked hex sections (250 x 400 spots of pitch 100 each),
``--z-step`` apart.  Calls: ``spatial_neighbors_knn(n_neighs=6)``, ``spatial_neighbors_radius(radius=150)``,
``spatial_neighbors_grid(n_neighs=6)``.  Kernel time is the sum of the library's HIP-event timers (``LaunchTimer``) over the
call; wall time is the whole front end (cell list on the host, copies, CSR assembly with scipy)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import squidpy_amd as sq  # noqa: E402
from squidpy_amd._lib import default_context  # noqa: E402
from squidpy_amd._synthetic import hex_grid  # noqa: E402


def timed(ctx, fn, reps):
    """min wall seconds over `reps` calls after one warm-up; kernel milliseconds by timer name of the fastest call"""
    fn()
    best = None
    for _ in range(reps):
        ctx.timer_enable(True)
        ctx.timer_reset()
        try:
            t = time.perf_counter()
            res = fn()
            wall = time.perf_counter() - t
            rep = ctx.timer_report()
        finally:
            ctx.timer_enable(False)
        kern = {name: round(ms, 4) for name, (cnt, ms) in rep.items() if cnt > 0 and name.startswith("neighbors")}
        if best is None or wall < best["wall_s"]:
            best = {"wall_s": round(wall, 4), "kernel_ms": round(sum(kern.values()), 4), "kernels_ms": kern, "nnz": int(res.connectivities.nnz)}
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors3d_time.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--z-step", type=float, default=100.0)
    ap.add_argument("--skip-cpu", action="store_true")
    a = ap.parse_args()
    ctx = default_context()
    side = np.arange(100.0) * 100.0
    section = hex_grid(250, 400)
    inputs = {
        "cubic_lattice_100x100x100": np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3),
        "hex_sections_10x100000": np.concatenate([np.column_stack([section, np.full(len(section), a.z_step * s)]) for s in range(10)]),
        "hex_2d_1000x1000": hex_grid(1000, 1000),  # the 2-D search on the same number of points, for comparison
    }
    out = {"z_step": a.z_step, "reps": a.reps, "inputs": {}}
    for name, coords in inputs.items():
        adata = sq.AnnDataLite(obs=pd.DataFrame(index=[str(i) for i in range(len(coords))]), obsm={"spatial": coords})
        calls = {"knn k=6": lambda: sq.gr.spatial_neighbors_knn(adata, n_neighs=6, copy=True)}
        if coords.shape[1] == 3:
            calls["radius 150"] = lambda: sq.gr.spatial_neighbors_radius(adata, radius=150.0, copy=True)
            calls["grid n_neighs=6"] = lambda: sq.gr.spatial_neighbors_grid(adata, n_neighs=6, copy=True)
        row = {"n": int(len(coords)), "width": int(coords.shape[1]), "calls": {}}
        for label, fn in calls.items():
            row["calls"][label] = timed(ctx, fn, a.reps)
            print(f"{name:28s} {label:16s} {json.dumps(row['calls'][label])}", flush=True)
        if not a.skip_cpu and coords.shape[1] == 3:
            from sklearn.neighbors import NearestNeighbors

            t = time.perf_counter()
            NearestNeighbors(n_neighbors=6).fit(coords).kneighbors()
            row["sklearn_kneighbors_k6_one_core_s"] = round(time.perf_counter() - t, 3)
            print(f"{name:28s} sklearn kneighbors k=6, one core: {row['sklearn_kneighbors_k6_one_core_s']} s", flush=True)
        out["inputs"][name] = row
    base = out["inputs"]["hex_2d_1000x1000"]["calls"]["knn k=6"]["kernel_ms"]
    for name, row in out["inputs"].items():
        if row["width"] == 3 and base:
            row["knn_kernel_vs_2d"] = round(row["calls"]["knn k=6"]["kernel_ms"] / base, 3)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
