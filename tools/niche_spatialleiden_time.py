"""Timing of ``sq.gr.niche_spatialleiden`` (csrc/sqgr_leiden_multiplex.hip) on the device, with ``sq.gr.niche_leiden`` on the latent
layer alone in the same run as the yardstick.  There is no CPU baseline: spatialleiden and leidenalg are not installed.

    python tools/niche_spatialleiden_time.py [--out profiles/niche_spatialleiden_time.json] [--rows 100000]

The driver runs the measurement as a process of its own under ``timeout -k 10 <seconds>`` (a run that fails or runs out of time ends
there) and writes what it returned.

- Latent layer: ``rows`` x 30 columns drawn from 20 overlapping Gaussian blobs, ``niche_neighbors(n_neighbors=15)`` (the fuzzy kNN-15
  graph; not timed here).  Spatial layer: the 6-neighbour hexagonal lattice of unit weights on a near-square grid with that many cells.
  ``resolution = (1, 1)``, ``layer_ratio = 1``.
- Recorded for both calls: the whole call (quantisation on the host, upload, every iteration, the canonical relabelling; wall clock),
  the host quantisation alone, the HIP-event time of each kernel by phase, sweeps, levels, iterations and the number of communities;
  and the ratio of the two whole calls."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_NEIGHBORS, COLUMNS, RESOLUTION, LAYER_RATIO = 15, 30, 1.0, 1.0
SECONDS = 560


def cloud(n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + COLUMNS)
    centres = rng.normal(size=(20, COLUMNS)) * 1.5
    return centres[rng.integers(0, 20, size=n)] + rng.normal(size=(n, COLUMNS))


def hex_lattice(n: int):
    """The 6-neighbour lattice on the first ``n`` cells of a near-square grid in row-major order (odd rows shifted right by half a cell)."""
    from scipy import sparse

    side = int(np.ceil(np.sqrt(n)))
    row, col = np.divmod(np.arange(n), side)
    r, c = [], []
    for dr, dc_even, dc_odd in ((0, 1, 1), (1, 0, 1), (1, -1, 0)):  # right, down-right, down-left; the transpose adds the other three
        rr = row + dr
        cc = col + np.where(row % 2 == 0, dc_even, dc_odd)
        ok = (cc >= 0) & (cc < side) & (rr * side + cc < n)
        r.append(np.arange(n)[ok])
        c.append((rr * side + cc)[ok])
    r, c = np.concatenate(r), np.concatenate(c)
    a = sparse.coo_matrix((np.ones(2 * r.shape[0]), (np.r_[r, c], np.r_[c, r])), shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def timed(ctx, prefix: str, call) -> tuple:
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    res = call()
    wall = time.perf_counter() - t0
    rep = {name: v for name, v in ctx.timer_report().items() if name.startswith(prefix)}
    ctx.timer_enable(False)
    return res, wall, rep


def measure(n: int) -> dict:
    import squidpy_amd as sq
    from squidpy_amd._lib import default_context

    ctx = default_context()
    warm = sq.gr.niche_neighbors(cloud(3000), N_NEIGHBORS).connectivities  # loads the code objects
    sq.gr.niche_leiden(warm, RESOLUTION)
    sq.gr.niche_spatialleiden((warm, hex_lattice(3000)), RESOLUTION, layer_ratio=LAYER_RATIO)
    latent = sq.gr.niche_neighbors(cloud(n), N_NEIGHBORS).connectivities
    spatial = hex_lattice(n)
    multi, multi_wall, multi_rep = timed(ctx, "mleiden", lambda: sq.gr.niche_spatialleiden((latent, spatial), RESOLUTION, layer_ratio=LAYER_RATIO))
    single, single_wall, single_rep = timed(ctx, "leiden", lambda: sq.gr.niche_leiden(latent, RESOLUTION))
    t0 = time.perf_counter()
    sq.gr.quantise_layers(latent, spatial)
    host_multi = time.perf_counter() - t0
    t0 = time.perf_counter()
    sq.gr.quantise_weights(latent)
    host_single = time.perf_counter() - t0

    def part(res, wall, host, rep) -> dict:
        return {"whole_call_s": wall, "host_quantisation_s": host, "kernels_launches_ms": rep, "kernels_total_ms": sum(v[1] for v in rep.values()),
                "sweeps": res.sweeps, "levels": res.levels, "iterations": res.iterations, "n_communities": res.n_communities, "quality": res.quality}

    out = {"device": ctx.device_info(), "rows": n, "columns": COLUMNS, "n_neighbors": N_NEIGHBORS, "resolution": [RESOLUTION, RESOLUTION],
           "layer_ratio": LAYER_RATIO, "latent_nnz": int(latent.nnz), "spatial_nnz": int(spatial.nnz),
           "niche_spatialleiden": part(multi, multi_wall, host_multi, multi_rep), "niche_leiden_latent_only": part(single, single_wall, host_single, single_rep),
           "whole_call_ratio": multi_wall / single_wall, "cpu_baseline": "none: spatialleiden and leidenalg are not installed"}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--part", default=None, help="(internal) run the measurement and write it here")
    a = ap.parse_args()
    if a.part:
        with open(a.part, "w") as fh:
            json.dump(measure(a.rows), fh)
        return
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        part = os.path.join(tmp, "part.json")
        rc = subprocess.run(["timeout", "-k", "10", str(SECONDS), sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--part", part],
                            cwd=ROOT).returncode
        report = {"exit_status": rc}
        if os.path.exists(part):
            with open(part) as fh:
                report.update(json.load(fh))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")
    sys.exit(rc)


if __name__ == "__main__":
    main()
