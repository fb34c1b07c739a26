"""Timing of the device path of ``sq.gr.mask_graph`` (csrc/sqgr_mask.hip) and, scaled from a sample, of its numpy path.

    python tools/mask_graph_time.py [--out profiles/mask_graph_time.json] [--rows 1000 --cols 1000] [--repeats 5] [--host-edges 60000]

Input: a rows x cols hex lattice (1e6 spots by default) with its directed kNN-6 graph (6e6 edges), against a star-shaped outline of
2 048 vertices with one hole of 64.  Recorded:

- ``segments_within(device=None)``, the whole call (validation and flattening on the host, upload, every kernel, the copies back; wall
  clock around a synchronous call), ``--repeats`` times after a warm-up call of the same shape: every time and the median;
- the HIP-event time of each kernel from the context's timers, in one further call with the timers on;
- ``mask_graph(copy=True, device=None)``, the whole call with the CSR filter;
- the stats of the call and the constants of ``sqgr_mask_info``; the build stamp of the library;
- the numpy path on ``--host-edges`` of the same edges (every k-th, ``chunk=8192``: the default chunk needs a dozen temporaries of
  1 GiB at this polygon), one run on one core, and that time SCALED by E / host-edges to the whole graph.  The scaled number is an
  extrapolation, not a measurement of the whole graph: the numpy path is linear in the edges.

The device and host answers are compared on the sample before anything is written."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def outline(cx: float, cy: float, radius: float):
    from squidpy_amd.gr._mask import Polygon

    t = 2 * np.pi * np.arange(2048) / 2048
    r = radius * (1.0 + 0.3 * np.sin(9 * t))
    h = 2 * np.pi * np.arange(64) / 64
    return Polygon(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1),
                   holes=[np.stack([cx + 0.15 * radius * np.cos(h), cy + 0.15 * radius * np.sin(h)], axis=1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-edges", type=int, default=60000)
    a = ap.parse_args()

    import pandas as pd

    import squidpy_amd as sq
    from squidpy_amd import _build, _lib, _synthetic
    from squidpy_amd.gr._mask import segments_within

    ctx = _lib.default_context()
    xy = _synthetic.hex_grid(a.rows, a.cols)
    conn = _synthetic.knn_directed_graph(xy, 6, ctx)
    conn = conn.astype(np.float64)
    rows = np.repeat(np.arange(conn.shape[0]), np.diff(conn.indptr))
    pa, pb = xy[rows], xy[conn.indices]
    e = len(pa)
    mask = outline(float(xy[:, 0].mean()), float(xy[:, 1].mean()), 0.3 * float(np.ptp(xy[:, 0])))
    n_ring_edges = 2048 + 64

    segments_within(pa, pb, mask, device=None)  # warm-up: the same shape, loads the code objects and sizes the allocator's pool
    ctx.sync()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        within, stats = segments_within(pa, pb, mask, device=None, return_stats=True)
        times.append(time.perf_counter() - t0)
    ctx.timer_enable(True)
    ctx.timer_reset()
    segments_within(pa, pb, mask, device=None)
    kernels = {name: v for name, v in ctx.timer_report().items() if name.startswith("mask_")}
    ctx.timer_enable(False)

    adata = sq.AnnDataLite(X=None, obs=pd.DataFrame(index=np.arange(len(xy)).astype(str)), obsm={"spatial": xy},
                           obsp={"spatial_connectivities": conn, "spatial_distances": conn})
    t0 = time.perf_counter()
    adj, _ = sq.gr.mask_graph(adata, None, mask, copy=True, device=None)
    mask_graph_s = time.perf_counter() - t0
    assert adj.nnz == int(within.sum())

    step = max(1, e // a.host_edges)
    sample = np.arange(0, e, step)[: a.host_edges]
    t0 = time.perf_counter()
    host = segments_within(pa[sample], pb[sample], mask, chunk=8192)
    host_s = time.perf_counter() - t0
    assert np.array_equal(host, within[sample]), "the device and the host disagree on the sample"

    out = {
        "device": ctx.device_info(), "build_stamp": _build.source_fingerprint(), "mask_info": _lib.mask_info(),
        "spots": int(len(xy)), "edges": int(e), "ring_edges": n_ring_edges, "pairs": int(e) * n_ring_edges,
        "within": int(within.sum()), "stats": stats,
        "segments_within_device_s": times, "segments_within_device_median_s": float(np.median(times)),
        "kernels_launches_ms": kernels, "kernels_total_ms": sum(v[1] for v in kernels.values()),
        "mask_graph_device_s": mask_graph_s,
        "host_sample_edges": int(len(sample)), "host_sample_chunk": 8192, "host_sample_s": host_s, "host_threads": 1,
        "host_scaled_to_all_edges_s": host_s * e / len(sample),
        "host_scaled_note": "scaled linearly from the sample; the whole graph was not run on the host",
    }
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
