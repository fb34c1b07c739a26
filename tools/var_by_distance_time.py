"""Timing of ``sq.tl.var_by_distance`` (csrc/sqgr_anchor.hip) and of the reference's sklearn search on the same anchors.

    python tools/var_by_distance_time.py [--out profiles/var_by_distance_time.json] [--rows 1000 --cols 1000] [--repeats 5] [--host-anchors 3]

Input: a rows x cols hex lattice (1e6 spots by default) with 30 uniform labels, all 30 as anchors, as 1 slide and as 8 slides
(vertical strips); and the same lattice with one label confined to the corner 1 % of the area as the only anchor (every other spot
is a query outside its bounding box).  Recorded, per input:

- ``var_by_distance(copy=True)``, the whole call (wall clock around a synchronous call), ``--frame-repeats`` times after a warm-up
  of the search at the same shape: every time and the median;
- the search alone (``_lib.anchor_distances``: validation and grid layout on the host, uploads, every kernel, the copy back),
  ``--repeats`` times; and the HIP-event time of each kernel from the context's timers, in one further call with the timers on;
- the frame assembly alone, ``--frame-repeats`` times: the same function fed the distances already computed;
- the yardstick, in the same run on the same box: sklearn's ``KDTree`` build + ``query`` per (anchor, slide) on one core, for the
  first ``--host-anchors`` anchors, and that time SCALED by anchors / host-anchors (an extrapolation: the loop is linear in the
  anchors); the device's distances are compared with sklearn's on those anchors before anything is written.

And the sweeps behind the constants of ``sqgr_anchor_dist_info`` (medians of ``--repeats`` timed calls, HIP-event time of the query
kernel plus the grid build): target points per cell on the 30-anchor input; one cell against a grid for sets of 16 .. 1024 points
queried by every spot; and the order of the queries — lattice order, shuffled, shuffled then sorted along the Z-order curve."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-anchors", type=int, default=3)
    ap.add_argument("--frame-repeats", type=int, default=3)
    a = ap.parse_args()

    import pandas as pd
    from sklearn.neighbors import KDTree

    import squidpy_amd as sq
    from squidpy_amd import _build, _lib, _synthetic
    from squidpy_amd.tl import _var_by_distance as V

    ctx = _lib.default_context()
    xy = np.ascontiguousarray(_synthetic.hex_grid(a.rows, a.cols), dtype=np.float64)
    n = len(xy)
    rng = np.random.default_rng(0)
    K = 30
    labels = rng.integers(0, K, n)
    names = [f"c{i}" for i in range(K)]
    width = float(np.ptp(xy[:, 0])) + 1.0
    strips = np.minimum(((xy[:, 0] - xy[:, 0].min()) / width * 8).astype(np.int64), 7)

    def adata_of(lab, slides):
        obs = {"cluster": pd.Categorical.from_codes(lab, names)}
        if slides is not None:
            obs["lib"] = pd.Categorical.from_codes(slides, [f"s{i}" for i in range(8)])
        return sq.AnnDataLite(obs=pd.DataFrame(obs, index=[f"cell_{i}" for i in range(n)]), obsm={"spatial": xy})

    def kernel_ms(case, repeats, **kw):
        """median over `repeats` calls of (query kernel ms, grid build ms), after one warm-up call"""
        _lib.anchor_distances(ctx, **case, **kw)
        ctx.timer_enable(True)
        q, b = [], []
        for _ in range(repeats):
            ctx.timer_reset()
            _lib.anchor_distances(ctx, **case, **kw)
            rep = ctx.timer_report()
            q.append(rep["anchor_query"][1])
            b.append(sum(v[1] for k, v in rep.items() if k in ("anchor_count", "anchor_scan", "anchor_scatter")))
        ctx.timer_enable(False)
        return float(np.median(q)), float(np.median(b))

    def measure(tag, lab, slides, anchors):
        adata = adata_of(lab, slides)
        kwargs = dict(groups=anchors, cluster_key="cluster", library_key=None if slides is None else "lib")
        captured = {}

        def capture(coords, slide_codes, ref_coords, ref_sets, set_of, metric):
            captured["case"] = dict(coords=coords, slide_codes=slide_codes, ref_coords=ref_coords, ref_sets=ref_sets, set_of=set_of)
            captured["dist"] = _lib.anchor_distances(ctx, coords, slide_codes, ref_coords, ref_sets, set_of, metric)
            return captured["dist"]

        plan_args = (adata, anchors, "cluster", kwargs["library_key"], None, None, "euclidean", "spatial")
        # warm-up of the search at the same shape; keeps its arguments
        V._Plan(adata, anchors, "cluster", kwargs["library_key"], None, "euclidean", "spatial").distances(capture, "euclidean")
        ctx.sync()
        case, dist = captured["case"], captured["dist"]
        whole, search, assembly = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            _lib.anchor_distances(ctx, **case)
            search.append(time.perf_counter() - t0)
        for _ in range(a.frame_repeats):  # (the frame of 1e6 rows and 60 columns takes pandas tens of seconds)
            t0 = time.perf_counter()
            sq.tl.var_by_distance(adata, copy=True, **kwargs)
            whole.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            V._design_matrix(*plan_args, lambda *_a: dist)
            assembly.append(time.perf_counter() - t0)
        ctx.timer_enable(True)
        ctx.timer_reset()
        _, stats = _lib.anchor_distances(ctx, **case, return_stats=True)
        kernels = {k: v for k, v in ctx.timer_report().items() if k.startswith("anchor_")}
        ctx.timer_enable(False)
        # the yardstick: the reference's loop over (anchor, slide), sklearn on one core, for the first anchors
        m = min(a.host_anchors, len(anchors))
        slide_list = [None] if slides is None else list(range(8))
        t0 = time.perf_counter()
        ref = np.full((m, n), np.nan)
        for j in range(m):
            for s in slide_list:
                rows = np.arange(n) if s is None else np.nonzero(slides == s)[0]
                members = rows[lab[rows] == names.index(anchors[j])]
                if len(members):
                    ref[j, rows] = KDTree(xy[members]).query(xy[rows])[0][:, 0]
        host_s = time.perf_counter() - t0
        assert np.array_equal(dist[:m], ref, equal_nan=True), "the device and sklearn disagree"
        return case, {
            "input": tag, "spots": n, "anchors": len(anchors), "slides": len(slide_list), "reference_points": int(stats["ref_points"]), "stats": stats,
            "whole_call_s": whole, "whole_call_median_s": float(np.median(whole)),
            "search_call_s": search, "search_call_median_s": float(np.median(search)),
            "frame_assembly_s": assembly, "frame_assembly_median_s": float(np.median(assembly)),
            "kernels_launches_ms": kernels, "kernels_total_ms": sum(v[1] for v in kernels.values()),
            "sklearn_anchors": m, "sklearn_threads": 1, "sklearn_s": host_s, "sklearn_scaled_to_all_anchors_s": host_s * len(anchors) / m,
            "sklearn_scaled_note": "measured" if m == len(anchors) else "scaled linearly from the first anchors; the other anchors were not run through sklearn",
        }

    results = []
    case1, r = measure("30 uniform labels, 1 slide", labels, None, names)
    results.append(r)
    print(json.dumps(r), flush=True)
    _, r = measure("30 uniform labels, 8 slides", labels, strips, names)
    results.append(r)
    print(json.dumps(r), flush=True)
    corner = (xy[:, 0] < xy[:, 0].min() + 0.1 * np.ptp(xy[:, 0])) & (xy[:, 1] < xy[:, 1].min() + 0.1 * np.ptp(xy[:, 1]))
    lab_c = np.where(corner, 0, 1 + labels % (K - 1))
    _, r = measure("one label confined to the corner 1 % of the area", lab_c, None, ["c0"])
    results.append(r)
    print(json.dumps(r), flush=True)

    info = _lib.anchor_dist_info()
    sweep_cell = []
    for per_cell in (1.0, 2.0, 4.0, 8.0, 16.0):
        q_ms, b_ms = kernel_ms(case1, a.repeats, brute_below=2, per_cell=per_cell)
        sweep_cell.append({"per_cell": per_cell, "query_ms": q_ms, "build_ms": b_ms})
        print(json.dumps(sweep_cell[-1]), flush=True)
    sweep_brute = []
    for size in (16, 32, 64, 128, 256, 1024):
        pts = xy[rng.choice(n, size, replace=False)]
        case = dict(coords=xy, slide_codes=np.zeros(n, np.int32), ref_coords=pts, ref_sets=np.zeros(size, np.int32), set_of=np.zeros((1, 1), np.int32))
        one, _ = kernel_ms(case, a.repeats, brute_below=10**9)
        grid, _ = kernel_ms(case, a.repeats, brute_below=2, per_cell=float(info["per_cell"]))
        sweep_brute.append({"set_size": size, "one_cell_query_ms": one, "grid_query_ms": grid})
        print(json.dumps(sweep_brute[-1]), flush=True)
    order = {}
    perm = rng.permutation(n)
    shuffled = dict(case1, coords=np.ascontiguousarray(case1["coords"][perm]), slide_codes=case1["slide_codes"][perm])
    z = _lib.spatial_order_device(ctx, shuffled["coords"])
    resorted = dict(case1, coords=np.ascontiguousarray(shuffled["coords"][z]), slide_codes=shuffled["slide_codes"][z])
    for tag, case in (("lattice_order", case1), ("shuffled", shuffled), ("shuffled_then_z_order", resorted)):
        order[tag + "_query_ms"] = kernel_ms(case, a.repeats)[0]
    print(json.dumps(order), flush=True)

    out = {"device": ctx.device_info(), "build_stamp": _build.source_fingerprint(), "anchor_dist_info": info, "repeats": a.repeats, "frame_repeats": a.frame_repeats,
           "inputs": results, "sweep_points_per_cell": sweep_cell, "sweep_one_cell_against_grid": sweep_brute, "query_order": order}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
