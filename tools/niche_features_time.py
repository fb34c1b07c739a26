"""Timing of the niche feature matrices (sq.gr.niche_nhood_profile / niche_utag_features / niche_cellcharter_features) on the device
and of the same sparse steps in scipy on the same box.

    python tools/niche_features_time.py [--out profiles/niche_features_time.json] [--rows 1000000] [--rows-wide 100000] [--skip-cpu]

Inputs: a hex lattice and a directed kNN-6 graph of ``rows`` spots, 30 categories, distance 3; ``n_vars`` = 50 (dense float32) on
``rows`` spots and ``n_vars`` = 2 000 (CSR float32, 20 entries per row) on ``rows-wide`` spots — the CellCharter result of 2 000
variables is 64 GB at 1e6 spots, so the wide case runs on fewer.  Per workload: the whole call (host checks, upload, kernels, result on
the host; wall clock of a second call), and the HIP-event time per kernel from a run of its own.

For the aggregation kernel the achieved fraction of two ceilings, from the measured kernel time: HBM — the bytes it must move
(every column block read once and written once per sparse block, 4 bytes per stored entry and 16 per row for the indices, row
pointers and scales; the gathers of the neighbours' rows are left to the caches) against 6.29 TB/s, the measured copy rate of the
device; float64 issue — one multiply and one add per stored entry and column against ``v_add_f64``'s measured rate
(profiles/r06_ubench_f64.json) x 64 lanes.

CPU baseline (``--skip-cpu`` leaves it out): the reference's steps written with the same scipy calls — sparse products, a comparison
and a sum per shell, a normalised product per block; ``A @ A @ ...`` and column-sliced sums for the profile — on 1e5 rows, scaled to
``rows`` as a stated scaling, not a measurement.  The reference package itself is not importable where this runs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import squidpy_amd as sq  # noqa: E402
from squidpy_amd import AnnDataLite  # noqa: E402
from squidpy_amd._lib import Graph, HopShells, default_context  # noqa: E402
from tests import niche_features_cases as FC  # noqa: E402

HBM_MEASURED = 6.29e12  # bytes / s, float4 copy
DISTANCE, CATEGORIES = 3, 30


def wide_expression(n: int, n_vars: int, per_row: int, seed: int) -> sparse.csr_matrix:
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.integers(0, n_vars, (n, per_row)), axis=1)
    x = sparse.csr_matrix((rng.integers(1, 10, n * per_row).astype(np.float32), cols.ravel(), np.arange(0, n * per_row + 1, per_row)), shape=(n, n_vars))
    x.sum_duplicates()
    return x


def graphs(n: int) -> dict:
    side = int(round(np.sqrt(n)))
    return {"hex": FC.hex_lattice(side, n // side), "knn6": FC.knn_graph(n, 6, 7)}


def timed(ctx, fn) -> dict:
    fn()  # first call: uploads the graph into the cache, sizes the pool
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    wall = time.perf_counter() - t0
    ctx.timer_enable(True)
    ctx.timer_reset()
    fn()
    ctx.sync()
    rep = {name: v for name, v in ctx.timer_report().items() if name.startswith(("niche", "autocorr_csr_to_csc"))}
    ctx.timer_enable(False)
    return {"shape": list(out.shape), "whole_call_s": wall, "kernels_launches_ms": rep, "kernel_sum_ms": sum(v[1] for v in rep.values())}


def shell_entries(ctx, a) -> list:
    g = Graph(ctx, a, with_data=False)
    shells = HopShells(ctx, g, DISTANCE)
    try:
        return [shells.info(k)["hop_nnz"] for k in range(1, DISTANCE + 1)]
    finally:
        shells.close()
        g.close()


def aggregate_ceilings(rep: dict, n: int, n_vars: int, entries: list, f64_lane_ops: float) -> dict:
    """Shares of the HBM and float64-issue ceilings of the `niche_aggregate` launches of one call: ``entries`` = stored entries of every
    sparse block walked (block 0 of the shells is a copy and launches no aggregation)."""
    ms = rep["kernels_launches_ms"]["niche_aggregate"][1]
    hbm_bytes = len(entries) * 2 * n * n_vars * 8 + sum(entries) * 4 + len(entries) * n * 16
    flops = 2 * sum(entries) * n_vars
    return {"aggregate_ms": ms, "stored_entries": entries, "hbm_bytes": hbm_bytes, "share_of_hbm_6.29TBs": hbm_bytes / HBM_MEASURED / (ms * 1e-3),
            "f64_ops": flops, "share_of_f64_issue": flops / f64_lane_ops / (ms * 1e-3)}


def cpu_baseline(a, x, codes) -> dict:
    """The reference's steps with its scipy calls, timed stage by stage."""
    out = {"rows": a.shape[0]}
    t0 = time.perf_counter()
    hop = a.tolil()
    hop.setdiag(0)
    hop = hop.tocsr()
    hop.eliminate_zeros()
    vis = a.tolil()
    vis.setdiag(1)
    vis = vis.tocsr()
    blocks = [x]
    for k in range(1, DISTANCE + 1):
        if k > 1:
            hop = hop @ a
            hop = hop > vis
            vis = vis + hop
        deg = np.asarray(hop.sum(axis=1)).ravel()
        with np.errstate(divide="ignore"):
            inv = np.where(deg > 0, 1.0 / deg, 0.0)
        blocks.append(sparse.diags(inv) @ hop @ x)
    arr = sparse.hstack([sparse.csr_matrix(b) for b in blocks]).toarray()
    out["cellcharter_mean_s"] = time.perf_counter() - t0
    del arr
    t0 = time.perf_counter()
    from sklearn.preprocessing import normalize

    normalize(a, norm="l1", axis=1) @ x
    out["utag_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    power = a.copy()
    for h in range(DISTANCE):
        if h:
            power = power @ a
        csc = power.tocsc()
        prof = np.stack([np.asarray(csc[:, np.flatnonzero(codes == c)].sum(axis=1)).ravel() for c in range(CATEGORIES)], axis=1)
        with np.errstate(invalid="ignore"):
            prof = np.nan_to_num(prof / prof.sum(axis=1, keepdims=True))
    out["nhood_profile_s"] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rows-wide", type=int, default=100_000)
    ap.add_argument("--skip-cpu", action="store_true")
    a = ap.parse_args()
    ctx = default_context()
    with open(os.path.join(ROOT, "profiles", "r06_ubench_f64.json")) as fh:
        f64 = {r["op"]: r["wave_instr_per_s"] for r in json.load(fh)["valu"]}["v_add_f64"] * 64
    report = {"device": ctx.device_info(), "f64_issue_ceiling_lane_ops_per_s": f64, "hbm_measured_bytes_per_s": HBM_MEASURED, "distance": DISTANCE,
              "workloads": {}, "cpu": {}}
    for n, n_vars in ((a.rows, 50), (a.rows_wide, 2000)):
        for gname, adj in graphs(n).items():
            n_obs = adj.shape[0]
            rng = np.random.default_rng(n_vars)
            x = rng.random((n_obs, n_vars), dtype=np.float32) if n_vars == 50 else wide_expression(n_obs, n_vars, 20, 3)
            codes = rng.integers(0, CATEGORIES, n_obs)
            obs = pd.DataFrame({"cell_type": pd.Categorical.from_codes(codes, [f"t{i:02d}" for i in range(CATEGORIES)])})
            adata = AnnDataLite(X=x, obs=obs, obsp={"spatial_connectivities": adj})
            w = {"n_obs": n_obs, "n_vars": n_vars, "graph_nnz": int(adj.nnz)}
            w["cellcharter_mean"] = timed(ctx, lambda: sq.gr.niche_cellcharter_features(adata, DISTANCE, "mean"))
            w["shell_entries"] = shell_entries(ctx, adj)
            w["cellcharter_mean"]["ceilings"] = aggregate_ceilings(w["cellcharter_mean"], n_obs, n_vars, w["shell_entries"], f64)
            w["cellcharter_variance"] = timed(ctx, lambda: sq.gr.niche_cellcharter_features(adata, DISTANCE, "variance"))
            w["utag"] = timed(ctx, lambda: sq.gr.niche_utag_features(adata))
            w["utag"]["ceilings"] = aggregate_ceilings(w["utag"], n_obs, n_vars, [int(adj.nnz)], f64)
            if n_vars == 50:
                w["nhood_profile"] = timed(ctx, lambda: sq.gr.niche_nhood_profile(adata, "cell_type", distance=DISTANCE))
            report["workloads"][f"{gname}_n{n_obs}_v{n_vars}"] = w
            print(gname, n_obs, n_vars, json.dumps(w), flush=True)
            if not a.skip_cpu and n_vars == 50:
                m = min(n_obs, 100_000)
                sub = graphs(m)[gname]
                c = cpu_baseline(sub, sparse.csr_matrix(x[: sub.shape[0]].astype(np.float64)), codes[: sub.shape[0]])
                scale = n_obs / sub.shape[0]
                c["scaled_to_rows"] = {k: v * scale for k, v in c.items() if k.endswith("_s")}
                c["note"] = f"timed on {sub.shape[0]} rows; x{scale:.1f} is a scaling, not a measurement"
                report["cpu"][f"{gname}_v{n_vars}"] = c
                print("cpu", gname, json.dumps(c), flush=True)
            sq._lib.clear_graph_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
