"""Timing of the PCA behind the utag and cellcharter flavours (sq.gr.niche_utag_embedding / niche_cellcharter_embedding / niche_pca)
on the device and of sklearn's ``PCA(svd_solver="arpack")`` on the same box.

    python tools/niche_pca_time.py [--out profiles/niche_pca_time.json] [--rows 1000000] [--skip-sklearn]

Workload: a hex lattice of ``rows`` spots x 50 dense float32 columns; CellCharter features at distance 3 (D = 200) and UTAG features
(D = 50), 50 and 49 components (the default rule).  Per workload: the whole embedding call (host checks, upload, shells, feature blocks filled on the
device, moments, the host eigenproblem, projection, the n x 50 result on the host; wall clock of a second call); ``niche_pca`` on the
feature matrix already on the host (its upload included); the HIP-event time per kernel from a run of its own; the host eigenproblem
alone; and the scatter kernel's share of the float64 issue ceiling: ``v_add_f64``'s measured rate (profiles/r06_ubench_f64.json) x 64
lanes / the float64 multiplies, adds and subtracts the kernel issues per row — counted from the loop structure of csrc/sqgr_pca.hip:
every upper-triangular 64 x 64 tile pair forms 4096 products and 4096 sums per row and centres its 64 (diagonal pair) or 128 staged
values; the useful ones are D (D + 1).
sklearn (``PCA(c, svd_solver="arpack", random_state=0).fit_transform``): on the first 1e5 rows of the same feature matrix with the
BLAS pool limited to 1 thread and to 16 threads, times ``rows`` / 1e5 as a stated scaling, not a measurement."""
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
from squidpy_amd import AnnDataLite  # noqa: E402
from squidpy_amd._lib import default_context, pca_info  # noqa: E402
from squidpy_amd.gr._niche import pca_components  # noqa: E402
from tests import niche_features_cases as FC  # noqa: E402

DISTANCE, N_VARS, N_COMPS, SKLEARN_ROWS = 3, 50, 50, 100_000


def scatter_ops(d: int) -> dict:
    tile = pca_info()["tile_columns"]
    nt = -(-d // tile)
    pairs = nt * (nt + 1) // 2
    return {"tile_pairs": pairs, "issued_per_row": pairs * 2 * tile * tile + nt * tile + (pairs - nt) * 2 * tile, "useful_per_row": d * (d + 1)}


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
    rep = {name: v for name, v in ctx.timer_report().items() if name.startswith(("niche", "pca"))}
    ctx.timer_enable(False)
    return {"shape": list(out.shape), "whole_call_s": wall, "kernels_launches_ms": rep, "kernel_sum_ms": sum(v[1] for v in rep.values())}


def ceilings(rep: dict, n: int, d: int, ceiling_lane_ops: float) -> dict:
    ops = scatter_ops(d)
    ms = rep["kernels_launches_ms"]["pca_scatter"][1]
    return {"scatter_ms": ms, **ops, "share_of_f64_issue_issued": n * ops["issued_per_row"] / ceiling_lane_ops / (ms * 1e-3),
            "share_of_f64_issue_useful": n * ops["useful_per_row"] / ceiling_lane_ops / (ms * 1e-3)}


def sklearn_time(x: np.ndarray, c: int, threads: int) -> dict:
    from sklearn.decomposition import PCA
    from threadpoolctl import threadpool_limits

    with threadpool_limits(limits=threads):
        t0 = time.perf_counter()
        PCA(n_components=c, svd_solver="arpack", random_state=0).fit_transform(x)
        wall = time.perf_counter() - t0
    return {"rows": len(x), "columns": x.shape[1], "components": c, "threads": threads, "fit_transform_s": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--skip-sklearn", action="store_true")
    a = ap.parse_args()
    ctx = default_context()
    with open(os.path.join(ROOT, "profiles", "r06_ubench_f64.json")) as fh:
        ceiling = {r["op"]: r["wave_instr_per_s"] for r in json.load(fh)["valu"]}["v_add_f64"] * 64
    side = int(round(np.sqrt(a.rows)))
    adj = FC.hex_lattice(side, a.rows // side)
    n = adj.shape[0]
    x = np.random.default_rng(N_VARS).random((n, N_VARS), dtype=np.float32)
    adata = AnnDataLite(X=x, obs=pd.DataFrame(index=[f"c{i}" for i in range(n)]), obsp={"spatial_connectivities": adj})
    report = {"device": ctx.device_info(), "f64_issue_ceiling_lane_ops_per_s": ceiling, "n_obs": n, "n_vars": N_VARS, "distance": DISTANCE,
              "n_comps": N_COMPS, "scatter_kernel": "VALU 4 x 4 register tiles (the f64 MFMA was not built)", "workloads": {}, "sklearn": {}}
    for name, embed, features in (
        ("cellcharter_d200", lambda: sq.gr.niche_cellcharter_embedding(adata, DISTANCE, "mean"), lambda: sq.gr.niche_cellcharter_features(adata, DISTANCE, "mean")),
        ("utag_d50", lambda: sq.gr.niche_utag_embedding(adata), lambda: sq.gr.niche_utag_features(adata)),
    ):
        w = {"embedding": timed(ctx, embed)}
        feats = features()
        d = feats.shape[1]
        c = min(N_COMPS, d - 1)
        w["columns"], w["components"] = d, c
        w["embedding"]["ceilings"] = ceilings(w["embedding"], n, d, ceiling)
        w["niche_pca_of_host_features"] = timed(ctx, lambda: sq.gr.niche_pca(feats, c).X_pca)
        w["niche_pca_of_host_features"]["ceilings"] = ceilings(w["niche_pca_of_host_features"], n, d, ceiling)
        scatter = np.cov(feats[:20000].astype(np.float64), rowvar=False) * 19999
        t0 = time.perf_counter()
        pca_components(scatter, 20000, c)
        w["host_eigenproblem_s"] = time.perf_counter() - t0
        report["workloads"][name] = w
        print(name, json.dumps(w), flush=True)
        if not a.skip_sklearn:
            rows = min(n, SKLEARN_ROWS)
            sub = np.ascontiguousarray(feats[:rows])
            for threads in (1, 16):
                s = sklearn_time(sub, c, threads)
                s["scaled_to_rows_s"] = s["fit_transform_s"] * n / rows
                s["note"] = f"timed on {rows} rows; x{n / rows:.1f} is a scaling, not a measurement"
                report["sklearn"][f"{name}_threads{threads}"] = s
                print("sklearn", name, json.dumps(s), flush=True)
        del feats
    sq._lib.clear_graph_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
