"""Timing of ``sq.gr.niche_neighbors`` (csrc/sqgr_knn_nd.hip) on the device, of sklearn's searches on the same box, and the accuracy of
the device's float64 ``exp`` that tests/test_niche_neighbors_gpu.py takes its bound from.

    python tools/niche_neighbors_time.py [--out profiles/niche_neighbors_time.json] [--legs gpu_1e5,gpu_1e6_d30,gpu_1e6_d50,exp_sweep,sklearn]

The driver runs every leg as a process of its own under ``timeout -k 10 <seconds>`` sized to that leg, chained with ``&&`` (a leg that
fails or runs out of time ends the run; nothing starts on the device after it), and merges what the legs wrote.

- ``gpu_1e5``: 1e5 rows of a standard normal cloud at D = 30 and D = 50, ``n_neighbors = 15``; ``gpu_1e6_d30`` / ``gpu_1e6_d50``: 1e6 rows,
  one step each.  Per shape: the whole call (host checks, upload, search, square roots, the bandwidth kernel, both CSR matrices and the
  host symmetrisation; wall clock), the HIP-event time of each kernel, the host symmetrisation alone, and the search kernel's share of the
  float64 issue ceiling: ``3 D n (n - 1)`` subtractions, products and sums over the kernel time over ``v_add_f64``'s measured rate x 64
  lanes (profiles/r06_ubench_f64.json).
- ``exp_sweep``: rows of 64 ascending distances spread log-uniformly over six decades, so that the arguments ``-(d - rho) / sigma`` the
  bandwidth kernel hands to ``exp`` cover [-745, 0]; the kernel's ``vals`` against ``exp`` of the same arguments in extended precision
  (numpy's ``longdouble``: 64 bits of mantissa), in units of the last place of the correctly rounded result.
- ``sklearn``: ``NearestNeighbors(n_neighbors=15, algorithm="kd_tree" | "brute")`` fitted on 1e5 rows (D = 30) and queried with the first
  ``--sklearn-queries`` of them, 1 and 16 threads, times 1e5 / queries as a stated scaling, not a measurement.  No device."""
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

N_NEIGHBORS = 15
LEG_SECONDS = {"gpu_1e5": 150, "gpu_1e6_d30": 300, "gpu_1e6_d50": 400, "exp_sweep": 240, "sklearn": 600}


def ceiling_lane_ops() -> float:
    with open(os.path.join(ROOT, "profiles", "r06_ubench_f64.json")) as fh:
        return {r["op"]: r["wave_instr_per_s"] for r in json.load(fh)["valu"]}["v_add_f64"] * 64


def cloud(n: int, d: int) -> np.ndarray:
    return np.random.default_rng(d).normal(size=(n, d))


def timed_shape(ctx, n: int, d: int, repeat: bool) -> dict:
    import squidpy_amd as sq
    from squidpy_amd.gr._niche_graph import connectivities_from_memberships

    x = cloud(n, d)
    if repeat:
        sq.gr.niche_neighbors(x, N_NEIGHBORS)  # sizes the pool
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    res = sq.gr.niche_neighbors(x, N_NEIGHBORS)
    wall = time.perf_counter() - t0
    rep = {name: v for name, v in ctx.timer_report().items() if name.startswith(("knn_nd", "fuzzy_knn"))}
    ctx.timer_enable(False)
    vals = np.exp(-np.maximum(res.knn_distances - res.rho[:, None], 0.0) / res.sigma[:, None])  # stand-in of equal sparsity for the timing
    t0 = time.perf_counter()
    connectivities_from_memberships(res.knn_indices, vals)
    sym = time.perf_counter() - t0
    ms = rep["knn_nd"][1]
    ops = 3.0 * d * n * (n - 1)
    return {"rows": n, "columns": d, "n_neighbors": N_NEIGHBORS, "first_call_of_its_size": not repeat, "whole_call_s": wall,
            "kernels_launches_ms": rep, "host_symmetrisation_s": sym, "search_f64_lane_ops": ops,
            "search_share_of_f64_issue_ceiling": ops / (ms * 1e-3) / ceiling_lane_ops(),
            "connectivities_nnz": int(res.connectivities.nnz)}


def leg_gpu(shapes, repeat: bool) -> dict:
    import squidpy_amd as sq
    from squidpy_amd._lib import default_context

    ctx = default_context()
    sq.gr.niche_neighbors(cloud(3000, 8), N_NEIGHBORS)  # loads the code objects
    out = {"device": ctx.device_info()}
    for n, d in shapes:
        out[f"n{n}_d{d}"] = timed_shape(ctx, n, d, repeat)
        print(f"n{n}_d{d}", json.dumps(out[f"n{n}_d{d}"]), flush=True)
    return out


def leg_exp_sweep(rows: int = 400_000, k: int = 64) -> dict:
    from squidpy_amd._lib import default_context, fuzzy_knn

    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision longdouble"
    rng = np.random.default_rng(64)
    dist = np.sort(10.0 ** rng.uniform(-3.0, 3.0, size=(rows, k)), axis=1)
    rho, sigma, _, vals = fuzzy_knn(default_context(), dist, float(dist.sum() / (rows * (k + 1))))
    assert np.array_equal(rho, dist[:, 0])
    e = dist - rho[:, None]
    arg = -(e / sigma[:, None])
    keep = e > 0
    ref = np.exp(arg[keep].astype(np.longdouble))
    ref64 = ref.astype(np.float64)
    got = vals[keep]
    a = arg[keep]
    live = ref64 > 0
    err = np.abs(got[live].astype(np.longdouble) - ref[live]) / np.spacing(ref64[live]).astype(np.longdouble)
    a = a[live]
    out = {"rows": rows, "k": k, "arguments": int(keep.sum()), "arguments_with_a_nonzero_result": int(live.sum()),
           "results_that_round_to_zero_and_are_zero": int((got[~live] == 0).sum()), "results_that_round_to_zero": int((~live).sum()),
           "unit": "last place of the correctly rounded result", "worst_ulp": float(err.max()), "by_argument": {}}
    for lo, hi in ((-1.0, 0.0), (-10.0, -1.0), (-100.0, -10.0), (-708.0, -100.0), (-746.0, -708.0)):
        m = (a >= lo) & (a < hi)
        out["by_argument"][f"[{lo:g}, {hi:g})"] = {"count": int(m.sum()), "worst_ulp": float(err[m].max()) if m.any() else None}
    print("exp_sweep", json.dumps(out), flush=True)
    return out


def leg_sklearn(queries: int, rows: int = 100_000, d: int = 30) -> dict:
    from sklearn.neighbors import NearestNeighbors
    from threadpoolctl import threadpool_limits

    x = cloud(rows, d)
    out = {}
    for algorithm in ("kd_tree", "brute"):
        for threads in (1, 16):
            with threadpool_limits(limits=threads):
                t0 = time.perf_counter()
                nn = NearestNeighbors(n_neighbors=N_NEIGHBORS, algorithm=algorithm, n_jobs=threads).fit(x)
                fit = time.perf_counter() - t0
                t0 = time.perf_counter()
                nn.kneighbors(x[:queries])
                query = time.perf_counter() - t0
            out[f"{algorithm}_threads{threads}"] = {
                "rows": rows, "columns": d, "queries": queries, "threads": threads, "fit_s": fit, "query_s": query,
                "scaled_to_all_rows_s": fit + query * rows / queries,
                "note": f"queried with {queries} of the {rows} rows; x{rows / queries:.1f} is a scaling, not a measurement"}
            print("sklearn", algorithm, threads, json.dumps(out[f"{algorithm}_threads{threads}"]), flush=True)
    return out


def run_leg(name: str, a) -> dict:
    if name == "gpu_1e5":
        return leg_gpu([(100_000, 30), (100_000, 50)], repeat=True)
    if name == "gpu_1e6_d30":
        return leg_gpu([(1_000_000, 30)], repeat=False)
    if name == "gpu_1e6_d50":
        return leg_gpu([(1_000_000, 50)], repeat=False)
    if name == "exp_sweep":
        return leg_exp_sweep()
    if name == "sklearn":
        return leg_sklearn(a.sklearn_queries)
    raise SystemExit(f"unknown leg {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=",".join(LEG_SECONDS))
    ap.add_argument("--sklearn-queries", type=int, default=2_000)
    ap.add_argument("--leg", default=None, help="(internal) run one leg and write its part")
    ap.add_argument("--part", default=None)
    a = ap.parse_args()
    if a.leg:
        part = run_leg(a.leg, a)
        with open(a.part, "w") as fh:
            json.dump(part, fh)
        return
    legs = [s for s in a.legs.split(",") if s]
    with tempfile.TemporaryDirectory() as tmp:
        steps = [f"timeout -k 10 {LEG_SECONDS[leg]} {sys.executable} {os.path.abspath(__file__)} --leg {leg} --part {tmp}/{leg}.json "
                 f"--sklearn-queries {a.sklearn_queries}" for leg in legs]
        rc = subprocess.run(" && ".join(steps), shell=True, cwd=ROOT).returncode
        report = {"f64_issue_ceiling_lane_ops_per_s": ceiling_lane_ops(), "exit_status": rc, "legs": {}}
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
