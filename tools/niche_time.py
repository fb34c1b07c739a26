"""Timing of squidpy_amd.gmm_fit (the mixture behind sq.gr.calculate_niche_cellcharter) on the device and of sklearn on the same box.

    python tools/niche_time.py [--out profiles/niche_time.json] [--rows 1000000] [--skip-sklearn]

Workloads: planted Gaussian data, ``rows`` x d with k = d components, d = 10 (the front end's default) and d = 50 (a scVI
representation).  Per workload: the whole ``gmm_fit`` call (host checks, upload, every EM step, labels; wall clock), the
HIP-event time per kernel and per EM step from a run of its own, and each of the two heavy kernels' share of the float64 issue
ceiling: ``v_add_f64``'s measured rate (profiles/r06_ubench_f64.json) x 64 lanes / the kernel's float64 multiplies, adds and
subtracts per row and component (counted from the loop structure of csrc/sqgr_gmm.hip, see ``f64_ops``).
sklearn (``GaussianMixture(k, random_state=0, init_params="random_from_data", tol=0, max_iter=STEPS).fit``): seconds per EM step
with the BLAS pool limited to 1 thread and to 16 threads; at d = k = 50 on a tenth of the rows, times 10 as a stated scaling."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import squidpy_amd as sq  # noqa: E402
from squidpy_amd._lib import default_context  # noqa: E402

SKLEARN_STEPS = 3


def planted(n: int, d: int, k: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 2.0, (k, d))
    member = rng.choice(k, size=n, p=rng.dirichlet(np.full(k, 4.0)))
    return centres[member] + rng.normal(0.0, 1.0, (n, d))


def f64_ops(d: int) -> dict:
    """float64 multiplies / adds / subtracts per row and component, as the kernels issue them (padding included)."""
    strips = -(-d // 16)
    estep = sum(min(d, 16 * (s + 1)) * (1 + 32) + 32 for s in range(strips))  # per strip: rows of P x (sub + 16 mul + 16 add) + 16 squares
    nbt = -(-d // 4)
    cov = nbt * (nbt + 1) // 2 * 32 + 2 * 4 * nbt  # 4 x 4 tiles of the upper triangle x (mul + add) + staging (sub, mul)
    return {"estep": estep, "cov": cov, "useful_estep": d * (d + 1) + 2 * d, "useful_cov": d * (d + 1)}


def device(ctx, x: np.ndarray, k: int, ceiling_lane_ops: float) -> dict:
    n, d = x.shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        ctx.sync()
        t0 = time.perf_counter()
        fit = sq.gmm_fit(x, k, 0)
        first = time.perf_counter() - t0
        t0 = time.perf_counter()
        fit2 = sq.gmm_fit(x, k, 0)
        second = time.perf_counter() - t0
        ctx.timer_enable(True)  # a run of its own: the event pairs around every launch cost host time
        ctx.timer_reset()
        fit3 = sq.gmm_fit(x, k, 0)
        ctx.sync()
        rep = {name: v for name, v in ctx.timer_report().items() if name.startswith("gmm")}
        ctx.timer_enable(False)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for f in (fit2, fit3) for a, b in zip(fit, f))
    per_launch = {name: ms / max(cnt, 1) for name, (cnt, ms) in rep.items()}
    ops = f64_ops(d)
    share = {}
    for kernel, key in (("gmm_estep", "estep"), ("gmm_cov", "cov")):
        floor_ms = n * k * ops[key] / ceiling_lane_ops * 1e3
        share[kernel] = floor_ms / per_launch[kernel]
    step_ms = sum(per_launch[name] for name in ("gmm_estep", "gmm_lower_bound", "gmm_sums", "gmm_means", "gmm_cov", "gmm_cholesky"))
    return {"n": n, "d": d, "k": k, "n_iter": fit.n_iter, "converged": fit.converged, "whole_call_first_s": first, "whole_call_second_s": second,
            "kernels_launches_ms": rep, "ms_per_launch": per_launch, "ms_per_em_step": step_ms, "kernel_sum_ms": sum(v[1] for v in rep.values()),
            "f64_ops_per_row_component": ops, "share_of_f64_issue_ceiling": share, "component_sizes_head": np.bincount(fit.labels, minlength=k)[:5].tolist()}


def sklearn_time(x: np.ndarray, k: int, threads: int) -> dict:
    from sklearn.mixture import GaussianMixture
    from threadpoolctl import threadpool_limits

    with threadpool_limits(limits=threads), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm = GaussianMixture(n_components=k, random_state=0, init_params="random_from_data", tol=0.0, max_iter=SKLEARN_STEPS)
        t0 = time.perf_counter()
        gmm.fit(x)
        wall = time.perf_counter() - t0
    return {"rows": len(x), "threads": threads, "steps": int(gmm.n_iter_), "fit_s": wall, "s_per_em_step": wall / max(int(gmm.n_iter_), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--skip-sklearn", action="store_true")
    a = ap.parse_args()
    ctx = default_context()
    with open(os.path.join(ROOT, "profiles", "r06_ubench_f64.json")) as fh:
        ubench = {r["op"]: r["wave_instr_per_s"] for r in json.load(fh)["valu"]}
    ceiling = ubench["v_add_f64"] * 64
    report = {"device": ctx.device_info(), "f64_issue_ceiling_lane_ops_per_s": ceiling, "workloads": {}, "sklearn": {}}
    for d in (10, 50):
        x = planted(a.rows, d, d, seed=d)
        report["workloads"][f"d{d}k{d}"] = w = device(ctx, x, d, ceiling)
        print(f"d{d}k{d}", json.dumps(w), flush=True)
        if not a.skip_sklearn:
            scale = 1 if d == 10 else 10
            xs = x[: len(x) // scale]
            for threads in (1, 16):
                s = sklearn_time(xs, d, threads)
                s["scaled_s_per_em_step_at_all_rows"] = s["s_per_em_step"] * scale
                if scale != 1:
                    s["note"] = f"timed on 1/{scale} of the rows; x{scale} is a scaling, not a measurement"
                report["sklearn"][f"d{d}k{d}_{threads}_threads"] = s
                print(f"sklearn d{d}k{d} {threads} threads", json.dumps(s), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
