#!/usr/bin/env python
"""Benchmark of the sq.gr hot path on MI355X (contract: see the task statement / DESIGN.md §Measurement).

    python bench.py --gpus N --steps K --warmup W [--scaling weak|strong --total-perms P] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps of the headline and prints its line (the headline's ``roofline`` / ``kernels``
come from the HIP-event timers of those same steps).  Every other measurement below — ``secondary``, ``legs``,
``numpy_stream_mode``, ``cpu_baseline``, ``emulated_ranks`` and the detail file — runs only with ``--full`` (the ``--no-*``
options then leave single parts out).  ``--dump-outputs DIR`` writes what the last timed step returned (rank 0):
``moments_s1.npy`` / ``moments_s2.npy`` (the step's sums of d and d^2, d = count - expected, float64, exact), ``zscore.npy``
(the z-scores of that step's permutations alone) and ``counts.npy`` (the observed counts); the inputs depend only on the arguments.

Workload (N=1): ``nhood_enrichment`` permutation test on the 1e6-spot hex grid x 30 clusters that BASELINE.json's
metric is quoted on (config 5's shape); one *step* = one pass of the hot path over one batch of permutations with
graph and labels already resident in HBM.  N>1: one process per GPU started by any launcher that exports
RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (``python -m torch.distributed.run``); the ranks find each other through
squidpy_amd's own socket rendezvous — torch is not imported — and every step ends with the path's one real exchange:
the all-reduce of the exact integer moments, done ON THE DEVICE by RCCL inside libsqgr (``sqgr_nhood_set_comm``).

* ``--scaling weak`` (default): every rank runs ``--perms-per-step`` (10 000) permutations per step, disjoint global
  permutation indices per rank and step.
* ``--scaling strong``: a step is BASELINE config 5 as specified — ``--total-perms`` (100 000) permutations split
  1/N over the ranks.

Rank 0 prints ONE JSON line:

* ``roofline``            the CSR-gather kernel (``nhood_count*``) against HBM: measured memory-side traffic per launch (PMC
                          of this build and workload, 2 x FETCH_SIZE + WRITE_SIZE as calibrated in
                          profiles/<round>_fetch_calibration.json) / its HIP-event time / 8 TB/s; ``frac`` is the compulsory-DRAM
                          model (no counter separates Infinity-Cache hits).  SURVEY §8d's algorithmic bytes exceed the traffic by
                          ``algorithmic_reuse`` (16 permutations per pass over the edge list).
                          ``issue_limits``: what actually limits the kernel — the L1 access rate of its label-row gathers,
                          the ``ds_add_u32`` rate of its LDS atomics, VALU issue — each against a rate measured on this chip.
* ``kernels``             the same for the other kernels of the step (label shuffle: VALU issue; reduce: HBM).
* ``secondary``           Moran's I genes/s on the config-3 shape — SURVEY §8d's directed kNN-6 graph, 2048 genes resident per
                          step (LDS-read bound; p-value reductions on the device).
* ``legs``                co_occurrence / Ripley L / Ripley G on the config-4 shape; Geary's C (hex grid: row-sum classes) and
                          Geary's general kernel (arbitrary float64 weights) on the config-3 shape; config 3 IN FULL through the
                          front end (20 000 genes, upload included); the headline's other regimes — 64 / 100 / 200 clusters, the
                          directed kNN-6 graph, Dirichlet cluster sizes (``nhood_*``); every leg with its own ``roofline``, the
                          statistics' legs with a ``cpu_baseline`` (Ripley: the reference's own sklearn calls).
* ``numpy_stream_mode``   the test with numpy's own PCG64 streams reproduced bit for bit on the GPU.
* ``cpu_baseline``        the oracle's C restatement of Squidpy's numba kernel driven by numpy's PCG64 shuffles, timed
                          on this box's host cores on a bounded sample (N=1, rank 0 only).
* ``emulated_ranks``      (``--emulate-ranks N``) the N shards of config 5 run one after the other on this GPU: a projection.
PMC-derived inputs (HBM traffic, instruction counts per launch) cannot be collected inside this process; they come from
``profiles/<PROFILE_TAG>_counters.json``, written by ``tools/profile_round.sh`` from rocprofv3 ``--pmc`` passes of THIS command, and
are used only when that file was taken from this build of the kernels (``source_sha16``) on this workload."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = COLS = 1000
N_CLS = 30
PERMS_PER_STEP = 10_000
HBM_PEAK = 8.0e12   # B/s, MI355X_MICROARCH.md
L2_PEAK = 34.5e12   # B/s aggregate L2 bandwidth, MI355X_MICROARCH.md §L2
LDS_READ_PEAK = 256 * 256 * 2.4e9  # B/s: 256 B/clk/CU (ds_read_b64/b128, MI355X_MICROARCH.md §LDS) x 256 CUs x 2.4 GHz
PROFILE_TAG = "r06"


# --------------------------------------------------------------------------------------------- measured ceilings
def _profile(name: str) -> str:
    """profiles/<tag>_<name> of this round; an earlier round's file only while this round's lease has not produced its own (the
    `source` / `ceiling_source` fields of the record say which file was read)."""
    for tag in (PROFILE_TAG, "r05", "r04", "r03", "r02"):
        path = os.path.join(ROOT, "profiles", f"{tag}_{name}")
        if os.path.exists(path):
            return path
    return os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_{name}")


def load_ceilings() -> dict:
    """Issue-rate ceilings measured by tools/ubench_ops.hip on an MI355X (committed: profiles/<tag>_ubench_ops.json)."""
    path = _profile("ubench_ops.json")
    out = {"source": os.path.relpath(path, ROOT), "valu_simple": None, "valu_complex": None, "lds_add": None, "lds_add_pattern": None}
    try:
        with open(path) as fh:
            ub = json.load(fh)
        ops = {r["op"]: r["wave_instr_per_s"] for r in ub["valu"]}
        simple = [ops[k] for k in ("v_fma_f32", "v_add_u32", "v_sub_u32", "v_xor_b32", "v_and_b32", "v_lshrrev_b32") if k in ops]
        cplx = [v for k, v in ops.items() if k.startswith(("v_pk_", "v_mad_u32_u24", "v_mul_u32_u24", "v_lshl_", "v_alignbit", "v_perm", "v_bfe")) or "sdwa" in k or "dpp" in k]
        out["valu_simple"] = float(np.mean(simple))     # wave-instructions/s, whole chip: add/sub/xor/and/shift/fma class
        out["valu_complex"] = float(np.mean(cplx))      # packed-16, VOP3, SDWA, DPP, 24-bit multiply class
        lds = {r["pattern"]: r["wave_instr_per_s"] for r in ub["lds"]}
        out["lds_add"] = max(v for k, v in lds.items() if "conflict-free" in k)
        out["lds_add_pattern"] = max(v for k, v in lds.items() if "count-kernel pattern" in k and "57.6" in k)
    except Exception as exc:  # pragma: no cover
        out["error"] = repr(exc)
    return out


def load_counters() -> dict:
    """PMC averages written by tools/profile_round.sh.  They are used only if they come from THIS build of the kernels
    (`source_sha16` = squidpy_amd._build.source_fingerprint()) — and, per kernel, from this workload (kernel_counters)."""
    from squidpy_amd._build import source_fingerprint

    path = os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_counters.json")
    try:
        with open(path) as fh:
            d = json.load(fh)
    except Exception:
        return {"_status": f"no {os.path.relpath(path, ROOT)}"}
    if d.get("source_sha16") != source_fingerprint():
        return {"_status": f"{os.path.relpath(path, ROOT)} was taken from another build of the kernels (source_sha16 {d.get('source_sha16')} != "
                           f"{source_fingerprint()}): PMC fields left null; re-run tools/profile_round.sh"}
    d["_source"] = os.path.relpath(path, ROOT)
    d["_status"] = "ok"
    return d


def load_f64_ceilings() -> dict:
    """float64 VALU issue costs measured by tools/ubench_f64.hip (committed: profiles/r03_ubench_f64.json) as multiples of
    v_fma_f32 measured in the same process — the ratio does not depend on the clock the chip sustained during the run."""
    path = _profile("ubench_f64.json")
    out = {"source": os.path.relpath(path, ROOT)}
    try:
        with open(path) as fh:
            for r in json.load(fh)["valu"]:
                out[r["op"]] = r["cost_vs_v_fma_f32"]
    except (OSError, ValueError, KeyError):
        pass
    return out


def load_ds_mix(name: str) -> dict | None:
    """DS wave-instructions/s of a named LDS instruction mix at full occupancy (tools/ubench_ds_mix.hip, profiles/r03_ubench_ds_mix.json)."""
    path = _profile("ubench_ds_mix.json")
    try:
        with open(path) as fh:
            rows = [r for r in json.load(fh)["ds_mix"] if r["mix"] == name]
        best = max(rows, key=lambda r: r["ds_wave_instr_per_s"])
        return {"rate": best["ds_wave_instr_per_s"], "source": os.path.relpath(path, ROOT)}
    except (OSError, ValueError, KeyError):
        return None


def load_lds_read_ceilings() -> dict:
    """LDS read rates measured by tools/ubench_lds_read.hip on an MI355X (committed: profiles/<tag>_ubench_lds_read.json)."""
    path = _profile("ubench_lds_read.json")
    out = {"source": os.path.relpath(path, ROOT), "random_b128_bytes_per_s": None, "linear_b128_bytes_per_s": None, "scheduled_b128_bytes_per_s": None}
    try:
        with open(path) as fh:
            rows = json.load(fh)["lds_read"]
        for r in rows:
            if r["pattern"].startswith("ds_read_b128 random 16-byte rows"):
                out["random_b128_bytes_per_s"] = r["bytes_per_s"]
            if r["pattern"].startswith("ds_read_b128 random rows, row mod 16 = lane mod 16"):  # 16 row classes per service group
                out["scheduled_b128_bytes_per_s"] = r["bytes_per_s"]
            if r["pattern"].startswith("ds_read_b128 conflict-free"):
                out["linear_b128_bytes_per_s"] = r["bytes_per_s"]
    except (OSError, ValueError, KeyError):
        pass
    return out


def load_gather_rate() -> dict:
    """L2 random-access rate measured by tools/ubench_gather.hip: random 16-byte rows out of a 16 MB table (rows/s, chip-wide)."""
    path = _profile("ubench_gather.json")
    out = {"source": os.path.relpath(path, ROOT), "random_rows_per_s": None}
    try:
        with open(path) as fh:
            rows = json.load(fh)["gather"]
        rates = [r.get("rows_per_s") for r in rows if "random" in str(r.get("pattern", "")) and r.get("rows_per_s")]
        out["random_rows_per_s"] = max(rates) if rates else None
    except (OSError, ValueError, KeyError):
        pass
    return out


def kernel_counters(counters: dict, kernel_prefix: str, workload: dict) -> dict | None:
    """Per-launch PMC averages of a kernel from the committed profile, only if it was taken on this workload."""
    if not counters or counters.get("workload") != workload:
        return None
    for name, rec in counters.get("kernels", {}).items():
        if kernel_prefix in name:
            return rec
    return None


def valu_mix_peak(ceil: dict, frac_complex: float) -> float | None:
    """Ceiling (wave-instructions/s) of an instruction stream with the given share of complex-class instructions."""
    if not ceil.get("valu_simple"):
        return None
    return 1.0 / ((1.0 - frac_complex) / ceil["valu_simple"] + frac_complex / ceil["valu_complex"])


# --------------------------------------------------------------------------------------------- CPU baseline legs
def _cpu_worker(args):
    path, n_cls, first, count = args
    from oracle import cport  # checker code: cpu_baseline leg only

    z = np.load(path)
    indices, indptr, base = z["indices"], z["indptr"], z["base"]
    gens = [np.random.default_rng(s) for s in np.random.SeedSequence(0).spawn(first + count)][first:]
    cport.lib(native=True)
    t0 = time.perf_counter()
    for g in gens:
        shuffled = base.copy()
        g.shuffle(shuffled)
        cport.nenrich(indices, indptr, shuffled, n_cls, parallel=False, native=True).astype(np.float64)
    return time.perf_counter() - t0


def _cpu_baseline_all_cores(indices, indptr, base, n_cls: int, per_worker: int) -> dict:
    """One single-threaded worker *process* per host core this process may run on (plain subprocesses, hard timeout)."""
    import subprocess
    import tempfile

    workers = len(os.sched_getaffinity(0))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "graph.npz")
        np.savez(path, indices=indices, indptr=indptr, base=base)
        t0 = time.perf_counter()
        procs = [
            subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", path, str(n_cls), str(w * per_worker), str(per_worker)],
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
            for w in range(workers)
        ]
        busy = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=180)
                busy.append(float(o.strip().splitlines()[-1]))
            except Exception:
                p.kill()
        wall = time.perf_counter() - t0
    if len(busy) != workers:
        return {"error": f"{workers - len(busy)} of {workers} workers failed"}
    # throughput while all cores are busy: workers run concurrently, each reports the time of its own loop
    return {"value": workers * per_worker / max(busy), "unit": "permutations/s", "cores": workers,
            "mode": "n_jobs=-1 analogue: one single-threaded worker process per core (len(os.sched_getaffinity(0))), contiguous permutation chunks",
            "sample": f"{workers * per_worker} permutations, slowest worker loop {max(busy):.1f} s (wall incl. process start-up {wall:.1f} s)"}


def cpu_baseline(adj, labels: np.ndarray, budget_s: float = 12.0) -> dict:
    """Squidpy's default CPU path (n_jobs=None, numba_parallel=False: ONE core) on a bounded sample of the same
    workload: per permutation `shuffled = int_clust.copy(); rng.shuffle(shuffled); _nenrich(...)`
    (gr/_nhood.py:530-539), numba kernel restated in C (oracle/c/sqgr_cpu.c) because numba is absent."""
    from oracle import cport  # checker code: cpu_baseline leg only
    from squidpy_amd._synthetic import hex_grid_graph

    cport.lib(native=True)
    indices, indptr = adj.indices.astype(np.uint32), adj.indptr.astype(np.uint32)
    base = labels.astype(np.uint32)
    gens = [np.random.default_rng(s) for s in np.random.SeedSequence(0).spawn(4096)]
    t0 = time.perf_counter()
    done = 0
    while done < len(gens):
        shuffled = base.copy()
        gens[done].shuffle(shuffled)
        cport.nenrich(indices, indptr, shuffled, N_CLS, parallel=False, native=True).astype(np.float64)
        done += 1
        if time.perf_counter() - t0 > budget_s and done >= 5:
            break
    dt = time.perf_counter() - t0
    out = {
        "value": done / dt,
        "unit": "permutations/s",
        "cores": 1,
        "kind": "port",
        "sample": f"{done} permutations of the same {len(base)}-spot x {N_CLS}-cluster workload (numpy PCG64 shuffle + C restatement "
        f"of the numba kernel incl. its res[N,K] scratch), {dt:.1f} s on 1 core = Squidpy's default n_jobs=None",
    }
    # all host cores: Squidpy's n_jobs=-1 (joblib process fan-out, contiguous permutation chunks per worker,
    # _utils.py:223-231), each worker single-threaded like `_callback_wrapper` forces numba to be
    try:
        out["all_cores"] = _cpu_baseline_all_cores(indices, indptr, base, N_CLS, per_worker=4)
    except Exception as exc:  # pragma: no cover
        out["all_cores"] = {"error": repr(exc)}
    # BASELINE config 1 (the reference's own CPU-runnable case) in FULL: 5 000-spot hex grid, 10 clusters, n_perms = 1000
    try:
        g1 = hex_grid_graph(50, 100)
        lab1 = np.random.default_rng(0).integers(0, 10, g1.shape[0]).astype(np.uint32)
        i1, p1 = g1.indices.astype(np.uint32), g1.indptr.astype(np.uint32)
        gens1 = [np.random.default_rng(s) for s in np.random.SeedSequence(0).spawn(1000)]
        t1 = time.perf_counter()
        for r in gens1:
            sh = lab1.copy()
            r.shuffle(sh)
            cport.nenrich(i1, p1, sh, 10, parallel=False, native=True).astype(np.float64)
        d1 = time.perf_counter() - t1
        out["config1_full"] = {"value": 1000 / d1, "unit": "permutations/s", "cores": 1, "seconds": d1,
                               "sample": "config 1 in full: 5 000-spot hex grid x 10 clusters x 1000 permutations, 1 core"}
    except Exception as exc:  # pragma: no cover
        out["config1_full"] = {"error": repr(exc)}
    return out


# --------------------------------------------------------------------------------------------- Moran's I leg
def gather_roofline(kernels: dict, counters: dict, n: int, G: int, P: int, steps: int, b_gene: int) -> dict:
    """Roofline entry of the gather kernel (k_perm_dot): fabric-bound 512-byte row gathers."""
    cnt, ms = kernels.get("autocorr_perm_dot_moran", (0, 0.0))
    gather_bps = (b_gene * G * steps / (ms * 1e-3)) if ms > 0 else None
    avg_ms = ms / max(cnt, 1)
    pmc = kernel_counters(counters.get("moran", {}), "k_perm_dot<", {"spots": n, "genes": G, "perms": P})
    roof = {
        "kernel": "autocorr_perm_dot_moran",
        "bound": "hbm",
        "achieved": None,
        "peak": HBM_PEAK / 1e9,
        "unit": "GB/s",
        "frac": None,
        "traffic": None,
        "launches": cnt,
        "avg_launch_ms": avg_ms,
        "algorithmic_bytes_per_gene": b_gene,
        "workload_key": {"spots": n, "genes": G, "perms": P},
        "algorithmic_GBps": gather_bps / 1e9 if gather_bps else None,
        "note": "`achieved` = MEASURED memory-side traffic of the gather kernel (PMC FETCH_SIZE doubled per MI355X_MICROARCH.md §HBM + WRITE_SIZE, "
        "per launch) / its HIP-event time — the 51 MB working set of the [spot][64 genes] tiles in flight misses the 4 MB L2s (TCC hit rate "
        "below) and streams from the Infinity Cache / HBM as 512-byte rows, so the fabric is the bound.  SURVEY §8d's algorithmic bytes "
        "(one float64 pass over a gene's N values per evaluation) exceed the traffic by `algorithmic_reuse` (the L2 hits)",
    }
    if pmc and avg_ms > 0:
        fetch, write = pmc.get("FETCH_SIZE_bytes"), pmc.get("WRITE_SIZE_bytes")
        if fetch is not None and write is not None:
            roof["traffic"] = 2.0 * fetch + write
            roof["traffic_source"] = counters.get("_source")
            roof["achieved"] = roof["traffic"] / (avg_ms * 1e-3) / 1e9
            roof["frac"] = roof["achieved"] * 1e9 / HBM_PEAK
            roof["algorithmic_reuse"] = b_gene * G / roof["traffic"]
        if pmc.get("TCC_HIT_sum") is not None and pmc.get("TCC_MISS_sum") is not None:
            roof["l2_hit_rate"] = pmc["TCC_HIT_sum"] / max(pmc["TCC_HIT_sum"] + pmc["TCC_MISS_sum"], 1.0)
    if roof["achieved"] is None and gather_bps:  # no matching PMC file: price the algorithmic gather bytes against the aggregate L2 bandwidth
        roof.update({"bound": "l2_gather", "achieved": gather_bps / 1e9, "peak": L2_PEAK / 1e9, "frac": gather_bps / L2_PEAK})
    return roof


def alloc_delta(a: dict, b: dict) -> dict:
    """What the library asked of the HIP allocator between two `Context.alloc_counters()` readings."""
    return {"hipMalloc_calls": b["mallocs"] - a["mallocs"], "hipMalloc_MB": round((b["malloc_bytes"] - a["malloc_bytes"]) / 1e6, 1),
            "hipMalloc_ms": round((b["malloc_ns"] - a["malloc_ns"]) / 1e6, 3), "hipFree_calls": b["frees"] - a["frees"],
            "hipFree_ms": round((b["free_ns"] - a["free_ns"]) / 1e6, 3), "pool_hits": b["pool_hits"] - a["pool_hits"]}


GRAPH_KINDS = {
    "knn6": "directed 6-nearest-neighbour graph of the jittered lattice (KNNBuilder logic, SURVEY §8d), row-normalised: one row sum",
    "hex": "hex-grid graph (degrees 2-6), row-normalised float32 weights: one row sum per degree",
    "general": "hex-grid graph with float64 weights uniform(0.5, 1.5), transformation=False: every row sum different",
}


def autocorr_graph(ctx, kind: str, rows: int, cols: int):
    """The scipy CSR graph of an autocorr leg (GRAPH_KINDS)."""
    from sklearn.preprocessing import normalize

    from squidpy_amd._synthetic import hex_grid, hex_grid_graph, knn_directed_graph

    if kind == "knn6":
        xy = hex_grid(rows, cols) + np.random.default_rng(5).normal(0.0, 1.0, (rows * cols, 2))
        return normalize(knn_directed_graph(xy, 6, ctx), norm="l1", axis=1)
    g = hex_grid_graph(rows, cols)
    if kind == "hex":
        return normalize(g, norm="l1", axis=1)
    g = g.astype(np.float64)
    g.data = np.random.default_rng(9).uniform(0.5, 1.5, g.nnz)
    return g


def autocorr_leg(ctx, mode: str, world: int, fence, reduce_max, steps: int, with_cpu: bool, counters: dict, graph_kind: str = "knn6") -> dict:
    """Second half of BASELINE.json's metric: Moran's I (``mode="moran"``; ``"geary"``: Geary's C) genes/sec on the C3 shape
    (1e5 spots, n_perms=1000) on the graph `graph_kind` names (GRAPH_KINDS; the headline of the leg runs SURVEY §8d's directed
    kNN-6 graph); one step = observed score + 1000 permuted scores for a resident block of 2048 genes per GPU, the p-value
    reductions formed on the device (``sqgr_autocorr_perm_stats``)."""
    from squidpy_amd import _lib

    rows, cols, G, P = 250, 400, 2048, 1000
    n = rows * cols
    rank = int(os.environ.get("RANK", "0"))
    g = autocorr_graph(ctx, graph_kind, rows, cols)
    vals = np.random.default_rng(1 + rank).gamma(2.0, 1.0, size=(G, n))
    graph = _lib.Graph(ctx, g, with_data=True)
    plan = _lib.AutocorrPlan(ctx, graph, vals)  # resident from here on
    # warm-up = the TIMED path, once: observed scores + P permutations through the kernel P selects + the device reductions, on a
    # permutation range of its own — every workspace of that path (pair layout, bucket lists, partials, score block) exists before
    # the clock starts.  (Round 5 warmed up with 32 permutations — another kernel — and the first of 3 timed steps paid ~20 GB of
    # first-use hipMalloc: 0.5 ms on the builder's boxes, ~130 ms on the driver's, VERDICT r5 weak #3.)  Its cost is reported.
    a0 = ctx.alloc_counters()
    t0 = time.perf_counter()
    score = plan.scores(mode)
    plan.perm_stats(mode, score, seed=7, perm_begin=steps * P, perm_end=(steps + 1) * P)
    fence()
    first_call_ms = (time.perf_counter() - t0) * 1e3
    a1 = ctx.alloc_counters()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    for i in range(steps):
        score = plan.scores(mode)
        red = plan.perm_stats(mode, score, seed=7, perm_begin=i * P, perm_end=(i + 1) * P)
    fence()
    elapsed = reduce_max(time.perf_counter() - t0)
    kernels = ctx.timer_report()
    ctx.timer_enable(False)
    a2 = ctx.alloc_counters()
    assert np.isfinite(score).all() and np.isfinite(red["std"]).all() and (red["n_ge"] <= P).all()
    wall_ms = elapsed / steps * 1e3
    kernel_sum_ms = sum(v[1] for v in kernels.values()) / steps   # HIP events around every launch of the leg, on the library's stream
    kname = f"autocorr_perm_dot_lds_{mode}"
    lds_cnt, lds_ms = kernels.get(kname, (0, 0.0))
    geary = mode == "geary"
    b_gene = (P + 1) * 8 * n
    # LDS bytes per (spot, permutation, gene): the 16-byte z and y rows of a gene PAIR (8 + 8 per gene); Geary's C adds one 8-byte read of
    # r[idx] — or of its class table — per pair of genes (4 per gene)
    per = 16.0
    if geary:
        rs_vals, rs_counts = np.unique(np.asarray(g.astype(np.float64).sum(axis=1)).ravel(), return_counts=True)
        others = 1.0 - rs_counts.max() / n
        if rs_vals.size == 1:
            per = 16.0  # one row sum: a constant term, Moran's kernel
        elif rs_vals.size <= 8 and others <= 0.25:
            per = 16.0 + 12.0 * others  # the spots with another row sum than most: a 16-byte z row + the 8-byte table per gene pair
        else:
            per = 20.0
    if lds_cnt:  # the LDS-bucketed kernel (n_perms >= 512): both operands of every z*y product are read from LDS
        avg_ms = lds_ms / lds_cnt
        lds_bytes = per * n * P * G
        achieved = lds_bytes * lds_cnt / (lds_ms * 1e-3)
        ceil = load_lds_read_ceilings()
        roof = {
            "kernel": kname,
            "bound": "lds_read",
            "achieved": achieved / 1e9,
            "peak": LDS_READ_PEAK / 1e9,
            "unit": "GB/s",
            "frac": achieved / LDS_READ_PEAK,
            "traffic": None,
            "launches": lds_cnt,
            "avg_launch_ms": avg_ms,
            "workload_key": {"spots": n, "genes": G, "perms": P},
            "algorithmic_bytes_per_gene": b_gene,
            "algorithmic_GBps": b_gene * G * lds_cnt / (lds_ms * 1e-3) / 1e9,
            "list_build_ms_per_launch": kernels.get("autocorr_bucket_lists", (0, 0.0))[1] / max(lds_cnt, 1),
            "perm_stats_ms_per_launch": kernels.get("autocorr_perm_stats", (0, 0.0))[1] / max(lds_cnt, 1),
            "note": "spots are cut into chunks, the pairs (i, idx_p(i)) of every permutation are bucketed by (chunk of i, chunk of idx_p(i)) once "
            "per gene block; a workgroup keeps Z[chunk a] and Y[chunk b] of two genes in LDS and every lane walks the list of its own "
            "permutation: two ds_read_b128 per pair, no global gather (Geary's C: + one ds_read_b64 of the row sum or its class table — or, "
            "when one row sum holds on 3 spots in 4, a constant + short exception lists).  `achieved` = "
            f"{per:.2f} B x spots x permutations x genes / time (padding pairs not counted) against the LDS read peak of the guide (256 B/clk/CU).  "
            "Random 16-byte rows conflict ~3-way inside a 16-lane service group; the lists are scheduled so that the 16 lanes of a group read "
            "different row classes on both sides where the pairs allow it (k_bucket_order_steps): `frac_of_pattern_ceiling` prices the kernel "
            "against the measured rate of random rows with 16 classes per group — what a perfect schedule would reach —, `random_pattern_GBps` "
            "is the unscheduled rate (tools/ubench_lds_read.hip).  HBM side: lists + chunks, `traffic` from PMC when the committed profile matches",
        }
        pattern = ceil.get("scheduled_b128_bytes_per_s") or ceil.get("random_b128_bytes_per_s")
        if pattern:
            roof["pattern_ceiling_GBps"] = pattern / 1e9
            roof["frac_of_pattern_ceiling"] = achieved / pattern
            roof["random_pattern_GBps"] = ceil["random_b128_bytes_per_s"] / 1e9 if ceil.get("random_b128_bytes_per_s") else None
            roof["ceiling_source"] = ceil["source"]
        pmc = kernel_counters(counters.get(mode, {}), "k_perm_dot_lds<", {"spots": n, "genes": G, "perms": P})
        if pmc and pmc.get("FETCH_SIZE_bytes") is not None and pmc.get("WRITE_SIZE_bytes") is not None:
            roof["traffic"] = 2.0 * pmc["FETCH_SIZE_bytes"] + pmc["WRITE_SIZE_bytes"]
            roof["traffic_source"] = counters.get("_source")
            roof["hbm_GBps"] = roof["traffic"] / (avg_ms * 1e-3) / 1e9
            roof["hbm_frac_of_peak"] = roof["hbm_GBps"] * 1e9 / HBM_PEAK
            if pmc.get("TCC_HIT_sum") is not None and pmc.get("TCC_MISS_sum") is not None:
                roof["l2_hit_rate"] = pmc["TCC_HIT_sum"] / max(pmc["TCC_HIT_sum"] + pmc["TCC_MISS_sum"], 1.0)
            if pmc.get("SQ_LDS_BANK_CONFLICT") is not None and pmc.get("SQ_LDS_IDX_ACTIVE"):
                roof["lds_conflict_cycle_share"] = pmc["SQ_LDS_BANK_CONFLICT"] / pmc["SQ_LDS_IDX_ACTIVE"]
    else:
        roof = gather_roofline(kernels, counters, n, G, P, steps, b_gene)
    stat = "Geary's C" if geary else "Moran's I"
    out = {
        "metric": f"{stat} genes/sec (1e5 spots, {graph_kind} graph, {G} genes/step, n_perms=1000)",
        "graph": GRAPH_KINDS[graph_kind], "genes_per_step": G,
        "value": steps * G * world / elapsed,
        "unit": "genes/s",
        "ms_per_step": wall_ms,
        "steps": steps,
        # the clock the value is computed from (host perf_counter, fenced) against the sum of the HIP-event times of every kernel of
        # the same steps: what is neither is allocation, copies, synchronisation or host code — above 1.1 the leg is marked FAILED
        "wall_ms_per_step": wall_ms, "kernel_sum_ms_per_step": kernel_sum_ms, "wall_over_kernels": wall_ms / kernel_sum_ms if kernel_sum_ms > 0 else None,
        "timed_region_alloc": alloc_delta(a1, a2),
        "first_call": {"ms": first_call_ms, "alloc": alloc_delta(a0, a1),
                       "note": "the warm-up call = the first scores + perm_stats of a fresh plan at the timed size: what a user's first call pays"},
        "dtype": "f64",
        "config": {"workload": f"spatial_autocorr {mode}: {n} spots, {GRAPH_KINDS[graph_kind]}; {G} genes resident per GPU and step, {P} permutations, "
                               "device permutations, p-value reductions on the device (G x 4 numbers leave the GPU per step)"},
        "kernel_time_share": {k: round(v[1] / max(sum(x[1] for x in kernels.values()), 1e-9), 3) for k, v in kernels.items() if v[0] > 0},
        "roofline": roof,
    }
    if with_cpu:
        from oracle import cport  # checker code: cpu_baseline leg only

        gsub, evals = 64, 0
        gens = [np.random.default_rng(s) for s in np.random.SeedSequence(0).spawn(64)]
        g64 = g.astype(np.float64)
        func = cport.gearys_c if geary else cport.morans_i
        t0 = time.perf_counter()
        while evals < len(gens):
            idx = gens[evals].permutation(n)
            func(g64[idx, :], vals[:gsub], parallel=False, native=True)  # gr/_ppatterns.py:271-272
            evals += 1
            if time.perf_counter() - t0 > (3.0 if geary else 6.0) and evals >= 2:
                break
        per_eval_gene = (time.perf_counter() - t0) / (evals * gsub)
        out["cpu_baseline"] = {
            "value": 1.0 / ((P + 1) * per_eval_gene),
            "unit": "genes/s",
            "cores": 1,
            "kind": "port",
            "sample": f"{evals} permutations x {gsub} genes (scipy row permutation g[idx,:] + C restatement of scanpy's per-gene "
            f"{stat} loop), scaled to {P + 1} evaluations per gene",
        }
    plan.close()
    graph.close()
    if kernel_sum_ms > 0 and wall_ms > 1.1 * kernel_sum_ms:
        out["FAILED"] = (f"wall {wall_ms:.2f} ms per step > 1.1 x the kernels' {kernel_sum_ms:.2f} ms: the value is NOT a kernel throughput "
                         f"(allocator in the timed region: {out['timed_region_alloc']})")
        print(f"bench.py: autocorr leg {mode}/{graph_kind} FAILED its wall-vs-kernels check: {out['FAILED']}", file=sys.stderr, flush=True)
    return out


def moran_p100_leg(ctx, cpu_value: float | None) -> dict:
    """Moran's I on the config-3 shape with the reference's EVERYDAY number of permutations (`n_perms=100`; its docs and tests use
    50-100, tests/graph/test_ppatterns.py): the LDS-bucketed kernel on 8 virtual permutations per permutation (what the library
    picks below 512 permutations), and — forced through `SQGR_AUTOCORR_KERNEL=gather` — the round-1 gather kernel it replaces there."""
    from squidpy_amd import _lib

    rows, cols, G, P, steps = 250, 400, 2048, 100, 5
    n = rows * cols
    g = autocorr_graph(ctx, "knn6", rows, cols)
    vals = np.random.default_rng(11).gamma(2.0, 1.0, size=(G, n))
    graph = _lib.Graph(ctx, g, with_data=True)
    plan = _lib.AutocorrPlan(ctx, graph, vals)
    out, saved = {}, os.environ.get("SQGR_AUTOCORR_KERNEL")
    try:
        for label, env in (("default", None), ("gather", "gather")):
            if env is None:
                os.environ.pop("SQGR_AUTOCORR_KERNEL", None)
            else:
                os.environ["SQGR_AUTOCORR_KERNEL"] = env
            score = plan.scores("moran")
            plan.perm_stats("moran", score, seed=3, perm_begin=0, perm_end=P)  # warm-up: workspaces of this kernel
            ctx.sync()
            ctx.timer_enable(True)
            ctx.timer_reset()
            t0 = time.perf_counter()
            for i in range(steps):
                score = plan.scores("moran")
                red = plan.perm_stats("moran", score, seed=7, perm_begin=(i + 1) * P, perm_end=(i + 2) * P)
            ctx.sync()
            dt = time.perf_counter() - t0
            out[label] = {"genes_per_s": steps * G / dt, "ms_per_step": dt / steps * 1e3, "kernels": ctx.timer_report()}
            ctx.timer_enable(False)
            assert np.isfinite(red["std"]).all()
    finally:
        if saved is None:
            os.environ.pop("SQGR_AUTOCORR_KERNEL", None)
        else:
            os.environ["SQGR_AUTOCORR_KERNEL"] = saved
    plan.close()
    graph.close()
    k = out["default"]["kernels"]
    kname = next((name for name, v in k.items() if name.startswith("autocorr_perm_dot_lds") and v[0] > 0), None)  # (timers of earlier legs report 0 launches)
    cnt, ms = k.get(kname, (0, 0.0)) if kname else (0, 0.0)
    lds_bytes = 16.0 * n * P * G
    achieved = lds_bytes * cnt / (ms * 1e-3) if ms > 0 else None
    return {
        "metric": "Moran's I genes/sec (1e5 spots, knn6 graph, 2048 genes/step, n_perms=100)", "value": out["default"]["genes_per_s"], "unit": "genes/s",
        "ms_per_step": out["default"]["ms_per_step"], "gather_kernel_genes_per_s": out["gather"]["genes_per_s"],
        "speedup_vs_gather_kernel": out["default"]["genes_per_s"] / out["gather"]["genes_per_s"],
        "kernel_ms_per_step": {name: round(v[1] / steps, 3) for name, v in k.items() if v[0] > 0},
        "gather_kernel_ms_per_step": {name: round(v[1] / steps, 3) for name, v in out["gather"]["kernels"].items() if v[0] > 0},
        "roofline": {"kernel": kname, "bound": "lds_read", "achieved": achieved / 1e9 if achieved else None, "peak": LDS_READ_PEAK / 1e9, "unit": "GB/s",
                     "frac": achieved / LDS_READ_PEAK if achieved else None, "traffic": None,
                     "note": "16 B of LDS reads per (spot, permutation, gene), padding pairs not counted; the 8 sub-lists of a permutation are ~31 pairs long per "
                     "bucket and padded to the longest of 64 lanes (+50 %): the fraction is that much below the n_perms = 1000 kernel's"},
        "cpu_baseline": {"value": cpu_value * 1001.0 / 101.0, "unit": "genes/s", "cores": 1, "kind": "port",
                         "sample": "the secondary leg's CPU rate per (gene, evaluation), scaled to 101 evaluations per gene"} if cpu_value else None,
    }


def config3_full_leg(with_cpu_value: float | None) -> dict:
    """BASELINE config 3 IN FULL through the front end: `spatial_autocorr` on 1e5 spots x 20 000 genes (16 GB of float64
    expression handed over as a host array), 1000 permutations, both statistics — upload, graph normalisation, p-values, FDR
    and the sorted frame included; what README quotes as "config 3 end to end"."""
    import warnings

    import pandas as pd

    import squidpy_amd as sq
    from squidpy_amd._synthetic import hex_grid_graph

    from squidpy_amd import _lib

    actx = _lib.default_context()
    rows, cols, G, P = 250, 400, 20_000, 1000
    n = rows * cols
    t0 = time.perf_counter()
    base = np.random.default_rng(3).gamma(2.0, 1.0, size=(n, 2000))
    X = np.empty((n, G), dtype=np.float64)
    for j in range(G // 2000):  # ten shifted copies of a 2000-gene block: cheap to build, no two columns equal
        np.add(base, 0.01 * j, out=X[:, j * 2000 : (j + 1) * 2000])
    del base
    adata = sq.AnnDataLite(X=X, obs=pd.DataFrame(index=[f"s{i}" for i in range(n)]), obsp={"spatial_connectivities": hex_grid_graph(rows, cols)})
    build_s = time.perf_counter() - t0
    out = {"metric": "spatial_autocorr end to end, BASELINE config 3 in full (1e5 spots x 20 000 genes, n_perms=1000)", "unit": "s",
           "input": "dense float64 host array (16 GB), uploaded once inside the call", "synthetic_input_build_s": build_s}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sq.gr.spatial_autocorr(adata, genes=list(adata.var_names[:256]), mode="moran", n_perms=64, seed=1, copy=True)  # warm-up (module load)
        for mode in ("moran", "geary"):
            runs, allocs = [], []
            for _ in range(2):  # two whole calls, both listed (the second call of a process used to stall ~5 s in hipMalloc once
                a0 = actx.alloc_counters()
                t0 = time.perf_counter()  # the driver had handed out all of the HBM once; buffers are parked and reused now)
                df = sq.gr.spatial_autocorr(adata, mode=mode, n_perms=P, seed=1, copy=True)
                runs.append(time.perf_counter() - t0)
                allocs.append(alloc_delta(a0, actx.alloc_counters()))
                assert df.shape == (G, 9) and np.isfinite(df.iloc[:, 0]).all()
            out[mode] = {"seconds": min(runs), "genes_per_s": G / min(runs), "runs_s": runs, "alloc_per_run": allocs}
    # The same configuration with the expression matrix RESIDENT in HBM when the clock starts (the contract's rule for `value`; the
    # end-to-end figure above is PCIe-bound: 16 GB cross the bus inside the call): BASELINE's config 3 as it is quoted — 20 000 genes,
    # ONE set of 1000 permutations — on the secondary leg's directed kNN-6 graph: ten feature blocks of 2048 genes cut out of the
    # resident matrix on the device, observed scores + permutation scores + the p-value reductions per block; the bucket lists of the
    # permutations are built once and shared by the blocks, as in every real call (the secondary leg's step is ONE block and builds
    # them per step).
    try:
        g3 = autocorr_graph(actx, "knn6", rows, cols)
        graph3 = _lib.Graph(actx, g3, with_data=True)
        dm = _lib.DeviceMatrix(actx, X)  # uploaded here, outside the timed region
        blocks = [(b0, min(G, b0 + 2048)) for b0 in range(0, G, 2048)]

        def one_call(seed: int) -> float:
            t0 = time.perf_counter()
            for b0, b1 in blocks:
                plan = _lib.AutocorrPlan.from_columns(actx, graph3, dm, b0, b1 - b0)
                try:
                    sc = plan.scores("moran")
                    red = plan.perm_stats("moran", sc, seed=seed, perm_begin=0, perm_end=P)
                finally:
                    plan.close()
            actx.sync()
            assert np.isfinite(sc).all() and (red["n_ge"] <= P).all()
            return time.perf_counter() - t0

        one_call(11)  # warm-up = the timed path
        actx.timer_enable(True)
        actx.timer_reset()
        a0 = actx.alloc_counters()
        runs = [one_call(12 + r) for r in range(2)]  # a new seed per run: the lists are built again, once per run
        rep = actx.timer_report()
        actx.timer_enable(False)
        out["moran_resident"] = {"metric": "Moran's I genes/sec, BASELINE config 3 with the matrix resident in HBM (1e5 spots x 20 000 genes in 10 blocks, "
                                 "n_perms=1000, directed kNN-6 graph; the permutations' bucket lists built once per call)",
                                 "value": G / min(runs), "unit": "genes/s", "seconds": min(runs), "runs_s": runs,
                                 "list_builds_per_call": rep.get("autocorr_bucket_lists", (0, 0.0))[0] / len(runs),
                                 "kernel_sum_s_per_call": sum(v[1] for v in rep.values()) / len(runs) * 1e-3,
                                 "kernels_ms_per_call": {k_: round(v[1] / len(runs), 2) for k_, v in sorted(rep.items(), key=lambda kv: -kv[1][1]) if v[0]},
                                 "alloc": alloc_delta(a0, actx.alloc_counters())}
        dm.close()
        graph3.close()
    except Exception as exc:  # pragma: no cover  (never at the cost of the leg above)
        out["moran_resident"] = {"error": repr(exc)}
    if with_cpu_value:
        out["cpu_baseline"] = {"value": G / with_cpu_value, "unit": "s", "cores": 1, "kind": "port",
                               "sample": "config 3 (Moran) at the per-gene rate of the secondary leg's CPU baseline (C restatement, 1 core): 20 000 genes / that rate"}
    return out


# --------------------------------------------------------------------------------------------- config-4 legs
def config4_legs(ctx, ceil: dict, with_cpu: bool, counters: dict, short_radii: bool = True) -> dict:
    """co_occurrence, Ripley L and Ripley G on BASELINE config 4's shape: 1e6 points (hex grid + N(0,5) jitter), 30 clusters,
    50 interval edges (49 thresholds) / 50 Ripley radii.  Unit of work = one ORDERED pair evaluation.  Neither HBM
    nor MFMA bounds these kernels: the pair kernels are VALU-issue bound, priced against the measured issue rate of their own
    instruction mix — the mix per 64 unordered pairs is read off the hot loop's ISA (tools/isa_mix.py) and, when the committed
    profile matches, cross-checked by the PMC instruction counts of the same launch."""
    from squidpy_amd import _lib
    from squidpy_amd._synthetic import hex_grid
    from squidpy_amd.gr._ppatterns import _find_min_max

    n = ROWS * COLS
    rng = np.random.default_rng(0)
    xy = hex_grid(ROWS, COLS) + rng.normal(0, 5, (n, 2))
    labels = rng.integers(0, N_CLS, n).astype(np.int32)
    out = {}
    wkey = {"points": n, "clusters": N_CLS}
    # ---- co_occurrence (gr/_ppatterns.py:283-310): float32 coordinates, 49 squared thresholds
    sp = xy.astype(np.float32)
    lo, hi = _find_min_max(sp)
    interval = np.linspace(lo, hi, num=50, dtype=np.float32)
    thr2 = interval[1:] ** 2
    _lib.cooccur_counts(ctx, sp[:4096, 0], sp[:4096, 1], labels[:4096], N_CLS, thr2)  # warm-up (module load, allocations)
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    counts = _lib.cooccur_counts(ctx, sp[:, 0], sp[:, 1], labels, N_CLS, thr2)
    wall = time.perf_counter() - t0
    k = ctx.timer_report()
    ctx.timer_enable(False)
    kms = sum(v[1] for name, v in k.items() if name.startswith("cooccur_pairs"))
    pairs = n * (n - 1)
    assert int(counts[:, :, -1].sum()) <= pairs
    valu_per_pair = 15.0 / 2.0 / 64.0   # wave-instructions per ORDERED pair: 15 VALU per 64 unordered pairs in the hot loop (tools/isa_mix.py)
    peak = valu_mix_peak(ceil, 0.5)
    roof = {"kernel": "cooccur_pairs_fast", "bound": "valu_issue", "achieved": pairs * valu_per_pair / (kms * 1e-3) if kms > 0 else None,
            "peak": peak, "unit": "wave-instr/s", "frac": (pairs * valu_per_pair / (kms * 1e-3) / peak) if kms > 0 and peak else None,
            "traffic": None, "workload_key": wkey, "algorithmic_hbm_bytes": (n / 256.0) * n * 8.0, "isa_mix_per_64_unordered_pairs": {"valu_32": 15, "lds": 3},
            "note": "15 VALU + 3 LDS wave-instructions per 64 unordered pairs (hot loop of k_cooccur_fast<false>, tools/isa_mix.py: 120 VALU + 24 DS per "
            "8 pairs per lane; every unordered pair evaluated once and credited to (a,b) and (b,a)); HBM side negligible: (N/256)*N*8 B of tile re-reads"}
    pmc = kernel_counters(counters.get("legs", {}), "k_cooccur_fast", wkey)
    if pmc and pmc.get("SQ_INSTS_VALU_timed_total") is not None and kms > 0:
        # (totals over the timed launches of the profiled run: its first dispatch is the small warm-up call above)
        vi, li = pmc["SQ_INSTS_VALU_timed_total"], pmc.get("SQ_INSTS_LDS_timed_total") or 0.0
        roof["pmc"] = {"valu_wave_instr": vi, "lds_wave_instr": li, "valu_per_64_unordered_pairs": vi / (pairs / 2 / 64.0), "lds_per_64_unordered_pairs": li / (pairs / 2 / 64.0),
                       "achieved_valu_wave_instr_per_s": vi / (kms * 1e-3), "frac_of_mix_peak": vi / (kms * 1e-3) / peak if peak else None, "source": counters.get("_source")}
        roof["frac"] = roof["pmc"]["frac_of_mix_peak"]
        roof["achieved"] = roof["pmc"]["achieved_valu_wave_instr_per_s"]
        if pmc.get("FETCH_SIZE_bytes_timed_total") is not None and pmc.get("WRITE_SIZE_bytes_timed_total") is not None:
            roof["traffic"] = 2.0 * pmc["FETCH_SIZE_bytes_timed_total"] + pmc["WRITE_SIZE_bytes_timed_total"]
        ds = load_ds_mix("co_occurrence: ds_read_u16 + ds_read2_b32 + ds_add_u32")
        if ds and li > 0:  # the LDS side: DS wave-instructions per second against the rate of exactly this triple (tools/ubench_ds_mix.hip)
            roof["lds_issue"] = {"achieved": li / (kms * 1e-3), "peak": ds["rate"], "unit": "DS wave-instr/s", "frac": min(1.0, li / (kms * 1e-3) / ds["rate"]),
                                 "achieved_over_microbenchmark": li / (kms * 1e-3) / ds["rate"],
                                 "ceiling_source": ds["source"], "note": "table look-up + two thresholds (bank-staggered copies) + histogram add per pair, against the rate the same three DS "
                                 "instructions reach alone in tools/ubench_ds_mix.hip (its best occupancy; the kernel matches it to within the run-to-run clock, "
                                 "`frac` is capped at 1): co-occurrence is LDS-issue bound, with VALU issue (`frac` above) close behind"}
    out["co_occurrence"] = {
        "metric": "co_occurrence ordered pair evaluations/sec (1e6 points x 30 clusters x 49 thresholds)",
        "value": pairs / wall, "unit": "pairs/s", "wall_s": wall, "kernel_ms": kms, "roofline": roof,
    }
    if short_radii:
        # ---- the same cloud with the intervals users pass: 50 edges up to 20 spot spacings — tile pairs beyond the last
        # threshold are skipped (k_co_candidates), the dense sweep of the same thresholds (SQGR_COOCCUR_SPARSE=0) is timed beside it
        short = np.linspace(0.0, 2000.0, num=50, dtype=np.float32)  # (the synthetic hex grid's spot spacing is 100)
        thr2s = short[1:] ** 2
        _lib.cooccur_counts(ctx, sp[:8192, 0], sp[:8192, 1], labels[:8192], N_CLS, thr2s)
        res = {}
        saved = os.environ.get("SQGR_COOCCUR_SPARSE")
        try:
            for route, env in (("near", None), ("dense", "0")):
                if env is None:
                    os.environ.pop("SQGR_COOCCUR_SPARSE", None)
                else:
                    os.environ["SQGR_COOCCUR_SPARSE"] = env
                ctx.sync()
                ctx.timer_enable(True)
                ctx.timer_reset()
                t0 = time.perf_counter()
                c = _lib.cooccur_counts(ctx, sp[:, 0], sp[:, 1], labels, N_CLS, thr2s)
                w = time.perf_counter() - t0
                kk = ctx.timer_report()
                ctx.timer_enable(False)
                res[route] = {"wall_s": w, "kernel_ms": {name: round(v[1], 3) for name, v in kk.items() if name.startswith("cooccur") and v[0] > 0}, "counts": c}
        finally:
            if saved is None:
                os.environ.pop("SQGR_COOCCUR_SPARSE", None)
            else:
                os.environ["SQGR_COOCCUR_SPARSE"] = saved
        same = bool(np.array_equal(res["near"]["counts"], res["dense"]["counts"]))
        near_ms, dense_ms = sum(res["near"]["kernel_ms"].values()), sum(res["dense"]["kernel_ms"].values())
        out["co_occurrence_short_radii"] = {
            "metric": "co_occurrence wall seconds, 1e6 points x 30 clusters, interval = linspace(0, 20 spot spacings, 50)", "unit": "s", "value": res["near"]["wall_s"],
            "kernel_ms": near_ms, "kernels_ms": res["near"]["kernel_ms"], "dense_wall_s": res["dense"]["wall_s"], "dense_kernel_ms": dense_ms,
            "kernel_speedup_vs_dense": dense_ms / near_ms if near_ms > 0 else None, "wall_speedup_vs_dense": res["dense"]["wall_s"] / res["near"]["wall_s"],
            "counts_equal_dense": same, "pairs_counted": int(res["near"]["counts"][:, :, -1].sum()),
            "note": "the wall time includes the host's counting sort (by cluster and Hilbert cell), the upload and the copy-out; `kernel_ms` = candidate lists + sweep",
        }
        assert same, "short-radius co_occurrence differs from the dense sweep"
    # ---- Ripley L (gr/_ripley.py:212-227): float64 pair counts per cluster, 50 radii
    from scipy.spatial import ConvexHull

    hull = ConvexHull(xy[:: max(n // 20000, 1)])
    area = hull.volume
    support = np.linspace(0, (area / 2) ** 0.5, 50)
    by_cluster = [np.ascontiguousarray(xy[labels == c]) for c in range(N_CLS)]
    _lib.pair_counts(ctx, by_cluster[0][:2048], support)
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    all_counts = _lib.pair_counts_batch(ctx, by_cluster, support)  # one launch for the 30 clusters, as `sq.gr.ripley(mode="L")` issues it
    first_counts = all_counts[0]
    wall = time.perf_counter() - t0
    k = ctx.timer_report()
    ctx.timer_enable(False)
    kms = sum(v[1] for name, v in k.items() if name.startswith("ripley_pair_hist"))
    rp = sum(len(p) * (len(p) - 1) for p in by_cluster)
    f64 = load_f64_ceilings()
    # hot loop of k_pair_hist_fast<0> (tools/isa_mix.py): per lane and unordered pair 2 v_add_f64 (dx, dy) + 2 v_mul_f64 + 1 v_add_f64 (d2)
    # + 1 v_mul_f64 (cell) + 1 v_cvt_i32_f64 + 2 v_cmp_f64 = 9 float64 VALU, 6 32-bit VALU, 3 DS (table read, two thresholds in one
    # ds_read2_b64, one ds_add_u32)
    mix = {"v_add_f64": 3, "v_mul_f64": 3, "v_cvt_i32_f64": 1, "v_cmp_le_f64": 2}
    clk = None
    if all(op in f64 for op in mix) and ceil.get("valu_complex") and ceil.get("valu_simple"):
        # issue time of the mix in units of one v_fma_f32 (= the simple class of tools/ubench_ops.hip), then in wave-instructions/s
        fma_units = sum(cnt * f64[op] for op, cnt in mix.items()) + 6 * (ceil["valu_simple"] / valu_mix_peak(ceil, 0.5))
        clk = fma_units * (ctx.device_info().get("cu_count") or 256) * 4 * 2.4e9 / ceil["valu_simple"]  # SIMD clk per 64 unordered pairs at 2.4 GHz
        peak_pairs = ceil["valu_simple"] / fma_units * 64 * 2                                          # ORDERED pairs/s at which the VALU mix saturates
    out["ripley_L"] = {
        "metric": "ripley L ordered pair evaluations/sec (1e6 points in 30 clusters, 50 radii, float64)",
        "value": rp / wall, "unit": "pairs/s", "wall_s": wall, "kernel_ms": kms, "pairs": rp,
        "roofline": {"kernel": "ripley_pair_hist_fast", "bound": "valu_f64_issue",
                     "achieved": rp / (kms * 1e-3) if kms > 0 else None, "peak": peak_pairs if clk else None, "unit": "ordered pairs/s",
                     "frac": (rp / (kms * 1e-3) / peak_pairs) if clk and kms > 0 else None, "traffic": None,
                     "isa_mix_per_64_unordered_pairs": {**mix, "valu_32": 6, "lds": 3}, "simd_clk_per_64_unordered_pairs": clk, "ceiling_source": f64.get("source"),
                     "note": "float64 VALU issue: the hot loop spends 9 float64 instructions per pair (4 clk class) beside 6 32-bit ones; `peak` = pair rate at which "
                     "that mix saturates the four SIMDs of every CU at the issue rates of tools/ubench_f64.hip.  One launch for the 30 clusters "
                     "(sqgr_pair_counts_batch), as the front end issues it"},
    }
    pmc = kernel_counters(counters.get("legs", {}), "k_pair_hist_fast", wkey)
    if pmc and pmc.get("SQ_INSTS_VALU_timed_total") is not None and kms > 0:
        out["ripley_L"]["roofline"]["pmc"] = {
            "valu_wave_instr": pmc["SQ_INSTS_VALU_timed_total"], "lds_wave_instr": pmc.get("SQ_INSTS_LDS_timed_total"),
            "valu_per_64_unordered_pairs": pmc["SQ_INSTS_VALU_timed_total"] / (rp / 2 / 64.0),
            "lds_per_64_unordered_pairs": (pmc.get("SQ_INSTS_LDS_timed_total") or 0.0) / (rp / 2 / 64.0), "source": counters.get("_source"),
            "note": "PMC instruction counts of the timed launch of the profiled run / pairs: the ISA count (15 VALU, 3 DS) plus tile set-up and the diagonal tiles' checked path"}
    # ---- Ripley G (gr/_ripley.py:163-169): for every cluster, the 2 nearest cluster points of every point NOT in it, histogram of the distances
    pts_dev = _lib.DevicePoints(ctx, xy, labels)
    edges = np.linspace(0, (area / 2) ** 0.5, 50)
    pts_dev.knn_hist(by_cluster[0], 2, edges, exclude_label=0)
    ctx.sync()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    gq = 0
    for c in range(N_CLS):
        h = pts_dev.knn_hist(by_cluster[c], 2, edges, exclude_label=c)
        gq += n - len(by_cluster[c])
    wall_g = time.perf_counter() - t0
    kg = ctx.timer_report()
    ctx.timer_enable(False)
    pts_dev.close()
    kms_g = sum(v[1] for name, v in kg.items() if name.startswith("ripley_knn_hist"))
    brute = sum((n - len(p)) * len(p) for p in by_cluster)
    g_roof = {"kernel": "ripley_knn_hist_cells", "bound": "l2_random_access", "achieved": None, "peak": None, "unit": "L2 read requests/s", "frac": None, "traffic": None,
              "queries_per_s_of_kernel_time": gq / (kms_g * 1e-3) if kms_g > 0 else None, "brute_force_distance_evaluations_avoided": brute,
              "note": "one thread per query walks the cells ring by ring around its own (divergent, dependent loads: cell bounds, then ~2 reference points per "
              "cell): what the kernel asks of the machine is random 64-byte requests to L2.  `achieved` = L2 read requests of the 30 timed launches (PMC "
              "TCP_TCC_READ_REQ_sum) / their HIP-event time; `peak` = the rate at which random 16-byte rows out of a 16 MB table arrive "
              f"(tools/ubench_gather.hip).  The brute-force sweep this replaces evaluates {brute:.3g} distances (round 2: 0.60 s at this shape)"}
    gather = load_gather_rate()
    pmc = kernel_counters(counters.get("legs", {}), "k_knn_cells", wkey) or kernel_counters(counters.get("legs", {}), "k_knn_hist", wkey)
    if pmc and pmc.get("TCP_TCC_READ_REQ_sum_timed_total") is not None and kms_g > 0 and gather.get("random_rows_per_s"):
        req = pmc["TCP_TCC_READ_REQ_sum_timed_total"]
        g_roof.update({"achieved": req / (kms_g * 1e-3), "peak": gather["random_rows_per_s"], "frac": req / (kms_g * 1e-3) / gather["random_rows_per_s"],
                       "l2_requests_per_query": req / gq, "l1_accesses_per_query": (pmc.get("TCP_TOTAL_CACHE_ACCESSES_sum_timed_total") or 0.0) / gq,
                       "ceiling_source": gather["source"], "traffic_source": counters.get("_source")})
    out["ripley_G"] = {
        "metric": "ripley G nearest-neighbour queries/sec (1e6 points, 30 clusters, n_neigh=2)",
        "value": gq / wall_g, "unit": "queries/s", "wall_s": wall_g, "kernel_ms": kms_g, "queries": gq,
        "roofline": g_roof,
    }
    if with_cpu:
        from oracle import cport  # checker code: cpu_baseline leg only

        m = 20000
        t0 = time.perf_counter()
        cport.occur_count(sp[:m, 0], sp[:m, 1], thr2, labels[:m], N_CLS, parallel=False, native=True)
        dt = time.perf_counter() - t0
        out["co_occurrence"]["cpu_baseline"] = {"value": m * (m - 1) / dt, "unit": "pairs/s", "cores": 1, "kind": "port",
                                                "sample": f"C restatement of _occur_count on the first {m} points ({dt:.1f} s, 1 core); cost scales with N^2"}
        # Ripley L: the reference's own call (gr/_ripley.py:220-222) — sklearn is installed here, so this is the reference, not a port
        from sklearn.neighbors import KDTree, NearestNeighbors

        t0 = time.perf_counter()
        done, pr = 0, 0
        for pts in by_cluster:
            cnt = KDTree(pts).two_point_correlation(pts, support, dualtree=True) - len(pts)
            if done == 0:
                assert np.array_equal(cnt, first_counts), "sklearn and the device disagree on cluster 0"
            done += 1
            pr += len(pts) * (len(pts) - 1)
            if time.perf_counter() - t0 > 12.0:
                break
        dt = time.perf_counter() - t0
        out["ripley_L"]["cpu_baseline"] = {"value": pr / dt, "unit": "pairs/s", "cores": 1, "kind": "reference",
                                           "sample": f"sklearn KDTree.two_point_correlation(dualtree=True) on {done} of the {N_CLS} clusters at full size ({dt:.1f} s, 1 core; "
                                           "counts of cluster 0 asserted equal to the device's)"}
        t0 = time.perf_counter()
        done, qs = 0, 0
        for c in range(N_CLS):
            nn = NearestNeighbors(n_neighbors=2).fit(by_cluster[c])
            sample = xy[labels != c][:: 8]  # every 8th query point
            nn.kneighbors(sample, n_neighbors=2)
            done += 1
            qs += len(sample)
            if time.perf_counter() - t0 > 8.0:
                break
        dt = time.perf_counter() - t0
        out["ripley_G"]["cpu_baseline"] = {"value": qs / dt, "unit": "queries/s", "cores": 1, "kind": "reference",
                                           "sample": f"sklearn NearestNeighbors(n_neighbors=2).kneighbors on every 8th query point of {done} clusters ({dt:.1f} s, 1 core)"}
    return out


def numpy_stream_leg(ctx, plan, shift, n: int, counters: dict) -> dict:
    """The test with numpy's own PCG64 streams reproduced bit for bit on the GPU (`rng="numpy"` — the mode whose z-scores ARE
    Squidpy's for a seed).  Round 4: the swaps of `Generator.shuffle` are replayed in a cache-friendly order (csrc/sqgr_pcg.hip,
    proof of the order: oracle/pcg_bucket.py): `k_pcg_draws_bucketed2` generates the draws (one wave per permutation, 128 raw
    draws per trip since round 6) into time-ordered lists per (64 K-step phase, 64 KB range), `k_pcg_apply_claims` (one workgroup
    per permutation; round 6: exact position claims in an LDS bitmap, contested records deferred and drained once per list) streams
    window and ranges through LDS in coalesced 64 KB pieces.  Algorithmic traffic per permutation of n bytes: records 2 x 4.3 n,
    ranges ~17 n, rows in and out 2 n — against 128 n + for the one-random-sector-per-swap-side kernel of rounds 1-3."""
    from squidpy_amd._utils import pcg64_states

    res, kern = {}, {}
    for n_exact in (1000, 8192):  # Squidpy's default n_perms, and a throughput-sized batch
        states = pcg64_states(0, n_exact)
        plan.run_pcg64(states, shift)  # warm-up at full size: the workspaces are allocated (and first touched) here
        ctx.timer_enable(True)
        ctx.timer_reset()
        t1 = time.perf_counter()
        plan.run_pcg64(states, shift)
        res[n_exact] = n_exact / (time.perf_counter() - t1)
        kern[n_exact] = ctx.timer_report()
        ctx.timer_enable(False)
    k = kern[8192]
    ms_shuffle = sum(v[1] for name, v in k.items() if "pcg64" in name)
    ms_all = sum(v[1] for v in k.values())
    bucketed = any(name.endswith("_apply") for name in k)
    # algorithmic bytes per permutation of the bucketed replay: 16 phases x 1040 blocks x 256 B of records written and read once,
    # each range r < f read and written once per phase (sum_f f * 64 KB * 2), every window read and written once, the row -> slab pass
    phases = -(-n // 65536)
    alg_bytes = (2.0 * phases * (1024 + phases) * 256 + 2.0 * 65536 * phases * (phases - 1) / 2 + 2.0 * n + 2.0 * n) if bucketed else 2.0 * (n - 1) * 64.0
    roof = {"kernel": "nhood_pcg64_shuffle_draws + _apply (k_pcg_draws_bucketed2, k_pcg_apply_claims)" if bucketed else "nhood_pcg64_shuffle (k_pcg_shuffle_wave)",
            "bound": "hbm", "achieved": 8192 * alg_bytes / (ms_shuffle * 1e-3) / 1e9 if ms_shuffle > 0 else None, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
            "frac": 8192 * alg_bytes / (ms_shuffle * 1e-3) / HBM_PEAK if ms_shuffle > 0 else None, "traffic": None,
            "algorithmic_bytes_per_perm": alg_bytes, "workload_key": {"spots": n, "perms": 8192},
            "swap_steps_per_s": 8192 * (n - 1) / (ms_shuffle * 1e-3) if ms_shuffle > 0 else None,
            "note": "`achieved` = algorithmic bytes of the bucketed replay (records, ranges, windows: all coalesced) / time of the two shuffle kernels; the "
            "measured traffic (`traffic`, `traffic_MB_per_perm`, `traffic_frac`) replaces it when the committed PMC profile matches.  Neither kernel is "
            "HBM-bound yet: the draw generator (one wavefront per permutation) is bound by the latencies of its own instruction stream and lives on "
            "occupancy (4.9 KB of LDS per wavefront; 8 KB more cost the 64-draw kernel 49.7 -> 73.4 ms), the replay by its barrier intervals (two per "
            "chunk of 2048 swaps + ~6 per drain; ablation of round 6: skeleton 23 %, range traffic 15-20 %, claims and swaps 25 %, drains 20 %) — the "
            "ranges' 17 MB per permutation put its HBM floor at ~36 ms per 8192 permutations (54 measured)"}
    names = ("k_pcg_draws_bucketed", "k_pcg_apply_bucketed", "k_pcg_apply_claims", "k_rows_to_slab", "k_pcg_shuffle_wave", "k_rows_to_columns", "k_columns_to_slab")
    cn = counters.get("numpy", {})
    if cn and cn.get("workload") == {"spots": n, "perms": 8192} and ms_shuffle > 0:
        fetch = sum((rec.get("FETCH_SIZE_bytes_timed_total") or 0.0) for name, rec in cn.get("kernels", {}).items() if any(x in name for x in names))
        write = sum((rec.get("WRITE_SIZE_bytes_timed_total") or 0.0) for name, rec in cn.get("kernels", {}).items() if any(x in name for x in names))
        if fetch > 0 or write > 0:
            # totals of the profiled run minus every kernel's first dispatch (the n_perms = 1000 warm-up): 1000 timed + 2 x 8192
            share = 8192.0 / (1000 + 2 * 8192)
            roof["traffic"] = (2.0 * fetch + write) * share
            roof["traffic_source"] = counters.get("_source")
            roof["traffic_MB_per_perm"] = roof["traffic"] / 8192 / 1e6
            roof["traffic_GBps"] = roof["traffic"] / (ms_all * 1e-3) / 1e9
            roof["traffic_frac"] = roof["traffic"] / (ms_all * 1e-3) / HBM_PEAK
    return {
        "value": res[8192], "unit": "permutations/s", "at_n_perms_1000": res[1000],
        "kernel_ms": {name: round(v[1], 3) for name, v in k.items() if v[0] > 0}, "shuffle_share_of_gpu_time": ms_shuffle / ms_all if ms_all > 0 else None,
        "roofline": roof,
        "note": "rng='numpy': z-scores equal Squidpy's for the same seed bit for bit",
    }


# --------------------------------------------------------------------------------------------- the headline's other regimes
def nhood_variant_legs(ctx, adj, graph, n: int, headline_value: float | None, perms: int = 10_000) -> dict:
    """The regimes the headline number does not describe: more than 50 clusters (the LDS pass kernel: 8 | 4 | 1
    permutations per pass at K = 64 | 100 | 200), the directed kNN-6 graph (full edge list: no symmetry to halve) and SURVEY
    §8d's Dirichlet(0.5) cluster sizes (the LDS atomics pile onto few counters) — all at the headline's size (1e6 spots), one step of
    `perms` permutations each.  `roofline` = the count kernel's compulsory DRAM bytes per launch (label slab once, partial
    histograms once, edge list once) / its HIP-event time / 8 TB/s, as for the headline; `vs_k30` = value / headline value."""
    from squidpy_amd import _lib
    from squidpy_amd._synthetic import hex_grid, knn_directed_graph
    from squidpy_amd.gr._nhood import expected_counts

    rng = np.random.default_rng(0)
    legs = {}
    reps = 3

    def run(name: str, g, nnz: int, labels: np.ndarray, K: int, what: str, spot_map: np.ndarray | None = None) -> None:
        plan = _lib.NhoodPlan(ctx, g, labels, K)
        if spot_map is not None:
            plan.set_spot_map(spot_map)
        shift = expected_counts(labels, K, nnz)
        plan.run(3, 0, perms, shift)         # warm-up = the timed call: edge lists, workspaces, every launch shape of it
        ctx.sync()
        a0 = ctx.alloc_counters()
        ctx.timer_enable(True)
        ctx.timer_reset()
        t0 = time.perf_counter()
        for i in range(reps):
            s1, s2, _ = plan.run(3, (i + 1) * perms, (i + 2) * perms, shift)
        ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        kern = {k: (v[0] // reps, v[1] / reps) for k, v in ctx.timer_report().items()}
        ctx.timer_enable(False)
        a1 = ctx.alloc_counters()
        info = plan.info()
        cnt = [(k, v) for k, v in kern.items() if k.startswith("nhood_count") and v[0] > 0]
        launches = sum(v[0] for _, v in cnt)
        ms = sum(v[1] for _, v in cnt)
        per_launch = perms / max(launches, 1)
        avg_ms = ms / max(launches, 1)
        dram = float(n) * per_launch + float(info["blocks_per_batch"]) * info["partial_bytes_per_chunk"] * (per_launch / 16.0) + 8.0 * info["list_edges"]
        legs[name] = {"value": perms / dt, "unit": "permutations/s", "clusters": K, "what": what, "steps": reps,
                      "wall_ms_per_step": dt * 1e3, "kernel_sum_ms_per_step": sum(v[1] for v in kern.values()),
                      "timed_hipMalloc_calls": a1["mallocs"] - a0["mallocs"],
                      "vs_k30": perms / dt / headline_value if headline_value else None,
                      "count_kernel": "+".join(k for k, _ in cnt), "count_us_per_perm": ms * 1e3 / perms, "perms_per_pass": info["perms_per_pass"], "counter_mode": info["counter_mode"], "blocks_per_batch": info["blocks_per_batch"],
                      "list_edges": info["list_edges"], "symmetric_half_list": info["symmetric"], "kernels_ms": {k: round(v[1], 3) for k, v in kern.items() if v[0] > 0},
                      "roofline": {"kernel": "+".join(k for k, _ in cnt), "bound": "hbm", "achieved": dram / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else None,
                                   "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": dram / (avg_ms * 1e-3) / HBM_PEAK if avg_ms > 0 else None, "traffic": dram,
                                   "frac_basis": "compulsory DRAM bytes per launch (slab once + partials once + edge list once) / HIP-event time"}}
        plan.close()

    nnz = int(adj.nnz)
    for K in (64, 100, 200):
        run(f"nhood_K{K}", graph, nnz, rng.integers(0, K, n).astype(np.int32), K, f"hex grid, {K} uniform clusters")
    lab30 = np.random.default_rng(0).integers(0, N_CLS, n).astype(np.int32)
    rows = int(round(np.sqrt(n)))
    if rows * rows == n:
        xy = hex_grid(rows, rows) + np.random.default_rng(1).normal(0.0, 5.0, (n, 2))
        knn = knn_directed_graph(xy, 6, ctx)
        gk = _lib.Graph(ctx, knn, with_data=False)
        run("nhood_knn6_directed", gk, int(knn.nnz), lab30, N_CLS, "directed 6-nearest-neighbour graph of the jittered lattice (split list: its mutual pairs once + its edges without a mirror), 30 uniform clusters")
        gk.close()
    # the headline workload with its observations in RANDOM order (cells of a real table come in no spatial order): as the caller
    # hands it over, and on the renumbered twin rng="philox" builds for it (Z-order curve of the coordinates, on the device) — same
    # moments, bit for bit (tests/test_nhood_gpu.py)
    try:
        import scipy.sparse as sp

        prng = np.random.default_rng(7)
        perm = prng.permutation(n)  # new -> old
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        coo = adj.tocoo()
        shuf = sp.csr_matrix((coo.data, (inv[coo.row], inv[coo.col])), shape=(n, n))
        shuf.sort_indices()
        gs = _lib.Graph(ctx, shuf, with_data=False)
        lab_s = lab30[perm]
        run("nhood_random_order_as_given", gs, nnz, lab_s, N_CLS, "the headline workload, observations in random order, counted as they come")
        t0 = time.perf_counter()
        order = _lib.spatial_order_device(ctx, hex_grid(rows, rows)[perm]) if rows * rows == n else None
        if order is not None:
            twin = gs.renumbered(order)
            ctx.sync()
            twin_ms = (time.perf_counter() - t0) * 1e3
            run("nhood_random_order", twin, nnz, lab_s[order], N_CLS, "the headline workload, observations in random order: the plan on the renumbered twin "
                "of the graph (what rng='philox' does), the generator permuting the caller's observations", spot_map=order)
            legs["nhood_random_order"]["order_and_twin_ms"] = twin_ms
            legs["nhood_random_order"]["as_given"] = legs["nhood_random_order_as_given"]["value"]
        gs.close()
    except Exception as exc:  # pragma: no cover
        legs["nhood_random_order"] = {"error": repr(exc)}
    lab_rng = np.random.default_rng(0)
    skew = lab_rng.choice(N_CLS, size=n, p=lab_rng.dirichlet(np.full(N_CLS, 0.5))).astype(np.int32)
    run("nhood_dirichlet", graph, nnz, skew, N_CLS, "hex grid, 30 clusters with Dirichlet(0.5) proportions")
    # the price of the generator's shortcut: the headline workload with every permutation drawing its OWN 8-round
    # bijection (k_shuffle_indep) instead of one bijection per 16 permutations + a 2-round network each
    saved = os.environ.get("SQGR_SHUFFLE_INDEPENDENT")
    os.environ["SQGR_SHUFFLE_INDEPENDENT"] = "1"
    try:
        run("nhood_independent_bijections", graph, nnz, lab30, N_CLS, "the headline workload, one independent 8-round bijection per permutation "
            "(no group bijection shared by 16 permutations): same count kernel, another label generator")
    finally:
        if saved is None:
            os.environ.pop("SQGR_SHUFFLE_INDEPENDENT", None)
        else:
            os.environ["SQGR_SHUFFLE_INDEPENDENT"] = saved
    ind = legs.get("nhood_independent_bijections")
    if ind:
        ind["shuffle_ms_per_step"] = ind["kernels_ms"].get("nhood_shuffle")
    return legs


# --------------------------------------------------------------------------------------------- the line the driver records
def _sig(x, digits: int = 5):
    """Numbers of the compact line carry `digits` significant figures (the full precision stays in the detail file)."""
    if isinstance(x, bool) or x is None or isinstance(x, (str, int)):
        return x
    try:
        return float(f"{float(x):.{digits}g}")
    except (TypeError, ValueError):
        return None


def _short(text, limit: int = 160):
    text = "" if text is None else str(text)
    return text if len(text) <= limit else text[: limit - 1] + "…"


def _leg(rec: dict | None, *, extra: tuple = ()) -> dict | None:
    """One leg of the compact line: its value, the roofline bound/fraction and the CPU baseline's value — one number each."""
    if not rec:
        return None
    roof = rec.get("roofline") or {}
    out = {"value": _sig(rec.get("value")), "unit": rec.get("unit"), "bound": _short(roof.get("bound"), 32), "frac": _sig(roof.get("frac"), 3),
           "cpu": _sig((rec.get("cpu_baseline") or {}).get("value"), 4)}
    for k in extra:
        if rec.get(k) is not None:
            out[k] = _sig(rec[k], 4)
    if out.get("cpu") is None:
        out.pop("cpu", None)
    return out


def compact_line(detail: dict, detail_path: str | None = None) -> dict:
    """The FINAL stdout line: the contract's keys, the headline `roofline` and `cpu_baseline`, and one number per leg —
    under 4 KB (the driver keeps 8 KB of stdout; round 3's 20 KB line left its record unparsed).  Notes, issue limits,
    PMC inputs and per-kernel tables go to the detail file (`detail_path`)."""
    roof = detail.get("roofline") or {}
    issue = roof.get("issue_limits") or {}
    cfg = detail.get("config") or {}
    line = {k: detail.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                        "vs_baseline", "dtype", "data")}
    line["value"], line["ms_per_step"] = _sig(line["value"], 7), _sig(line["ms_per_step"], 6)
    if detail.get("check"):
        line["check"] = detail["check"]
    line["config"] = {"workload": _short(cfg.get("workload"), 200), "perms_per_step": cfg.get("perms_per_step"),
                      "perms_per_step_per_gpu": cfg.get("perms_per_step_per_gpu"),
                      "collective": _short(cfg.get("collective"), 60), "rccl_world": cfg.get("rccl_world"),
                      "ranks_on_devices": cfg.get("ranks_on_devices")}
    line["roofline"] = {
        "kernel": roof.get("kernel"), "bound": roof.get("bound"), "achieved": _sig(roof.get("achieved")), "peak": _sig(roof.get("peak")),
        "unit": roof.get("unit"), "frac": _sig(roof.get("frac"), 3), "traffic": _sig(roof.get("traffic"), 6),
        "algorithmic_frac": _sig(roof.get("algorithmic_frac"), 3), "fabric_frac": _sig(roof.get("fabric_frac"), 3),
        "frac_basis": "compulsory DRAM bytes of the step's longest kernel / its HIP-event time" if roof.get("frac_basis") else None, "avg_launch_ms": _sig(roof.get("avg_launch_ms")),
        "perms_per_launch": _sig(roof.get("perms_per_launch")), "step_dram_frac": _sig(roof.get("step_dram_frac"), 3),
        "dram_frac_by_kernel": {k: _sig(v, 3) for k, v in (roof.get("dram_frac_by_kernel") or {}).items()},
        "issue_limits": {"l1_gather": _sig(issue.get("frac"), 3) if issue.get("bound") == "l1_gather" else None,
                         "lds_atomic": _sig(((issue.get("lds_atomic") or issue) if issue else {}).get("frac"), 3),
                         "valu": _sig((issue.get("valu") or {}).get("frac"), 3)},
    }
    kern = detail.get("kernels") or {}
    line["kernels"] = {name: {"bound": _short(rec.get("bound"), 24), "frac": _sig(rec.get("frac"), 3), "ms": _sig(rec.get("avg_launch_ms"), 4)}
                       for name, rec in kern.items() if isinstance(rec, dict)}
    cpu = detail.get("cpu_baseline")
    if cpu:
        line["cpu_baseline"] = {"value": _sig(cpu.get("value")), "unit": cpu.get("unit"), "cores": cpu.get("cores"), "kind": cpu.get("kind"),
                                "sample": _short(cpu.get("sample"), 130),
                                "all_cores": {"value": _sig((cpu.get("all_cores") or {}).get("value")), "cores": (cpu.get("all_cores") or {}).get("cores")},
                                "config1_full_perms_per_s": _sig((cpu.get("config1_full") or {}).get("value"))}
        line["speedup_vs_cpu_1core"] = _sig(detail.get("speedup_vs_cpu_1core"))
    sec = detail.get("secondary")
    sec_line = None
    if sec:
        sroof = sec.get("roofline") or {}
        sec_line = {"metric": _short(sec.get("metric"), 64), "value": _sig(sec.get("value")), "unit": sec.get("unit"),
                             "ms_per_step": _sig(sec.get("ms_per_step")), "steps": sec.get("steps"), "wall_ms_per_step": _sig(sec.get("wall_ms_per_step")),
                             "kernel_sum_ms_per_step": _sig(sec.get("kernel_sum_ms_per_step")), "wall_over_kernels": _sig(sec.get("wall_over_kernels"), 4),
                             "timed_hipMalloc_calls": (sec.get("timed_region_alloc") or {}).get("hipMalloc_calls"),
                             "first_call_ms": _sig((sec.get("first_call") or {}).get("ms"), 4),
                             "first_call_hipMalloc_ms": _sig(((sec.get("first_call") or {}).get("alloc") or {}).get("hipMalloc_ms"), 4),
                             "FAILED": _short(sec.get("FAILED"), 100) if sec.get("FAILED") else None, "dtype": sec.get("dtype"),
                             "roofline": {"kernel": sroof.get("kernel"), "bound": sroof.get("bound"), "achieved": _sig(sroof.get("achieved")),
                                          "peak": _sig(sroof.get("peak")), "unit": sroof.get("unit"), "frac": _sig(sroof.get("frac"), 3),
                                          "traffic": _sig(sroof.get("traffic"), 6), "frac_of_pattern_ceiling": _sig(sroof.get("frac_of_pattern_ceiling"), 3)},
                             "cpu_baseline": {k: (_short(v, 48) if k == "sample" else _sig(v)) for k, v in (sec.get("cpu_baseline") or {}).items()
                                              if k in ("value", "unit", "cores", "kind", "sample")}}
    legs = dict(detail.get("legs") or {})
    if "geary_c" not in legs and detail.get("geary_c"):
        legs["geary_c"] = detail["geary_c"]
    out_legs = {}
    cs = legs.get("co_occurrence_short_radii")
    if cs:
        out_legs["co_occurrence_short_radii"] = {"value": _sig(cs.get("value"), 4), "unit": "s", "kernel_ms": _sig(cs.get("kernel_ms"), 4),
                                                 "kernel_speedup_vs_dense": _sig(cs.get("kernel_speedup_vs_dense"), 4),
                                                 "wall_speedup_vs_dense": _sig(cs.get("wall_speedup_vs_dense"), 4), "counts_equal_dense": cs.get("counts_equal_dense")}
    for name in ("co_occurrence", "ripley_L", "ripley_G", "geary_general", "moran_p100", "geary_c"):
        rec = _leg(legs.get(name), extra=("kernel_ms", "speedup_vs_gather_kernel", "wall_ms_per_step", "kernel_sum_ms_per_step", "wall_over_kernels"))
        if rec and (legs.get(name) or {}).get("FAILED"):
            rec["FAILED"] = True
        if rec:
            out_legs[name] = rec
    late = {}  # (the driver's record keeps the LAST 2000 characters of the line verbatim: what the round is judged on goes last)
    for name in ("nhood_random_order", "nhood_knn6_directed", "nhood_dirichlet", "nhood_independent_bijections", "nhood_K64", "nhood_K100", "nhood_K200"):  # permutations/s, HBM fraction, ratio to the headline
        rec = legs.get(name)
        if rec:
            late[name] = {"value": _sig(rec.get("value"), 4), "frac": _sig((rec.get("roofline") or {}).get("frac"), 3), "vs_k30": _sig(rec.get("vs_k30"), 3),
                          "perms_per_pass": rec.get("perms_per_pass"), "counter_mode": rec.get("counter_mode")}
            if rec.get("shuffle_ms_per_step") is not None:
                late[name]["shuffle_ms_per_step"] = _sig(rec["shuffle_ms_per_step"], 4)
            if rec.get("as_given") is not None:  # the same observations counted in the order they came in (no renumbered twin)
                late[name]["as_given"] = _sig(rec["as_given"], 4)
                late[name]["order_and_twin_ms"] = _sig(rec.get("order_and_twin_ms"), 3)
    c3 = legs.get("config3_full")
    if c3:
        out_legs["config3_full"] = {"moran_s": _sig((c3.get("moran") or {}).get("seconds"), 4), "geary_s": _sig((c3.get("geary") or {}).get("seconds"), 4),
                                    "moran_resident_genes_per_s": _sig((c3.get("moran_resident") or {}).get("value"), 4),
                                    "cpu_s": _sig((c3.get("cpu_baseline") or {}).get("value"), 4), "error": c3.get("error")}
    npy = detail.get("numpy_stream_mode")
    if npy:
        nroof = npy.get("roofline") or {}
        out_legs["numpy_stream"] = {"value": _sig(npy.get("value")), "unit": npy.get("unit"), "at_n_perms_1000": _sig(npy.get("at_n_perms_1000")),
                                    "bound": nroof.get("bound"), "frac": _sig(nroof.get("frac"), 3), "traffic_frac": _sig(nroof.get("traffic_frac"), 3),
                                    "traffic_MB_per_perm": _sig(nroof.get("traffic_MB_per_perm"), 4), "cpu": _sig((npy.get("cpu_baseline") or {}).get("value"), 4)}
    emu = detail.get("emulated_ranks")
    if emu:
        line["emulated_ranks"] = {"PROJECTION": "shards run one by one on ONE GPU", "ranks": emu.get("ranks"), "total_perms": emu.get("total_perms"),
                                  "shard_ms": _sig(max(emu.get("shard_seconds") or [0.0]) * 1e3, 4), "whole_ms": _sig((emu.get("one_gpu_seconds") or 0.0) * 1e3, 4)}
    line["pmc_profile"] = _short(detail.get("pmc_profile"), 120)
    line["detail"] = detail_path
    out_legs.update(late)

    def drop_none(obj):  # (legs and the secondary leg only: the contract's own keys keep their nulls)
        return {k: drop_none(v) for k, v in obj.items() if v is not None} if isinstance(obj, dict) else obj

    if out_legs:
        line["legs"] = drop_none(out_legs)
    if sec_line:
        keep = {k: sec_line.get(k) for k in ("roofline", "cpu_baseline")}
        sec_line = drop_none(sec_line)
        sec_line["roofline"] = dict(keep["roofline"], **drop_none(keep["roofline"])) if keep["roofline"] else keep["roofline"]
        line["secondary"] = sec_line

    limits = {"unit": 28, "bound": 24, "kind": 12, "dtype": 40, "data": 16, "scaling": 8}

    def clip(obj, key=None):  # names, units and kernel labels are short by construction; nothing free-form may ever grow the line
        if isinstance(obj, dict):
            return {k: (v if k in ("workload", "sample") and isinstance(v, str) else clip(v, k)) for k, v in obj.items()}
        return _short(obj, limits.get(key, 72)) if isinstance(obj, str) else obj

    return clip(line)



# --------------------------------------------------------------------------------------------- launcher
def launch_ranks(cmd: list[str], n: int, extra_env: dict | None = None, timeout_s: float | None = None) -> int:
    """Start `n` ranks of `cmd` on this node (one process per GPU: RANK = LOCAL_RANK = r, WORLD_SIZE = n, MASTER_ADDR = 127.0.0.1,
    MASTER_PORT = a free port — the same environment ``python -m torch.distributed.run`` exports), wait for all of them and relay
    rank 0's stdout as our own, line by line, so that its LAST line — the compact record — is ours too.  The other ranks' stdout is
    discarded, every rank's stderr is inherited.  Replaces the reference's joblib fan-out (/root/reference/src/squidpy/_utils.py:188-237).
    A rank that fails takes the others down; the return value is the first non-zero exit code (0 when all ranks succeeded)."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), **(extra_env or {}))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL between processes needs dmabuf IPC on this driver
        env.setdefault("NCCL_SOCKET_IFNAME", "lo")           # one node: RCCL's bootstrap over loopback (a box without another interface has none to pick)
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=(r == 0) or None))
    deadline = None if timeout_s is None else time.monotonic() + timeout_s
    import threading

    def relay():
        for line in procs[0].stdout:
            sys.stdout.write(line)
            sys.stdout.flush()

    t = threading.Thread(target=relay, daemon=True)
    t.start()
    rc = 0
    live = set(range(n))
    try:
        while live:
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    print(f"bench.py: rank {r} exited with status {code}; stopping the other ranks", file=sys.stderr)
                    for q in live:
                        procs[q].terminate()
            if deadline is not None and time.monotonic() > deadline and live:
                rc = rc or 124
                print(f"bench.py: ranks {sorted(live)} still running after {timeout_s:.0f} s; stopping them", file=sys.stderr)
                for q in live:
                    procs[q].kill()
                deadline = None
            if live:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        t.join(timeout=10.0)
    return rc


# --------------------------------------------------------------------------------------------- main
def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        print(_cpu_worker((sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--perms-per-step", type=int, default=PERMS_PER_STEP)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--total-perms", type=int, default=100_000, help="--scaling strong: permutations per step over ALL ranks (config 5)")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--cols", type=int, default=COLS)
    ap.add_argument("--label-dist", choices=["uniform", "dirichlet"], default="uniform",
                    help="cluster sizes: uniform (the headline workload) or Dirichlet(0.5) proportions (SURVEY §8d: skewed variant "
                    "that concentrates the LDS-atomic traffic of the count kernel on few counters)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the Moran's I genes/sec leg")
    ap.add_argument("--no-legs", action="store_true", help="skip the co_occurrence / Ripley L legs (config 4)")
    ap.add_argument("--no-numpy-leg", action="store_true", help="skip the bit-compatible numpy-stream leg")
    ap.add_argument("--no-short-radii", action="store_true", help="skip the co_occurrence short-radii leg (tools/profile_round.sh: the PMC totals of "
                    "the co-occurrence kernel then belong to the config-4 sweep alone)")
    ap.add_argument("--no-config3-full", action="store_true", help="skip BASELINE config 3 in full through the front end (builds a 16 GB host matrix)")
    ap.add_argument("--emulate-ranks", type=int, default=8,
                    help="projection for a node this box does not have: run the N rank shards of BASELINE config 5 (--total-perms permutations, strong "
                    "scaling) one after the other on this GPU and print per-shard times; no collective runs, labelled as a projection")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: secondary leg, config-3/4 legs, nhood variants, numpy-stream leg, CPU baselines, "
                    "emulated ranks, and write the detail file (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--detail-out", type=str, default=None,
                    help="where the full record goes (the final stdout line is the compact one: < 4 KB); default with --full: "
                    + os.path.join("bench_out", "bench_detail.json"))
    ap.add_argument("--tune", type=str, default="", help="perms_per_pass,blocks_per_batch,batches_per_launch")
    ap.add_argument("--share-devices", action="store_true",
                    help="allow more ranks than GPUs (rank r on device r mod #GPUs, integer all-reduce through the host side channel): tests on a 1-GPU box")
    args = ap.parse_args()
    if not args.full:  # a plain run: the headline only
        args.no_cpu_baseline = args.no_secondary = args.no_legs = args.no_numpy_leg = True
        args.emulate_ranks = 0
    elif args.detail_out is None:
        args.detail_out = os.path.join("bench_out", "bench_detail.json")

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` with no launcher (what the driver runs): this process becomes the launcher of N ranks of itself
        from squidpy_amd import _lib as _probe

        n_dev = _probe.device_count()
        if args.gpus > n_dev and not args.share_devices:
            print(f"bench.py: --gpus {args.gpus} but this node has {n_dev} GPU(s); refusing to report a {args.gpus}-GPU figure from fewer devices "
                  "(--share-devices puts several ranks on one GPU for tests: host collective, not a scaling measurement)", file=sys.stderr)
            sys.exit(2)
        # (a bound on the whole launch: an RCCL rendezvous that never completes must not hold the driver's node forever)
        sys.exit(launch_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus,
                              extra_env={"SQGR_DIST_COLLECTIVE": "host"} if args.gpus > n_dev else None,
                              timeout_s=float(os.environ.get("SQGR_BENCH_LAUNCH_TIMEOUT", "2400"))))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        # the record's n_gpus is the number of ranks that RAN; a launcher that started another number than --gpus is an error, never a relabelled figure
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} rank(s)", file=sys.stderr)
        sys.exit(2)

    from squidpy_amd import _dist, _lib
    from squidpy_amd._synthetic import hex_grid_graph
    from squidpy_amd.gr._nhood import expected_counts, zscore_from_moments

    ctx = _lib.default_context(local_rank % max(_lib.device_count(), 1))
    comm = None
    if world > 1:
        _dist.init()                 # socket rendezvous from the launcher's environment; torch is not imported
        comm = _dist.device_comm()   # RCCL communicator owned by libsqgr (None: host fall-back through the rendezvous)
    adj = hex_grid_graph(args.rows, args.cols)
    n, nnz = adj.shape[0], int(adj.nnz)
    lab_rng = np.random.default_rng(0)
    if args.label_dist == "dirichlet":
        labels = lab_rng.choice(N_CLS, size=n, p=lab_rng.dirichlet(np.full(N_CLS, 0.5))).astype(np.int32)
    else:
        labels = lab_rng.integers(0, N_CLS, n).astype(np.int32)
    graph = _lib.Graph(ctx, adj, with_data=False)          # resident in HBM from here on
    plan = _lib.NhoodPlan(ctx, graph, labels, N_CLS)
    if args.tune:
        plan.tune(*[int(v) for v in args.tune.split(",")])
    if comm is not None:
        plan.set_comm(comm)
    count = _lib.nhood_counts(ctx, graph, labels, N_CLS)
    shift = expected_counts(labels, N_CLS, nnz)
    strong = args.scaling == "strong"
    P = args.total_perms if strong else args.perms_per_step   # strong: per step over all ranks; weak: per step per rank

    def step(i: int):
        if strong:
            lo, hi = _dist.shard_range(P, rank, world, begin=i * P)
        else:
            lo = (i * world + rank) * P                     # disjoint global permutation indices per rank & step
            hi = lo + P
        s1, s2, _ = plan.run(12345, lo, hi, shift)          # with a communicator: moments all-reduced on the device (RCCL)
        if world > 1 and comm is None:
            s1, s2 = _dist.allreduce_sum_([s1, s2])         # host fall-back
        return s1, s2

    def fence():
        if world > 1:
            _dist.barrier()
        ctx.sync()                                          # both library streams (== device synchronise for this process)

    def reduce_max(seconds: float) -> float:
        if world <= 1:
            return seconds
        ns = np.array([int(seconds * 1e9)], dtype=np.int64)
        if comm is not None:
            return float(comm.allreduce_i64(ns, op=_lib.Comm.MAX)[0]) / 1e9
        return max(float(v) for v in _dist.allgather_object(seconds))

    for i in range(args.warmup):
        step(i)
    fence()
    ctx.timer_enable(True)
    ctx.timer_reset()
    t0 = time.perf_counter()
    tot1 = np.zeros((N_CLS, N_CLS), dtype=np.int64)
    tot2 = np.zeros((N_CLS, N_CLS), dtype=np.uint64)
    for i in range(args.steps):
        s1, s2 = step(args.warmup + i)
        tot1 += s1
        tot2 += s2
    fence()
    elapsed = reduce_max(time.perf_counter() - t0)
    kernels = ctx.timer_report()
    ctx.timer_enable(False)
    if args.dump_outputs and rank == 0 and args.steps > 0:  # what the last timed step handed back, and the z-scores of its permutations
        dump = {"moments_s1": s1, "moments_s2": s2, "zscore": zscore_from_moments(count, shift, s1, s2, P if strong else P * world), "counts": count}
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.asarray(arr, dtype=np.float64))
    rank_devices = [local_rank % max(_lib.device_count(), 1)] if world == 1 else [int(d) for d in _dist.allgather_object(local_rank % max(_lib.device_count(), 1))]
    collective = "none" if world == 1 else ("rccl-in-library (device all-reduce of the moments)" if comm is not None else _dist.collective_kind() + " (host fall-back)")

    ceil = load_ceilings()
    counters = load_counters()
    secondary = geary = None
    with_cpu = world == 1 and rank == 0 and not args.no_cpu_baseline
    if not args.no_secondary:
        secondary = autocorr_leg(ctx, "moran", world, fence, reduce_max, max(1, min(args.steps, 10)), with_cpu, counters)
        if world == 1:  # Geary's C on the hex grid: the float32 row sums of its degrees exercise the constant + exception lists
            geary = autocorr_leg(ctx, "geary", world, fence, reduce_max, max(1, min(args.steps, 10)), with_cpu, counters, graph_kind="hex")
    legs = None
    if world == 1 and not args.no_legs:
        legs = config4_legs(ctx, ceil, not args.no_cpu_baseline, counters, short_radii=not args.no_short_radii)
        if geary is not None:
            legs["geary_c"] = geary
        if not args.no_secondary:
            legs["moran_p100"] = moran_p100_leg(ctx, (secondary.get("cpu_baseline") or {}).get("value") if secondary else None)
            # Geary's general kernel (a third random LDS read per pair: row sums that take more than 8 values) — arbitrary weights, transformation=False
            legs["geary_general"] = autocorr_leg(ctx, "geary", world, fence, reduce_max, 3, False, counters, graph_kind="general")
        try:
            legs.update(nhood_variant_legs(ctx, adj, graph, n, None))
        except Exception as exc:  # pragma: no cover  (a leg must never cost the headline line)
            legs["nhood_variants_error"] = {"error": repr(exc)}
        if not args.no_secondary and not args.no_config3_full:
            try:
                legs["config3_full"] = config3_full_leg(secondary.get("cpu_baseline", {}).get("value") if secondary else None)
            except MemoryError as exc:  # pragma: no cover  (a host without 20 GB of free memory)
                legs["config3_full"] = {"error": repr(exc)}
    emulated = None
    if world == 1 and args.emulate_ranks > 1:
        # the N shards of config 5 (strong scaling) as they would run on N GPUs, one after the other on this one: per-shard wall time
        # = plan.run over the shard's permutation range incl. its launch ramp/tail and the 14 KB copy-out; the all-reduce of 2*K*K
        # int64 moments (< 15 KB, latency-bound) is NOT included
        N = args.emulate_ranks
        times = []
        for r in range(N):
            lo, hi = _dist.shard_range(args.total_perms, r, N)
            plan.run(777, lo, hi, shift)  # warm
            ctx.sync()
            t1 = time.perf_counter()
            plan.run(777, lo, hi, shift)
            ctx.sync()
            times.append(time.perf_counter() - t1)
        t1 = time.perf_counter()
        plan.run(777, 0, args.total_perms, shift)
        ctx.sync()
        t_all = time.perf_counter() - t1
        emulated = {"PROJECTION": f"the {N} rank shards of BASELINE config 5 run sequentially on ONE GPU; no multi-GPU hardware was used",
                    "total_perms": args.total_perms, "ranks": N, "shard_seconds": times, "one_gpu_seconds": t_all,
                    "projected_speedup_if_ranks_ran_concurrently": t_all / max(times), "fixed_cost_per_shard_s": max(0.0, (sum(times) - t_all) / N),
                    "not_included": "RCCL all-reduce of int64[2*K*K] (14.4 KB) per call; process start-up; PCIe contention"}

    if rank == 0:
        total_perms = args.steps * (P if strong else P * world)
        z = zscore_from_moments(count, shift, tot1, tot2, total_perms)
        assert np.isfinite(z).all(), "non-finite z-score in benchmark run"
        info = plan.info()
        cu_count = ctx.device_info().get("cu_count") or 256
        list_edges = info["list_edges"]                    # edges the count kernel walks (half list on a symmetric graph)
        per_rank_step = (P // world) if strong else P
        cnt_name = [k for k in kernels if k.startswith("nhood_count") and kernels[k][0] > 0]
        launches = sum(kernels[k][0] for k in cnt_name)
        ms_count = sum(kernels[k][1] for k in cnt_name)
        perms_per_launch = args.steps * per_rank_step / max(launches, 1)
        workload = {"spots": n, "nnz": nnz, "clusters": N_CLS, "list_edges": list_edges, "perms_per_launch": round(perms_per_launch, 3)}
        shuf_launch, ms_shuf = kernels.get("nhood_shuffle", (0, 0.0))
        red_launch, ms_red = kernels.get("nhood_reduce", (0, 0.0))

        def hbm_side(prefix: str, algorithmic_bytes_per_launch: float, launch_ms: float) -> dict:
            rec = kernel_counters(counters.get("nhood", {}), prefix, workload)
            side = {"algorithmic_bytes_per_launch": algorithmic_bytes_per_launch,
                    "algorithmic_GBps": algorithmic_bytes_per_launch / (launch_ms * 1e-3) / 1e9 if launch_ms > 0 else None,
                    "traffic_bytes_per_launch": None, "traffic_source": None}
            if rec and rec.get("FETCH_SIZE_bytes") is not None and rec.get("WRITE_SIZE_bytes") is not None:
                # FETCH_SIZE reports exactly half the bytes of this kernel's access patterns, WRITE_SIZE all of them: calibrated in this
                # repository (tools/ubench_fetch_calib.hip -> profiles/<round>_fetch_calibration.json); the guide's §HBM says the same
                traffic = 2.0 * rec["FETCH_SIZE_bytes"] + rec["WRITE_SIZE_bytes"]
                side["traffic_bytes_per_launch"] = traffic
                side["traffic_source"] = counters.get("_source")
                side["traffic_GBps"] = traffic / (launch_ms * 1e-3) / 1e9 if launch_ms > 0 else None
                side["traffic_frac_of_hbm_peak"] = traffic / (launch_ms * 1e-3) / HBM_PEAK if launch_ms > 0 else None
                side["algorithmic_reuse"] = algorithmic_bytes_per_launch / traffic if traffic > 0 else None
            return side, rec

        # ---- CSR-gather kernel: one ds_add_u32 lane-operation per (list edge, permutation)
        avg_count_ms = ms_count / max(launches, 1)
        atomics_per_launch = list_edges * perms_per_launch / 64.0                  # wave-instructions (64 lanes each)
        lds_rate = atomics_per_launch / (avg_count_ms * 1e-3) if avg_count_ms > 0 else 0.0
        b_gather = 4 * nnz + 4 * (n + 1) + n                                        # SURVEY §8d, per permutation
        side, rec = hbm_side("k_count", b_gather * perms_per_launch, avg_count_ms)
        roof = {
            "kernel": "+".join(cnt_name) or "nhood_count",
            "bound": "lds_atomic",
            "achieved": lds_rate,
            "peak": ceil.get("lds_add"),
            "unit": "ds_add_u32 wave-instr/s",
            "frac": lds_rate / ceil["lds_add"] if ceil.get("lds_add") else None,
            "traffic": side["traffic_bytes_per_launch"],
            "launches": launches,
            "avg_launch_ms": avg_count_ms,
            "perms_per_launch": perms_per_launch,
            "list_edges": list_edges,
            "symmetric_half_list": info["symmetric"],
            "workload_key": workload,
            "frac_of_pattern_ceiling": lds_rate / ceil["lds_add_pattern"] if ceil.get("lds_add_pattern") else None,
            "ceiling_source": ceil.get("source"),
            "hbm": side,
            "note": "the CSR gather of the permutation test: every edge of the (half) list adds 1 to one LDS counter per permutation, so "
            "ds_add_u32 issue is the floor (conflict-free chip rate measured by tools/ubench_ops.hip; `frac_of_pattern_ceiling` uses the "
            "rate of this kernel's own quad-staggered address pattern).  HBM is NOT the bound: one pass over the edge list serves 16 "
            "permutations, so SURVEY §8d's algorithmic bytes (4*nnz + 4*(N+1) + N per permutation) exceed the measured traffic by "
            "`hbm.algorithmic_reuse`",
        }
        if rec and rec.get("TCP_TOTAL_CACHE_ACCESSES_sum") is not None and avg_count_ms > 0:
            # the measured limiter (profiles/r02_count_probes.json): the label-row gathers.  The L1 serves one cache access
            # (64-byte granule of a gather instruction) per clock and CU (tools/ubench_gather.hip: 16 lines -> 16.05 clk)
            acc = rec["TCP_TOTAL_CACHE_ACCESSES_sum"]
            l1_peak = cu_count * 2.4e9
            roof["lds_atomic"] = {k: roof[k] for k in ("achieved", "peak", "unit", "frac", "frac_of_pattern_ceiling")}
            roof.update({
                "bound": "l1_gather",
                "achieved": acc / (avg_count_ms * 1e-3),
                "peak": l1_peak,
                "unit": "L1 cache accesses/s",
                "frac": acc / (avg_count_ms * 1e-3) / l1_peak,
                "l1": {"cache_accesses_per_launch": acc, "tcc_read_requests_per_launch": rec.get("TCP_TCC_READ_REQ_sum"),
                       "l1_hit_rate": 1.0 - rec["TCP_TCC_READ_REQ_sum"] / acc if rec.get("TCP_TCC_READ_REQ_sum") is not None else None,
                       "gather_wave_instr_per_launch": rec.get("TA_FLAT_READ_WAVEFRONTS_sum"),
                       "td_busy_frac": rec["TD_TD_BUSY_sum"] / (cu_count * avg_count_ms * 1e-3 * 2.4e9) if rec.get("TD_TD_BUSY_sum") is not None else None,
                       "probes": os.path.relpath(_profile("count_probes.json"), ROOT)},
                "note": "the CSR gather of the permutation test.  Developer probes of this kernel (" + os.path.relpath(_profile("count_probes.json"), ROOT) + ") show what bounds "
                "it: without the ds_add_u32 atomics it is NOT faster (0.48 vs 0.51 ms per 1024 permutations), without the label-row gathers it "
                "runs at the LDS-atomic rate of its address pattern (0.355 ms) — the gathers of 16-byte label rows (4 lanes x 4 bytes, two rows per "
                "edge and 16 permutations) through the vector-memory/L1 path are the limiter.  `achieved` = L1 cache accesses per launch (PMC "
                "TCP_TOTAL_CACHE_ACCESSES) / HIP-event time against one access per clock and CU; `lds_atomic` keeps the previous figure (one "
                "ds_add_u32 lane-operation per list edge and permutation against the measured ds_add_u32 rates); HBM is not the bound: one pass "
                "over the edge list serves 16 permutations (`hbm.algorithmic_reuse`)",
            })
        if rec and rec.get("SQ_INSTS_VALU") is not None:
            vi = rec["SQ_INSTS_VALU"]
            roof["valu"] = {"wave_instr_per_launch": vi, "per_atomic": vi / max(atomics_per_launch, 1.0),
                            "achieved": vi / (avg_count_ms * 1e-3), "peak": valu_mix_peak(ceil, 0.8), "unit": "wave-instr/s",
                            "frac": vi / (avg_count_ms * 1e-3) / valu_mix_peak(ceil, 0.8) if valu_mix_peak(ceil, 0.8) else None,
                            "note": "VALU side of the same kernel (v_perm_b32 + v_dot2_u32_u16 address, DPP offset spread; ~90 % complex class): "
                            "the VALU-only skeleton of the kernel takes 0.24 ms per 1024 permutations (" + os.path.relpath(_profile("count_probes.json"), ROOT) + ")"}
        # ---- the line's `roofline` object: HBM (SURVEY §8d names HBM for this kernel; VERDICT r2 asks for the measured-traffic fraction).
        # What limits the kernel in practice — the issue rate of its label-row gathers / LDS atomics — stays beside it as `issue_limits`.
        issue = roof
        # compulsory DRAM bytes of one launch: every label row of the slab is read once (n bytes per permutation), the block-partial
        # histograms are written once, the (half) edge list comes from HBM once (8 B per entry); everything else the kernel pulls through
        # the fabric is a re-read that the 256 MiB Infinity Cache can serve.  No gfx950 counter separates the two: TCC_EA0_RDREQ_DRAM ==
        # TCC_EA0_RDREQ to the request, FETCH_SIZE counts Infinity-Cache hits (profiles/r04_mall_calibration.json).
        dram_bytes = float(n) * perms_per_launch + float(info["partial_bytes_per_launch"]) + 8.0 * list_edges
        dram_bps = dram_bytes / (avg_count_ms * 1e-3) if avg_count_ms > 0 else None
        roof = {
            "kernel": issue["kernel"], "bound": "hbm",
            "achieved": dram_bps / 1e9 if dram_bps else None, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": dram_bps / HBM_PEAK if dram_bps else None,
            "traffic": dram_bytes,
            "frac_basis": "compulsory DRAM bytes per launch (slab once + partials once + edge list once) / HIP-event time; no counter separates Infinity-Cache hits",
            "fabric_traffic": side["traffic_bytes_per_launch"], "fabric_GBps": side.get("traffic_GBps"), "fabric_frac": side.get("traffic_frac_of_hbm_peak"),
            "traffic_source": side.get("traffic_source"),
            "traffic_formula": "fabric_traffic = 2 x FETCH_SIZE + WRITE_SIZE: calibrated on this kernel's own access patterns (4 B/lane row gathers, 8 B/lane list loads, "
            "4 B/lane stores) over 512 MiB each — FETCH_SIZE reports exactly 0.5, WRITE_SIZE 1.0 (profiles/r03_fetch_calibration.json); it counts what crosses the L2's "
            "memory-side port INCLUDING Infinity-Cache hits (profiles/r04_mall_calibration.json: a 24 MiB buffer re-read 160 times reports 3.2 GB)",
            "launches": launches, "avg_launch_ms": avg_count_ms, "perms_per_launch": perms_per_launch, "list_edges": list_edges,
            "symmetric_half_list": info["symmetric"], "workload_key": workload,
            "algorithmic_bytes_per_launch": side["algorithmic_bytes_per_launch"], "algorithmic_GBps": side["algorithmic_GBps"],
            "algorithmic_frac": side["algorithmic_GBps"] * 1e9 / HBM_PEAK if side.get("algorithmic_GBps") else None,
            "algorithmic_reuse": side.get("algorithmic_reuse"),
            "issue_limits": issue,
            "note": "`frac` = COMPULSORY DRAM bytes of the CSR-gather kernel per launch / its HIP-event time on the library's stream / 8 TB/s.  `fabric_frac` = measured memory-side "
            "traffic (PMC, same build, same workload) — it includes re-reads of the 24 MB edge list that the Infinity Cache serves.  `algorithmic_frac` = SURVEY §8d's bytes "
            "(4*nnz + 4*(N+1) + N per permutation) over the same time: above 1 because one pass over the edge list serves 16 permutations — REUSE, not a roofline fraction.  "
            "The kernel is not HBM-bound: `issue_limits` prices it against the L1 access rate of its gathers and the LDS-atomic rate (probe variants: "
            + os.path.relpath(_profile("count_probes.json"), ROOT) + "; experiments: profiles/r03_nhood_experiments.json, profiles/r04_mall_groups.json)",
        }
        if roof["fabric_frac"] is None:
            roof["note"] += ".  No PMC profile of THIS build and workload is committed (" + str(counters.get("_status")) + "): the fabric figures are null"
        # ---- label shuffle: VALU issue
        avg_shuf_ms = ms_shuf / max(shuf_launch, 1)
        side_s, rec_s = hbm_side("k_shuffle", n * perms_per_launch, avg_shuf_ms)
        shuf = {"kernel": "nhood_shuffle", "bound": "valu_issue", "achieved": None, "peak": valu_mix_peak(ceil, 0.65), "unit": "wave-instr/s", "frac": None,
                "traffic": side_s["traffic_bytes_per_launch"], "avg_launch_ms": avg_shuf_ms, "launches": shuf_launch, "hbm": side_s,
                "labels_per_s": n * perms_per_launch / (avg_shuf_ms * 1e-3) if avg_shuf_ms > 0 else None,
                "note": "two-level generator: one 8-round bijection per spot and 16 permutations + a 2-round network and a table look-up per "
                "label, two labels per packed-16 instruction; ~65 % of its VALU instructions are of the complex class (packed-16 / SDWA), "
                "the ceiling is the measured mix rate (" + str(ceil.get("source")) + "); instruction count per launch from PMC SQ_INSTS_VALU"}
        if rec_s and rec_s.get("SQ_INSTS_VALU") is not None and avg_shuf_ms > 0:
            shuf["achieved"] = rec_s["SQ_INSTS_VALU"] / (avg_shuf_ms * 1e-3)
            shuf["frac"] = shuf["achieved"] / shuf["peak"] if shuf["peak"] else None
            shuf["valu_wave_instr_per_label"] = rec_s["SQ_INSTS_VALU"] * 64.0 / (n * perms_per_launch)
        # ---- reduce: HBM (reads the partial histograms once)
        avg_red_ms = ms_red / max(red_launch, 1)
        red_bytes = info["partial_bytes_per_launch"]
        red = {"kernel": "nhood_reduce", "bound": "hbm", "achieved": red_bytes / (avg_red_ms * 1e-3) / 1e9 if avg_red_ms > 0 else None, "peak": HBM_PEAK / 1e9,
               "unit": "GB/s", "frac": red_bytes / (avg_red_ms * 1e-3) / HBM_PEAK if avg_red_ms > 0 else None, "traffic": None, "avg_launch_ms": avg_red_ms,
               "launches": red_launch, "note": "block-partial histograms (blocks x K*K*16 x 4 B per batch, h + h^T already formed by the count kernel) read once; L2-resident"}
        kern_ms = {k: round(v[1] / max(v[0], 1), 4) for k, v in kernels.items() if v[0] > 0}
        gpu_ms = sum(v[1] for v in kernels.values())
        # ---- the line's `roofline` names the LONGEST kernel of the step with its own compulsory DRAM bytes per launch
        # over its own HIP-event time; the count kernel's record (the CSR gather north_star prices) stays inside it as `count_kernel`,
        # and `step_dram_frac` = compulsory DRAM bytes of ALL kernels of a step / the step's wall time / 8 TB/s
        count_roof = roof
        per_kernel = {
            "nhood_shuffle": {"launches": shuf_launch, "total_ms": ms_shuf, "avg_launch_ms": avg_shuf_ms, "dram_bytes_per_launch": float(n) * perms_per_launch,
                              "what": "the label slab written once (n bytes per permutation)", "fabric": side_s, "issue_limits": {"valu": shuf.get("frac")}},
            "+".join(cnt_name) or "nhood_count": {"launches": launches, "total_ms": ms_count, "avg_launch_ms": avg_count_ms, "dram_bytes_per_launch": dram_bytes,
                                                  "what": "slab read once + partial histograms written once + edge list once", "fabric": side},
            "nhood_reduce": {"launches": red_launch, "total_ms": ms_red, "avg_launch_ms": avg_red_ms, "dram_bytes_per_launch": float(red_bytes),
                             "what": "partial histograms read once"},
        }
        for rec_k in per_kernel.values():
            rec_k["dram_frac"] = rec_k["dram_bytes_per_launch"] / (rec_k["avg_launch_ms"] * 1e-3) / HBM_PEAK if rec_k["avg_launch_ms"] > 0 else None
        step_bytes = sum(r["dram_bytes_per_launch"] * r["launches"] for r in per_kernel.values()) / args.steps
        step_dram_frac = step_bytes / (elapsed / args.steps) / HBM_PEAK
        dom_name = max(per_kernel, key=lambda k: per_kernel[k]["total_ms"])
        dom = per_kernel[dom_name]
        fab = dom.get("fabric") or {}
        roof = {
            "kernel": dom_name, "bound": "hbm",
            "achieved": dom["dram_bytes_per_launch"] / (dom["avg_launch_ms"] * 1e-3) / 1e9 if dom["avg_launch_ms"] > 0 else None,
            "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": dom["dram_frac"], "traffic": dom["dram_bytes_per_launch"],
            "frac_basis": f"compulsory DRAM bytes per launch of the step's longest kernel ({dom['what']}) / its HIP-event time",
            "fabric_traffic": fab.get("traffic_bytes_per_launch"), "fabric_GBps": fab.get("traffic_GBps"), "fabric_frac": fab.get("traffic_frac_of_hbm_peak"),
            "traffic_source": fab.get("traffic_source"),
            "launches": dom["launches"], "avg_launch_ms": dom["avg_launch_ms"], "perms_per_launch": perms_per_launch,
            "workload_key": workload,   # (tools/summarize_round.py stamps the PMC profile with it; kernel_counters() matches on it)
            "ms_per_step": dom["total_ms"] / args.steps, "share_of_kernel_time": dom["total_ms"] / gpu_ms if gpu_ms > 0 else None,
            "step_dram_frac": step_dram_frac, "step_dram_bytes": step_bytes,
            "dram_frac_by_kernel": {k: r["dram_frac"] for k, r in per_kernel.items()},
            "ms_per_step_by_kernel": {k: r["total_ms"] / args.steps for k, r in per_kernel.items()},
            "algorithmic_frac": count_roof.get("algorithmic_frac"), "algorithmic_reuse": count_roof.get("algorithmic_reuse"),
            "issue_limits": count_roof.get("issue_limits"),
            "count_kernel": count_roof,
            "note": "`kernel` = the longest kernel of a step, `frac` = ITS compulsory DRAM bytes / its own time / 8 TB/s; `step_dram_frac` = the compulsory DRAM "
            "bytes of every kernel of a step / the step's wall time / 8 TB/s — the step is NOT an HBM-roofline result: the label slab is produced and "
            "consumed once per permutation (2 x n bytes) and both of its kernels are issue-bound (`kernels`: the shuffle on VALU issue of its packed-16 "
            "instruction mix, the count kernel on the L1 rate of its label-row gathers and the LDS-atomic rate).  `count_kernel` keeps the CSR-gather record of "
            "rounds 2-5 (`algorithmic_frac` = SURVEY 8d's bytes over its time: reuse — one pass over the half edge list serves 16 permutations — not a fraction)",
        }
        b_perm = 4 * nnz + 4 * (n + 1) + 2 * n
        out = {
            "metric": "nhood_enrichment permutations/sec (1e6 spots x 30 clusters)",
            "value": total_perms / elapsed,
            "unit": "permutations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "u8 labels / u32 counts / i64 moments",
            "data": "synthetic",
            "config": {
                "workload": f"nhood_enrichment: {n} spots ({args.rows}x{args.cols} hex grid, nnz={nnz}), {N_CLS} clusters, "
                + (f"{P} permutations per step split over {world} rank(s) (BASELINE config 5)" if strong else f"{P} permutations per step per GPU")
                + ", on-device Philox-keyed label shuffles" + ("" if args.label_dist == "uniform" else ", Dirichlet(0.5) cluster proportions"),
                "label_dist": args.label_dist,
                "perms_per_step": P,
                "perms_per_step_per_gpu": per_rank_step,
                "parallelism": f"permutation ranges over {world} rank(s), one all-reduce of int64[2*K*K] moments per step",
                "collective": collective,
                "rccl_world": comm.info()[1] if comm is not None else None,   # what RCCL itself reports (null: no device communicator)
                "ranks_on_devices": rank_devices,
            },
            "roofline": roof,
            "kernels": {"nhood_shuffle": shuf, "nhood_count": {k: issue.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "lds_atomic")}, "nhood_reduce": red},
            "pipeline": {
                "algorithmic_bytes_per_perm": b_perm,
                "gpu_ms_all_kernels": gpu_ms,
                "algorithmic_GBps": b_perm * args.steps * per_rank_step / (gpu_ms * 1e-3) / 1e9 if gpu_ms > 0 else None,
                "algorithmic_reuse_vs_hbm_peak": b_perm * args.steps * per_rank_step / (gpu_ms * 1e-3) / HBM_PEAK if gpu_ms > 0 else None,
                "avg_kernel_ms": kern_ms,
                "time_share": {k: round(v[1] / gpu_ms, 3) for k, v in kernels.items() if v[0] > 0 and gpu_ms > 0},
                "gpu_busy_frac_of_wall": gpu_ms * 1e-3 / (elapsed) if elapsed > 0 else None,
                "note": "SURVEY §8d's B_perm (30.0 MB) against the sum of all kernel times; > HBM peak because one pass over the graph serves "
                "16 permutations — an algorithmic-reuse figure, NOT a roofline fraction (those are in `roofline` / `kernels`)",
            },
        }
        import hashlib

        first = args.warmup * (P if strong else P * world)
        out["check"] = {"perm_range": [first, first + total_perms],   # the GLOBAL permutation indices of the timed steps, whatever the number of ranks
                        "moments_sha16": hashlib.sha256(np.ascontiguousarray(tot1).tobytes() + np.ascontiguousarray(tot2).tobytes()).hexdigest()[:16]}
        if secondary is not None:
            out["secondary"] = secondary
        if legs is not None:
            for name, rec in legs.items():
                if name.startswith("nhood_") and isinstance(rec, dict) and rec.get("value"):
                    rec["vs_k30"] = rec["value"] / out["value"] if world == 1 else None
            out["legs"] = legs
        elif geary is not None:
            out["geary_c"] = geary
        if emulated is not None:
            out["emulated_ranks"] = emulated
        if world == 1 and not args.no_numpy_leg:  # the same test with numpy's own PCG64 streams reproduced bit for bit on the GPU
            out["numpy_stream_mode"] = numpy_stream_leg(ctx, plan, shift, n, counters)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(adj, labels)
            out["speedup_vs_cpu_1core"] = out["value"] / out["cpu_baseline"]["value"]
            if "value" in out["cpu_baseline"].get("all_cores", {}):
                out["speedup_vs_cpu_all_cores"] = out["value"] / out["cpu_baseline"]["all_cores"]["value"]
            if "numpy_stream_mode" in out:  # the CPU path draws exactly these streams: the like-for-like ratio
                out["numpy_stream_mode"]["cpu_baseline"] = {k: out["cpu_baseline"][k] for k in ("value", "unit", "cores", "kind", "sample")}
                out["numpy_stream_mode"]["speedup_vs_cpu_1core"] = out["numpy_stream_mode"]["value"] / out["cpu_baseline"]["value"]
        out["pmc_profile"] = counters.get("_status")
        detail_path = None
        try:  # the full record (notes, issue limits, PMC inputs, per-kernel tables): a side file, never the driver's line
            if args.detail_out:
                os.makedirs(os.path.dirname(os.path.abspath(args.detail_out)), exist_ok=True)
                with open(args.detail_out, "w") as fh:
                    json.dump(out, fh, indent=1)
                detail_path = args.detail_out
        except OSError as exc:  # pragma: no cover  (read-only checkout)
            print(f"bench.py: could not write {args.detail_out}: {exc}", file=sys.stderr)
        print(json.dumps(compact_line(out, detail_path)), flush=True)
    if world > 1:
        _dist.barrier()
        _dist.shutdown()


if __name__ == "__main__":
    main()
