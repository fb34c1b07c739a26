"""Timing of sq.gr.sepal on the device (plan level: the lattice and the matrix resident, ``SepalPlan.run``) and of its CPU baseline.

    python tools/sepal_time.py [--out profiles/sepal_time.json] [--cpu-genes 32] [--skip-cpu]

Workloads: W1 Visium, 78 x 64 hex = 4 992 spots, 2 000 genes; W2 128 x 112 hex = 14 336 spots, 500 genes; W3 256 x 256
square = 65 536 spots (the global route), 64 genes — seeded mixed structure at the scale of spots (noise, stripes, blobs; ``tests/sepal_oracle.spot_scale_genes``),
default n_iter / dt / thresh.
Prints per workload: wall time, genes/s, spot-sweeps/s (sum of sweeps x n / wall), the kernel time of the library's HIP-event
timers, the kernels' VGPRs / occupancy (hipcc's resource remarks), and the fraction of the float64 VALU issue ceiling: the f64
instructions per spot-sweep (static count of the unrolled sweep in hipcc's gfx950 assembly / items per thread) at the
v_add_f64 rate of profiles/r06_ubench_f64.json.  CPU baseline (kind: port): tools/sepal_cport.c on one core and on 16 threads,
over the first --cpu-genes genes of each workload (at least 16, so that 16 threads have work).  Last, the longest launches: genes
that never stop, two full chunks of sweeps on each route."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from squidpy_amd._lib import DeviceMatrix, SepalPlan, default_context  # noqa: E402
from squidpy_amd.gr._sepal import sepal_lattice  # noqa: E402
from tests import sepal_oracle as SO  # noqa: E402

WORKLOADS = {"W1": ("hex", 78, 64, 2000), "W2": ("hex", 128, 112, 500), "W3": ("square", 256, 256, 64)}
SRC = os.path.join(ROOT, "squidpy_amd", "csrc", "sqgr_sepal.hip")


def resources() -> dict:
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", SRC,
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def f64_per_item(pattern: str, items: int) -> float:
    """f64 VALU instructions in the kernel's assembly (the unrolled sweep holds `items` spot updates and entropy terms)."""
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                               SRC, "-o", tmp.name], stderr=subprocess.DEVNULL)
        lines = open(tmp.name).read().split("\n")
    st = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and pattern in l)
    n = 0
    for l in lines[st:]:
        if "s_endpgm" in l:
            break
        if re.match(r"\s+v_\w+_f64", l):
            n += 1
    return n / items


def cport():
    d = tempfile.mkdtemp()
    so = os.path.join(d, "sepal_cport.so")
    subprocess.check_call(["gcc", "-O3", "-march=native", "-fopenmp", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(ROOT, "tools", "sepal_cport.c"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.sepal_genes.restype = None
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-genes", type=int, default=32)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    ctx = default_context()
    ub = json.load(open(os.path.join(ROOT, "profiles", "r06_ubench_f64.json")))
    add_rate = next(v["wave_instr_per_s"] for v in ub["valu"] if v["op"] == "v_add_f64")
    res = resources()
    # static float64 instruction counts per spot-sweep: the LDS kernel's unrolled sweep holds 8 spots per thread; the global kernel's
    # loops hold one spot each, so its count also carries the per-sweep reductions once (an upper bound of the per-spot work)
    f64 = {("lds", 6): f64_per_item("k_sepal_ldsILi6ELi8E", 8), ("lds", 4): f64_per_item("k_sepal_ldsILi4ELi8E", 8),
           ("global", 6): f64_per_item("k_sepal_globalILi6ENS0_5Tab16", 1), ("global", 4): f64_per_item("k_sepal_globalILi4ENS0_5Tab16", 1)}
    lib = None if a.skip_cpu else cport()
    report = {"device": ctx.device_info(), "resources": res, "f64_instr_per_spot_sweep_static": {f"{r}_{k}": v for (r, k), v in f64.items()}, "v_add_f64_wave_instr_per_s": add_rate, "workloads": {}}
    for key, (kind, rows, cols, G) in WORKLOADS.items():
        if a.only and key not in a.only.split(","):
            continue
        xy, g = SO.hex_grid(rows, cols) if kind == "hex" else SO.square_grid(rows, cols)
        K = 6 if kind == "hex" else 4
        X = np.ascontiguousarray(SO.spot_scale_genes(xy, G, seed=7))
        n = len(xy)
        sat, sat_idx, unsat, nearest = sepal_lattice(g, xy, K)
        pos = np.empty(n, np.int64)
        pos[sat] = np.arange(len(sat))
        plan = SepalPlan(ctx, n, K, sat, sat_idx, unsat, pos[nearest])
        m = DeviceMatrix(ctx, X)
        cols_ = np.arange(G, dtype=np.int32)
        plan.run(m, cols_[: min(G, 4)], 30000, 0.001, 1e-8)  # warm-up (first launch, allocations)
        ctx.timer_enable(True)
        ctx.timer_reset()
        t0 = time.perf_counter()
        it = plan.run(m, cols_, 30000, 0.001, 1e-8)
        wall = time.perf_counter() - t0
        rep = ctx.timer_report()
        ctx.timer_enable(False)
        sweeps = int(np.where(it >= 0, it + 1, 30000).sum())
        kern = {k: v for k, v in rep.items() if k.startswith("sepal")}
        rate = sweeps * n / wall
        # issue ceiling in spot-sweeps/s: f64 wave-instructions/s x 64 lanes / f64 instructions per spot-sweep
        route = "lds" if kern.get("sepal_lds", (0, 0.0))[0] > 0 else "global"  # which kernel the library launched
        ceiling = add_rate * 64 / f64[(route, K)]
        w = {"n": n, "genes": G, "route": route, "wall_s": wall, "genes_per_s": G / wall, "sum_sweeps": sweeps,
             "spot_sweeps_per_s": rate, "kernel_ms": kern, "stop_sweeps_min_median_max": [int(np.min(it)), int(np.median(it)), int(np.max(it))],
             "n_nan": int((it < 0).sum()), "f64_issue_ceiling_spot_sweeps_per_s": ceiling, "fraction_of_f64_issue_ceiling": rate / ceiling}
        if lib is not None:
            cg = min(a.cpu_genes, G)
            Xc = np.ascontiguousarray(X[:, :cg].T)
            out = np.empty(cg, np.int32)
            args = lambda Xb: (Xb.ctypes.data_as(C.c_void_p), C.c_int64(cg), C.c_int64(n), C.c_int(K == 6), C.c_int32(30000),  # noqa: E731
                                sat.ctypes.data_as(C.c_void_p), C.c_int64(len(sat)), np.ascontiguousarray(sat_idx).ctypes.data_as(C.c_void_p), C.c_int32(K),
                                unsat.ctypes.data_as(C.c_void_p), C.c_int64(len(unsat)), nearest.ctypes.data_as(C.c_void_p), C.c_double(0.001), C.c_double(1e-8),
                                out.ctypes.data_as(C.c_void_p))
            cpu = {}
            for threads in (1, 16):
                lib.sepal_set_threads(threads)
                Xb = Xc.copy()
                t0 = time.perf_counter()
                lib.sepal_genes(*args(Xb))
                dt_ = time.perf_counter() - t0
                cs = int(np.where(out >= 0, out + 1, 30000).sum())
                cpu[f"threads_{threads}"] = {"genes": cg, "wall_s": dt_, "spot_sweeps_per_s": cs * n / dt_, "genes_per_s_at_workload_mix": cg / dt_,
                                             "same_stop_sweeps_as_device": bool(np.array_equal(out, it[:cg]))}
            w["cpu_port"] = {"kind": "port", **cpu}
        report["workloads"][key] = w
        print(key, json.dumps(w), flush=True)
        m.close()
        plan.close()
    # the longest launches: genes that never stop (thresh < 0) run two full chunks; run_batch sizes a chunk to about
    # SEPAL_LAUNCH_BUDGET (LDS) / SEPAL_GLOBAL_BUDGET (global) spot-sweeps
    report["worst_launch"] = {}
    for key, (kind, rows, cols, G, budget) in {"lds_14336": ("hex", 128, 112, 512, 6.0e10), "global_65536": ("square", 256, 256, 64, 2.0e10)}.items():
        if a.only and "worst" not in a.only.split(","):
            continue
        xy, g = SO.hex_grid(rows, cols) if kind == "hex" else SO.square_grid(rows, cols)
        K = 6 if kind == "hex" else 4
        n = len(xy)
        sat, sat_idx, unsat, nearest = sepal_lattice(g, xy, K)
        pos = np.empty(n, np.int64)
        pos[sat] = np.arange(len(sat))
        plan = SepalPlan(ctx, n, K, sat, sat_idx, unsat, pos[nearest])
        m = DeviceMatrix(ctx, np.ascontiguousarray(SO.spot_scale_genes(xy, 3, seed=1)))
        chunk = int(budget / (G * n))
        ctx.timer_enable(True)
        ctx.timer_reset()
        it = plan.run(m, (np.arange(G) % 3).astype(np.int32), 2 * chunk, 0.001, -1.0)
        rep = ctx.timer_report()
        ctx.timer_enable(False)
        name = "sepal_lds" if kind == "hex" else "sepal_global"
        cnt, ms = rep[name]
        w = {"n": n, "genes": G, "sweeps_per_launch": chunk, "launches": cnt, "ms_per_launch": ms / cnt, "spot_sweeps_per_launch": G * n * chunk,
             "spot_sweeps_per_s": G * n * chunk * cnt / (ms / 1e3), "all_ran_to_n_iter": bool((it < 0).all())}
        report["worst_launch"][key] = w
        print("worst", key, json.dumps(w), flush=True)
        m.close()
        plan.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
