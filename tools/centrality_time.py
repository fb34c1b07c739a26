"""Timing of sq.gr.centrality_scores on the device and of networkx on one core of the same box.

    python tools/centrality_time.py [--out profiles/centrality_time.json] [--skip-networkx] [--side 1000]

Workloads: a side x side hex lattice (1e6 spots) x 30 clusters, labels uniform at random ("random") and in 30 horizontal bands
("bands": a tissue-domain labelling, many BFS levels), and the directed kNN-6 graph of 1e6 uniform points x 30 random clusters.
Per workload: the whole front-end call (host symmetrisation, upload, kernels, float formation; wall clock after a device
synchronise; a second call finds the graph resident), the HIP-event kernel sum by kernel, the number of BFS levels, and the two C
entry points alone on the resident graph.  networkx (``group_closeness_centrality``, ``group_degree_centrality``,
``average_clustering``): all 30 groups at 1e5 spots; at 1e6 spots ONE group, times 30 as a stated extrapolation."""
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
from squidpy_amd import AnnDataLite, _synthetic  # noqa: E402
from squidpy_amd._lib import cached_graph, clear_graph_cache, default_context, graph_triangles, group_bfs  # noqa: E402
from squidpy_amd.gr._nhood import centrality_graph  # noqa: E402

K = 30


def labels_of(kind: str, rows: int, cols: int, rng) -> np.ndarray:
    n = rows * cols
    if kind == "random":
        return rng.integers(0, K, n).astype(np.int32)
    return (np.arange(n) // cols * K // rows).astype(np.int32)  # bands of rows


def adata_of(g, codes) -> AnnDataLite:
    obs = pd.DataFrame({"cluster": pd.Categorical.from_codes(codes, [f"c{i}" for i in range(K)])})
    return AnnDataLite(X=None, obs=obs, obsp={"spatial_connectivities": g})


def device(ctx, g, codes) -> dict:
    ad = adata_of(g, codes)
    clear_graph_cache()
    ctx.sync()
    t0 = time.perf_counter()
    df = sq.gr.centrality_scores(ad, "cluster", copy=True)
    ctx.sync()
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    df2 = sq.gr.centrality_scores(ad, "cluster", copy=True)
    ctx.sync()
    second = time.perf_counter() - t0
    ctx.timer_enable(True)  # a run of its own: the event pairs around every launch cost host time
    ctx.timer_reset()
    df3 = sq.gr.centrality_scores(ad, "cluster", copy=True)
    ctx.sync()
    rep = {k: v for k, v in ctx.timer_report().items() if k.startswith("centrality")}
    ctx.timer_enable(False)
    assert df.equals(df2) and df.equals(df3)
    t0 = time.perf_counter()
    adj = centrality_graph(g)
    host_graph = time.perf_counter() - t0
    graph = cached_graph(ctx, adj, with_data=False)
    ctx.sync()
    t0 = time.perf_counter()
    _, _, _, levels = group_bfs(ctx, graph, codes, K)
    ctx.sync()
    t_bfs = time.perf_counter() - t0
    t0 = time.perf_counter()
    graph_triangles(ctx, graph)
    ctx.sync()
    t_tri = time.perf_counter() - t0
    return {"n": int(g.shape[0]), "nnz_symmetrised": int(adj.nnz), "clusters": K, "whole_call_first_s": first, "whole_call_graph_resident_s": second,
            "host_symmetrise_s": host_graph, "kernels_launches_ms": rep, "kernel_sum_ms": sum(v[1] for v in rep.values()), "bfs_levels": levels,
            "group_bfs_call_s": t_bfs, "graph_triangles_call_s": t_tri, "scores_head": df.head(3).to_dict()}


def networkx_time(g, codes, groups) -> dict:
    import networkx as nx

    adj = centrality_graph(g)
    t0 = time.perf_counter()
    G = nx.from_scipy_sparse_array(adj)
    build = time.perf_counter() - t0
    out = {"n": int(g.shape[0]), "groups_timed": len(groups), "graph_build_s": build, "closeness_s": 0.0, "degree_s": 0.0, "clustering_s": 0.0}
    vals = []
    for grp in groups:
        idx = [int(i) for i in np.flatnonzero(codes == grp)]
        t0 = time.perf_counter()
        c = nx.group_closeness_centrality(G, idx)
        t1 = time.perf_counter()
        d = nx.group_degree_centrality(G, idx)
        t2 = time.perf_counter()
        a = nx.average_clustering(G, idx)
        t3 = time.perf_counter()
        out["closeness_s"] += t1 - t0
        out["degree_s"] += t2 - t1
        out["clustering_s"] += t3 - t2
        vals.append((c, d, a))
    out["scores_s"] = out["closeness_s"] + out["degree_s"] + out["clustering_s"]
    out["values"] = vals[:3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--skip-networkx", action="store_true")
    a = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    side = a.side
    report = {"device": ctx.device_info(), "workloads": {}, "networkx": {}}
    hexg = _synthetic.hex_grid_graph(side, side)
    for kind in ("random", "bands"):
        codes = labels_of(kind, side, side, rng)
        report["workloads"][f"hex_{kind}"] = w = device(ctx, hexg, codes)
        print(f"hex_{kind}", json.dumps(w), flush=True)
    xy = rng.uniform(0.0, float(side), (side * side, 2))
    knn = _synthetic.knn_directed_graph(xy, 6, ctx)
    knn_codes = rng.integers(0, K, side * side).astype(np.int32)
    report["workloads"]["knn6_random"] = w = device(ctx, knn, knn_codes)
    print("knn6_random", json.dumps(w), flush=True)
    if not a.skip_networkx:
        import networkx as nx

        small = max(side * side // 10, 100)
        rows = int(round(small ** 0.5))
        g = _synthetic.hex_grid_graph(rows, rows)
        codes = labels_of("random", rows, rows, np.random.default_rng(1))
        nxs = networkx_time(g, codes, list(range(K)))
        dev = device(ctx, g, codes)
        report["networkx"]["hex_random_small_all_groups"] = {"version": nx.__version__, **nxs, "device_whole_call_graph_resident_s": dev["whole_call_graph_resident_s"],
                                                            "device_whole_call_first_s": dev["whole_call_first_s"]}
        print("networkx small", json.dumps(report["networkx"]["hex_random_small_all_groups"]), flush=True)
        codes = labels_of("random", side, side, np.random.default_rng(0))
        one = networkx_time(hexg, codes, [0])
        report["networkx"]["hex_random_one_group"] = {**one, "extrapolated_all_groups_s": one["scores_s"] * K,
                                                      "note": f"one group measured; x{K} is an extrapolation, not a measurement"}
        print("networkx one group", json.dumps(report["networkx"]["hex_random_one_group"]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
