"""Generates tests/golden/centrality_reference.npz.  Run in the build container from the repository root:
    python tests/golden/make_centrality_golden.py

Per case of ``tests/centrality_oracle.cases()``: the inputs (the connectivities as the caller stores them, the category codes with
-1 for NaN, the number of categories); the CSR the reference's LITERAL ``_build_graph`` makes of them (gr/_nhood.py:432-454,
executed through ``oracle.ref_shim`` with a stand-in for ``rx`` that only records nodes and edges) and the edges it hands rustworkx;
the per-node clustering coefficients of the literal ``_local_clustering`` (:457-491, numba stubbed) and their group means by the
reference's own expression; and networkx's ``group_closeness_centrality``, ``group_degree_centrality`` and ``average_clustering``
per group on the graph of those edges.  A category without observations (or one holding every node) is not pinned — rustworkx
alone defines what the reference returns there, and it is not installed — and is stored as 0.0 with ``pinned`` False.
Also: the reference's ``centrality_scores`` signature from the AST and the members of its ``Centrality`` enum."""

from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shim  # noqa: E402

import centrality_oracle as CO  # noqa: E402


class _RecordingGraph:
    """Stands in for ``rx.PyGraph``: keeps what ``_build_graph`` adds."""

    def __init__(self, multigraph: bool = True):
        self.multigraph = multigraph
        self.nodes: list = []
        self.edges: list = []

    def add_nodes_from(self, nodes):
        self.nodes.extend(nodes)

    def add_edges_from_no_data(self, edges):
        self.edges.extend(edges)


class _Rx:
    PyGraph = _RecordingGraph


def literal() -> dict:
    ns = {"np": np, "csr_matrix": sp.csr_matrix, "rx": _Rx, "njit": ref_shim._njit, "prange": range}
    with ref_shim._numba_stubbed():
        ref_shim._extract("gr/_nhood.py", ["_build_graph", "_local_clustering"], ns)
    return ns


def signature() -> str:
    src = open(os.path.join(ref_shim.REF_SRC, "gr", "_nhood.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == "centrality_scores":
            a = node.args
            pos = [x.arg for x in a.args]
            defaults = [ast.unparse(d) for d in a.defaults]
            k = len(pos) - len(defaults)
            return json.dumps({
                "positional": [{"name": n, "default": defaults[i - k] if i >= k else None} for i, n in enumerate(pos)],
                "keyword_only": [{"name": x.arg, "default": ast.unparse(d) if d is not None else None} for x, d in zip(a.kwonlyargs, a.kw_defaults)],
            })
    raise RuntimeError("centrality_scores not found")


def enum_members() -> str:
    src = open(os.path.join(ref_shim.REF_SRC, "_constants", "_constants.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name == "Centrality":
            return json.dumps([[t.targets[0].id, ast.literal_eval(t.value)] for t in node.body if isinstance(t, ast.Assign)])
    raise RuntimeError("Centrality not found")


def main() -> None:
    import networkx as nx

    ns = literal()
    blob: dict[str, np.ndarray] = {"signature": np.array(signature()), "enum": np.array(enum_members()), "networkx": np.array(nx.__version__)}
    names = []
    for c in CO.cases():
        name, conn, codes, K = c["name"], sp.csr_matrix(c["conn"]), c["codes"], c["n_cls"]
        graph, adj = ns["_build_graph"](conn.copy())
        n = adj.shape[0]
        assert graph.nodes == list(range(n)) and not graph.multigraph
        G = nx.Graph()
        G.add_nodes_from(graph.nodes)
        G.add_edges_from(graph.edges)
        cc = ns["_local_clustering"](adj.indptr, adj.indices, n)
        cols = {k: np.zeros(K) for k in CO.COLUMNS}
        nx_clustering = np.zeros(K)
        pinned = np.zeros(K, dtype=bool)
        for g in range(K):
            idx = np.where(codes == g)[0]
            if len(idx) == 0 or len(idx) == n:
                continue
            pinned[g] = True
            members = [int(i) for i in idx]
            cols["closeness_centrality"][g] = nx.group_closeness_centrality(G, members)
            cols["degree_centrality"][g] = nx.group_degree_centrality(G, members)
            cols["average_clustering"][g] = float(cc[idx].mean()) if len(idx) else 0.0  # gr/_nhood.py:316
            nx_clustering[g] = nx.average_clustering(G, members)
        blob.update({
            f"{name}/conn_indptr": conn.indptr.astype(np.int64), f"{name}/conn_indices": conn.indices.astype(np.int32),
            f"{name}/conn_data": conn.data.astype(np.float64), f"{name}/codes": codes.astype(np.int32), f"{name}/n_cls": np.array(K),
            f"{name}/adj_indptr": adj.indptr.astype(np.int64), f"{name}/adj_indices": adj.indices.astype(np.int32),
            f"{name}/edges": np.array(graph.edges, dtype=np.int32).reshape(-1, 2), f"{name}/cc": cc, f"{name}/pinned": pinned,
            f"{name}/nx_average_clustering": nx_clustering,
        })
        for k, v in cols.items():
            blob[f"{name}/{k}"] = v
        names.append(name)
        print(name, n, adj.nnz, K, int(pinned.sum()), flush=True)
    blob["cases"] = np.array(names)
    path = os.path.join(HERE, "centrality_reference.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
