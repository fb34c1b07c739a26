"""Generates tests/golden/sepal_reference.npz from the reference's LITERAL sepal source (gr/_sepal.py ``_compute_idxs``,
``_get_sat_unsat_idx``, ``_get_nhood_idx``, ``_diffusion``, ``_entropy``, ``_laplacian_hex``, ``_laplacian_rect``), executed through
``oracle.ref_shim`` with numba stubbed.  Run in the build container from the repository root:
    python tests/golden/make_sepal_golden.py

Per case: the inputs (graph, coordinates, genes, parameters), the lattice of ``_compute_idxs``, every gene's stop sweep from
``_diffusion`` (-1: NaN score), the band [i_lo, i_hi] of its entropy differences at delta = 1e-15, and the vectors of gene 0 after
1, 7 and 500 sweeps (``_diffusion`` with n_iter = k and a threshold no difference meets).  Also: the reference's ``sepal``
signature from the AST.  The reference's ``pairwise_distances`` call on zero rows (every unsaturated spot has a saturated
neighbour) raises in sklearn 1.7; the shim answers it with an empty distance matrix, which is what the drop-in returns."""

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

import sepal_oracle as SO  # noqa: E402

KEEP = (1, 7, 500)


def literal() -> dict:
    from sklearn.metrics import pairwise_distances

    def pd_(x, y, metric):
        if len(x) == 0:
            return np.zeros((0, len(y)))
        return pairwise_distances(x, y, metric=metric)

    ns = {"np": np, "pairwise_distances": pd_, "NDArrayA": np.ndarray, "spmatrix": sp.spmatrix}
    with ref_shim._numba_stubbed():
        ns["njit"] = ref_shim._njit
        ref_shim._extract("gr/_sepal.py", ["_compute_idxs", "_get_sat_unsat_idx", "_get_nhood_idx", "_diffusion", "_entropy",
                                           "_laplacian_rect", "_laplacian_hex"], ns)
    return ns


def signature() -> str:
    src = open(os.path.join(ref_shim.REF_SRC, "gr", "_sepal.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == "sepal":
            a = node.args
            pos = [x.arg for x in a.args]
            defaults = [ast.unparse(d) for d in a.defaults]
            k = len(pos) - len(defaults)
            return json.dumps({
                "positional": [{"name": n, "default": defaults[i - k] if i >= k else None} for i, n in enumerate(pos)],
                "keyword_only": [{"name": x.arg, "default": ast.unparse(d) if d is not None else None} for x, d in zip(a.kwonlyargs, a.kw_defaults)],
                "decorators": [ast.unparse(d) for d in node.decorator_list],
            })
    raise RuntimeError("sepal not found")


def visium49_graph(spatial: np.ndarray) -> sp.csr_matrix:
    """The reference's GridBuilder(n_neighs=6) logic on the fixture's coordinates: kNN(6), then edges shorter than 1.3 x median."""
    from sklearn.neighbors import NearestNeighbors

    xy = spatial.astype(np.float64)
    d, idx = NearestNeighbors(n_neighbors=7).fit(xy).kneighbors(xy)
    d, idx = d[:, 1:], idx[:, 1:]
    keep = d < 1.3 * np.median(d)
    rows = np.repeat(np.arange(len(xy)), 6)[keep.ravel()]
    g = sp.csr_matrix((np.ones(keep.sum(), np.float32), (rows, idx.ravel()[keep.ravel()])), shape=(len(xy), len(xy)))
    g = ((g + g.T) > 0).astype(np.float32).tocsr()
    g.sort_indices()
    return g


def cases() -> list[dict]:
    out = []
    v = np.load(os.path.join(HERE, "visium49.npz"))
    g = visium49_graph(v["spatial"])
    deg = np.diff(g.indptr).max()
    out.append(dict(name="visium49", g=g, spatial=v["spatial"].astype(np.float64), X=v["X40"][:, :6].astype(np.float32),
                    K=int(deg), n_iter=30000))
    xy, g = SO.hex_grid(20, 20)
    out.append(dict(name="hex20_shuffled", g=SO.shuffle_rows(g, 3), spatial=xy, X=SO.mixed_genes(xy, 4, seed=1), K=6, n_iter=30000))
    rng = np.random.default_rng(42)  # the reference's adata_squaregrid, standardised with numpy (scanpy's sc.pp.scale)
    coord = np.unique(rng.integers(0, 10, size=(400, 2)), axis=0)
    counts = rng.integers(0, 10, size=(coord.shape[0], 10)).astype(np.float64)
    Xs = (counts - counts.mean(0)) / counts.std(0, ddof=1)
    out.append(dict(name="squaregrid", g=SO.radius_graph(coord.astype(np.float64), 1.0), spatial=coord.astype(np.float64), X=Xs[:, :4], K=4, n_iter=30000))
    xy, g = SO.hex_grid(12, 12)
    n = len(xy)
    special = np.zeros((n, 5))
    special[:, 1] = 2.5                      # constant
    special[77, 2] = 9.0                     # a single hot spot
    special[:, 3] = SO.mixed_genes(xy, 1, seed=5)[:, 0]
    special[40, 3] = np.nan                  # a NaN
    special[:, 4] = SO.mixed_genes(xy, 3, seed=6)[:, 2]  # a blob
    out.append(dict(name="hex12_special", g=g, spatial=xy, X=special, K=6, n_iter=30000))
    out.append(dict(name="hex12_short", g=g, spatial=xy, X=special[:, [4]], K=6, n_iter=50))  # does not converge within n_iter
    return out


def main() -> None:
    ns = literal()
    dt, thresh = 0.001, 1e-8
    blob: dict[str, np.ndarray] = {"signature": np.array(signature()), "dt": np.array(dt), "thresh": np.array(thresh)}
    names = []
    for c in cases():
        g, K, name = c["g"], c["K"], c["name"]
        sat, sat_idx, unsat, unsat_idx = ns["_compute_idxs"](g, c["spatial"], K, "l1")
        X = np.asarray(c["X"])
        stops, bands = [], []
        for j in range(X.shape[1]):
            conc = np.ascontiguousarray(X[:, j], dtype=np.float64)
            r = ns["_diffusion"](conc.copy(), K == 6, c["n_iter"], sat, sat_idx, unsat, unsat_idx, dt, thresh)
            stops.append(-1 if np.isnan(r) else int(r))
            _, deltas, _, _ = SO.diffusion(conc, K == 6, c["n_iter"], SO.compute_idxs(g, c["spatial"], K), dt, thresh)
            bands.append(SO.band(deltas, thresh))
            print(name, j, stops[-1], bands[-1], flush=True)
        conc0 = np.ascontiguousarray(X[:, 0], dtype=np.float64)
        for k in KEEP:
            cc = conc0.copy()
            ns["_diffusion"](cc, K == 6, k, sat, sat_idx, unsat, unsat_idx, dt, -1.0)
            blob[f"{name}/conc{k}"] = cc
        blob.update({
            f"{name}/indptr": g.indptr.astype(np.int64), f"{name}/indices": g.indices.astype(np.int32), f"{name}/data": g.data.astype(np.float32),
            f"{name}/spatial": c["spatial"], f"{name}/X": X, f"{name}/K": np.array(K), f"{name}/n_iter": np.array(c["n_iter"]),
            f"{name}/sat": np.asarray(sat, np.int32), f"{name}/sat_idx": np.asarray(sat_idx, np.int32),
            f"{name}/unsat": np.asarray(unsat, np.int32), f"{name}/unsat_idx": np.asarray(unsat_idx, np.int32),
            f"{name}/stop": np.array(stops, np.int32), f"{name}/band": np.array(bands, np.int32),
        })
        names.append(name)
    blob["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "sepal_reference.npz"), **blob)
    print("wrote", os.path.join(HERE, "sepal_reference.npz"), os.path.getsize(os.path.join(HERE, "sepal_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
