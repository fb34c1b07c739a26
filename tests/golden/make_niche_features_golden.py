"""Generates tests/golden/niche_features_reference.npz.  Run in the build container from the repository root:
    python tests/golden/make_niche_features_golden.py

Everything stored is produced by the reference's LITERAL code on the small inputs of tests/niche_features_cases.py, converted to
float64 first (the result dtype of the reference is an accident of its inputs; the product is pinned to the float64 run):

- ``shell/<graph>/<k>/...``: ``hop_k`` and ``vis_k`` of ``_setdiag`` / ``_hop`` (gr/_niche.py:1002-1027, through ``oracle.ref_shim._extract``)
  for k = 1, 2, 3 on every graph of unit weights.
- ``agg/<graph>/<aggregation>/<k>``: ``_aggregate(adata, _normalize(hop_k), aggregation)`` (:1030-1054) on CSR ``X``, on two of the graphs.
- ``cc/<graph>/<aggregation>/<csr|dense>/<distance>``: ``arr`` of ``_CellcharterEmbedder.get_embedding`` (:1336-1355), the matrix handed to
  ``sc.tl.pca``; ``cc_dense_ok/...`` records where the literal source accepts a dense ``X``.
- ``utag/<graph>/<csr|dense>``: the matrix ``_UtagEmbedder.get_embedding`` (:1259-1262) hands to ``sc.tl.pca``.
- ``profile/<graph>/<labels>/<setting>``: what ``_NhoodProfileEmbedder.get_embedding`` (:1171-1226, ``scale=False``) returns.

The ``get_embedding`` bodies are class methods: they are compiled from the reference's AST at run time (annotations dropped), and
``ad.AnnData`` / ``sc`` are stand-ins that capture the matrix handed to scanpy.  No reference text is kept here or in the fixture."""

from __future__ import annotations

import ast
import io
import logging
import os
import sys
import types
import warnings
import zipfile

import numpy as np
import pandas as pd
from scipy import sparse as sps
from scipy.sparse import coo_matrix, hstack, issparse, lil_matrix, spdiags
from sklearn.preprocessing import normalize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shim  # noqa: E402

import niche_features_cases as FC  # noqa: E402


class _CapturedAnnData:
    """Stands in for ``ad.AnnData``: keeps the matrix it is given."""

    def __init__(self, X=None, obs=None):
        self.X = X
        self.obs = obs
        self.obsm: dict = {}


def _capture_pca(adata: _CapturedAnnData) -> None:
    adata.obsm["X_pca"] = adata.X  # the matrix scanpy would be handed


def _methods(class_name: str, names: list[str], ns: dict) -> dict:
    """The methods ``names`` of the reference's class ``class_name`` as plain functions (first argument ``self``) in ``ns``."""
    path = os.path.join(ref_shim.REF_SRC, "gr", "_niche.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    cls = next(node for node in tree.body if isinstance(node, ast.ClassDef) and node.name == class_name)
    keep = [ref_shim._Strip().visit(node) for node in cls.body if isinstance(node, ast.FunctionDef) and node.name in names]
    assert {node.name for node in keep} == set(names), (class_name, names)
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    out: dict = dict(ns)
    exec(compile(mod, path, "exec"), out)
    return out


def literal() -> dict:
    ns = {
        "np": np, "pd": pd, "sps": sps, "issparse": issparse, "spdiags": spdiags, "hstack": hstack, "lil_matrix": lil_matrix,
        "coo_matrix": coo_matrix, "normalize": normalize, "warnings": warnings, "logg": logging.getLogger("niche-features-golden"),
        "ad": types.SimpleNamespace(AnnData=_CapturedAnnData),
        "sc": types.SimpleNamespace(tl=types.SimpleNamespace(pca=_capture_pca), pp=types.SimpleNamespace(scale=None)),
    }
    ref_shim._extract("gr/_niche.py", ["_setdiag", "_hop", "_normalize", "_aggregate"], ns)
    ns["profile"] = _methods("_NhoodProfileEmbedder", ["_calculate_neighborhood_profile", "get_embedding"], ns)
    ns["utag"] = _methods("_UtagEmbedder", ["get_embedding"], ns)["get_embedding"]
    ns["cellcharter"] = _methods("_CellcharterEmbedder", ["get_embedding"], ns)["get_embedding"]
    return ns


def _table(graph, x=None, obs=None):
    return types.SimpleNamespace(obsp={"spatial_connectivities": graph}, X=x, obs=obs)


def _dense(m) -> np.ndarray:
    return np.ascontiguousarray(m.toarray() if issparse(m) else np.asarray(m), dtype=np.float64)


def profile_embedding(ns: dict, graph, column, distance: int, abs_nhood: bool, weights) -> np.ndarray:
    fns = ns["profile"]
    me = types.SimpleNamespace(groups="groups", spatial_connectivities_key="spatial_connectivities", scale=False, distance=distance,
                               abs_nhood=abs_nhood, n_hop_weights=weights)
    me._calculate_neighborhood_profile = lambda adata, matrix: fns["_calculate_neighborhood_profile"](me, adata, matrix)
    obs = pd.DataFrame({"groups": column}, index=[f"cell{i}" for i in range(graph.shape[0])])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = fns["get_embedding"](me, _table(graph.copy(), obs=obs))
    return _dense(out)


def main() -> None:
    logging.getLogger("niche-features-golden").setLevel(logging.ERROR)
    ns = literal()
    blob: dict[str, np.ndarray] = {}
    graphs = FC.golden_graphs()
    for name, a in graphs.items():
        a = a.astype(np.float64)
        n = a.shape[0]
        x = FC.expression(n, FC.N_VARS, 100 + n)
        codes = FC.label_codes(n, 200 + n)
        blob[f"in/{name}/indptr"], blob[f"in/{name}/indices"], blob[f"in/{name}/data"] = a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data
        blob[f"in/{name}/x"], blob[f"in/{name}/codes"] = x.toarray(), codes

        for kind, xin in (("csr", x), ("dense", x.toarray())):
            me = types.SimpleNamespace(spatial_connectivities_key="spatial_connectivities")
            blob[f"utag/{name}/{kind}"] = _dense(ns["utag"](me, _table(a.copy(), x=xin.copy())))
        for labels, column in (("categorical", FC.categorical(codes)), ("plain", FC.plain_labels(codes))):
            for distance, abs_nhood, weights in FC.PROFILE_SETTINGS:
                given = None if weights is None else list(weights)
                blob[f"profile/{name}/{labels}/{FC.setting_tag(distance, abs_nhood, weights)}"] = profile_embedding(ns, a, column, distance, abs_nhood, given)
                assert given == (None if weights is None else list(weights)), "the reference changed the caller's weights"
        if name not in FC.UNIT_GRAPHS:
            continue

        hop, vis = ns["_setdiag"](a, 0), ns["_setdiag"](a.copy(), 1)
        for k in (1, 2, 3):
            if k > 1:
                hop, vis = ns["_hop"](hop, a, vis)
            h, v = sps.csr_matrix(hop).astype(np.float64), sps.csr_matrix(vis).astype(np.float64)
            for m in (h, v):
                m.sum_duplicates()
                m.sort_indices()
            blob[f"shell/{name}/{k}/hop_indptr"], blob[f"shell/{name}/{k}/hop_indices"] = h.indptr.astype(np.int64), h.indices.astype(np.int32)
            blob[f"shell/{name}/{k}/vis_indptr"], blob[f"shell/{name}/{k}/vis_indices"] = v.indptr.astype(np.int64), v.indices.astype(np.int32)
            blob[f"shell/{name}/{k}/vis_counts"] = v.data.astype(np.int32)
            assert (h.data == 1).all() and (v.data == np.round(v.data)).all()
            norm = ns["_normalize"](hop)
            for aggregation in ("mean", "variance") if name in FC.AGGREGATE_GRAPHS else ():
                blob[f"agg/{name}/{aggregation}/{k}"] = _dense(ns["_aggregate"](_table(a, x=x), norm, aggregation))
        for aggregation in ("mean", "variance"):
            for kind, xin in (("csr", x), ("dense", x.toarray())):
                for distance in (1, 2, 3) if (name, aggregation) == ("knn", "mean") else (3,):
                    me = types.SimpleNamespace(distance=distance, aggregation=aggregation, spatial_connectivities_key="spatial_connectivities",
                                               n_components=10, use_rep=None)
                    try:
                        arr = _dense(ns["cellcharter"](me, _table(a.copy(), x=xin.copy())))
                    except (AttributeError, TypeError, ValueError) as exc:
                        assert kind == "dense", exc  # the literal source calls `.toarray()` on X for the variance
                        blob[f"cc_dense_ok/{name}/{aggregation}"] = np.array(False)
                        print(name, aggregation, kind, "not accepted by the literal source:", type(exc).__name__, flush=True)
                        break
                    if kind == "dense":
                        blob[f"cc_dense_ok/{name}/{aggregation}"] = np.array(True)
                    blob[f"cc/{name}/{aggregation}/{kind}/{distance}"] = arr
        print(name, n, "nnz", a.nnz, flush=True)
    blob["graphs"] = np.array(list(graphs))

    path = os.path.join(HERE, "niche_features_reference.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:  # np.savez stamps its members with the time of day: fixed stamps here
        for key in sorted(blob):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(blob[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote", path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
