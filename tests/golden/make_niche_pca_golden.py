"""Generates tests/golden/niche_pca_reference.npz.  Run in the build container from the repository root:
    python tests/golden/make_niche_pca_golden.py

For every chain case of tests/niche_pca_cases.py the reference's LITERAL embedder code (``_CellcharterEmbedder.get_embedding``,
gr/_niche.py:1336-1355, compiled from the reference's source at run time through ``oracle/ref_shim.py`` exactly as
tests/golden/make_niche_features_golden.py does, with stand-ins that capture the matrix handed to ``sc.tl.pca``) builds the feature
matrix, per library on ``adj[rows][:, rows]`` and ``X[rows]`` as ``adata[lib_indices].copy()`` would; then sklearn's
``PCA(svd_solver="arpack", random_state=0)`` with scanpy's default number of components and sklearn's ``GaussianMixture`` run on it in
float64.  Stored per case: the labels, ``n_iter_`` and ``converged_`` of every library, the smallest weighted-log-density margin, and
the largest difference between the literal features and the numpy restatement (tests/niche_features_oracle.py).  No reference text is
kept here or in the fixture."""

from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_niche_features_golden as MF  # noqa: E402

from tests import niche_features_oracle as FO  # noqa: E402
from tests import niche_pca_cases as PC  # noqa: E402


def main() -> None:
    import logging

    logging.getLogger("niche-features-golden").setLevel(logging.ERROR)
    ns = MF.literal()
    worst = {}

    def literal_features(graph, x, distance):
        me = types.SimpleNamespace(distance=distance, aggregation="mean", spatial_connectivities_key="spatial_connectivities", n_components=10,
                                   use_rep=None)
        from scipy import sparse

        arr = MF._dense(ns["cellcharter"](me, MF._table(graph.copy(), x=sparse.csr_matrix(x))))
        restated = FO.cellcharter(graph, x, distance, "mean")
        worst[name] = max(worst.get(name, 0.0), float(np.abs(arr - restated).max()))
        return arr

    blob: dict[str, np.ndarray] = {}
    for name in PC.CHAIN_NAMES:
        ref = PC.sklearn_chain(literal_features, name)
        assert ref.margin >= PC.MIN_MARGIN, (name, ref.margin)
        blob[f"{name}/labels"] = ref.labels.astype(np.int32)
        blob[f"{name}/n_iter"] = np.array(ref.n_iter, dtype=np.int32)
        blob[f"{name}/converged"] = np.array(ref.converged)
        blob[f"{name}/margin"] = np.array(ref.margin)
        blob[f"{name}/features_max_abs_diff"] = np.array(worst[name])
        print(name, "margin", ref.margin, "n_iter", ref.n_iter, "converged", ref.converged, "literal vs restated features", worst[name], flush=True)
    blob["chains"] = np.array(list(PC.CHAIN_NAMES))

    path = os.path.join(HERE, "niche_pca_reference.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:  # np.savez stamps its members with the time of day: fixed stamps here
        for key in sorted(blob):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(blob[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote", path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
