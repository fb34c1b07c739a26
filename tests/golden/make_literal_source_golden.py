"""Generates tests/golden/literal_source_cases.npz by executing the reference's OWN source through oracle/ref_shim.py on the
fresh inputs of three tests that used to call that source directly.  Needs the reference tree (build container only).

    python tests/golden/make_literal_source_golden.py

Cases (inputs and outputs are stored, so the tests need the reference tree no more):
  ligrec_fresh   tests/test_ligrec_cpu.py::test_oracle_matches_literal_reference_source — `_analysis` on 180 cells x 10 genes,
                 5 clusters, threshold 0.4, 40 perms, seed 9
  ligrec_single  tests/test_ligrec_cpu.py::test_single_cluster_subset_is_computed_like_the_reference — `_analysis` on the cells
                 of cluster "0" of that test's fixture, one cluster pair (0, 0), threshold 0.2, 7 perms, seed 1
  nhood / occur  tests/test_oracle_pinned.py::test_restatement_equals_literal_source_on_fresh_inputs — the nhood count kernel
                 (`create_function(3)`) on a random 120-node graph and `_occur_count` on 90 random points
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402


def _analysis(ns, data, cl, inter, cp, threshold, n_perms, seed):
    df = pd.DataFrame(data, columns=list(range(data.shape[1])))
    df["clusters"] = pd.Categorical(cl)
    res = ns["_analysis"](df, inter, cp, threshold=threshold, n_perms=n_perms, seed=seed, n_jobs=1, show_progress_bar=False)
    return np.asarray(res.means), np.asarray(res.pvalues)


def single_cluster_inputs():
    """The cells of cluster "0" and the interactions of test_single_cluster_subset_is_computed_like_the_reference (its
    `adata` / `pairs` fixtures; the interactions are the 25 ordered pairs of the first 5 raw genes, in the order
    PermutationTest keeps them)."""
    rng = np.random.default_rng(0)
    n, g = 60, 16
    x = sp.csr_matrix((rng.random((n, g)) < 0.5) * rng.gamma(2.0, 1.0, (n, g)))
    leiden = rng.integers(0, 3, n).astype(str)
    keep = leiden == "0"
    data = x.toarray()[:, :5][keep]
    inter = np.array([(a, b) for a in range(5) for b in range(5)], dtype=np.int32)
    return data, inter


def main() -> None:
    assert ref_shim.available(), "reference tree not mounted"
    ns = ref_shim.ligrec()
    out: dict[str, np.ndarray] = {}

    rng = np.random.default_rng(3)
    n, g, k = 180, 10, 5
    data = (rng.random((n, g)) < 0.4) * rng.gamma(2.0, 1.0, (n, g))
    cl = rng.integers(0, k, n).astype(np.int32)
    inter = np.array([(i, j) for i in range(g) for j in range(g)], dtype=np.int32)[::4]
    cp = np.array([(a, b) for a in range(k) for b in range(k)], dtype=np.int32)[::2]
    means, pvals = _analysis(ns, data, cl, inter, cp, 0.4, 40, 9)
    out.update({"ligrec_fresh_data": data, "ligrec_fresh_clusters": cl, "ligrec_fresh_interactions": inter, "ligrec_fresh_cpairs": cp,
                "ligrec_fresh_means": means, "ligrec_fresh_pvalues": pvals})

    data, inter = single_cluster_inputs()
    cp = np.array([(0, 0)], dtype=np.int32)
    means, pvals = _analysis(ns, data, np.zeros(len(data), dtype=np.int32), inter, cp, 0.2, 7, 1)
    out.update({"ligrec_single_data": data, "ligrec_single_interactions": inter, "ligrec_single_means": means, "ligrec_single_pvalues": pvals})

    rng = np.random.default_rng(11)
    n, k = 120, 3
    A = sp.random(n, n, density=0.05, format="csr", random_state=5)
    labels = rng.integers(0, k, n).astype(np.uint32)
    indices, indptr = A.indices.astype(np.uint32), A.indptr.astype(np.uint32)
    out.update({"nhood_indices": indices, "nhood_indptr": indptr, "nhood_labels": labels, "nhood_k": np.int64(k),
                "nhood_count": np.asarray(ref_shim.nhood()["create_function"](k)(indices, indptr, labels))})
    pp = ref_shim.ppatterns()
    x, y = (rng.random(90) * 30).astype(np.float32), (rng.random(90) * 30).astype(np.float32)
    labs = rng.integers(0, k, 90).astype(np.int32)
    thr = (np.linspace(1, 20, 7, dtype=np.float32)) ** 2
    out.update({"occur_x": x, "occur_y": y, "occur_thresholds": thr, "occur_labs": labs,
                "occur_counts": np.asarray(pp["_occur_count"](x, y, thr, labs, 90, k, len(thr)))})

    path = os.path.join(ROOT, "tests", "golden", "literal_source_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
