"""Generates tests/golden/niche_reference.npz.  Run in the build container from the repository root:
    python tests/golden/make_niche_golden.py

- ``signature``: the reference's ``calculate_niche_cellcharter`` signature from the AST (gr/_niche.py:402-416).
- ``post/<case>/...``: small label vectors pushed through the reference's LITERAL ``_postprocess_niche_results``
  (gr/_niche.py:1494-1542, executed through ``oracle.ref_shim``): mask only, ``min_niche_size`` only, prefix only, all three, and a mask
  whose index is a superset of ``obs``.
- ``lib/...``: the LITERAL ``_calculate_niche_custom`` and ``_run_niche_pipeline`` (:623-733) with a stand-in embedder (the row
  positions) and a stand-in clusterer (writes ``pd.Categorical`` of given labels, as ``_GMMClusterer`` does) over three libraries of
  different sizes, with a mask and a ``min_niche_size``.
- ``e2e/...``: sklearn's labels of the case ``default10`` (tests/niche_cases.py, random_state 42) pushed through the literal
  post-processing with a mask and a ``min_niche_size``: what the GPU end-to-end test expects."""

from __future__ import annotations

import ast
import json
import logging
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shim  # noqa: E402

import niche_cases as NC  # noqa: E402

COLUMN = "cellcharter_niche"


class _Table:
    """Stands in for AnnData: ``obs``, selection by obs names, ``copy``."""

    def __init__(self, obs: pd.DataFrame):
        self.obs = obs

    def __getitem__(self, names):
        return _Table(self.obs.loc[names])

    def copy(self) -> "_Table":
        return _Table(self.obs.copy())


class _RowEmbedder:
    def get_embedding(self, adata: _Table) -> np.ndarray:
        return adata.obs["row"].to_numpy()


class _GivenLabels:
    """What ``_GMMClusterer.cluster`` does with the labels of a fit (gr/_niche.py:1482-1486), the fit replaced by given labels."""

    def __init__(self, labels: np.ndarray):
        self.labels = labels

    def cluster(self, adata: _Table, embedding: np.ndarray) -> list:
        adata.obs[COLUMN] = pd.Categorical(self.labels[embedding])
        return [COLUMN]


def _assert_key_in_adata(adata, key, *, attr, extra_msg=""):
    assert key in getattr(adata, attr)


def literal() -> dict:
    ns = {
        "np": np, "pd": pd, "logg": logging.getLogger("niche-golden"), "SpatialData": type("SpatialData", (), {}),
        "extract_adata_if_sdata": lambda data, table_key=None: data, "assert_key_in_adata": _assert_key_in_adata,
        "sanitize_table": lambda adata: None,
    }
    ref_shim._extract("gr/_niche.py", ["_postprocess_niche_results", "_run_niche_pipeline", "_calculate_niche_custom"], ns)
    return ns


def signature() -> str:
    src = open(os.path.join(ref_shim.REF_SRC, "gr", "_niche.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == "calculate_niche_cellcharter":
            a = node.args
            pos = [x.arg for x in a.args]
            defaults = [ast.unparse(d) for d in a.defaults]
            k = len(pos) - len(defaults)
            return json.dumps({
                "positional": [{"name": n, "default": defaults[i - k] if i >= k else None} for i, n in enumerate(pos)],
                "keyword_only": [{"name": x.arg, "default": ast.unparse(d) if d is not None else None} for x, d in zip(a.kwonlyargs, a.kw_defaults)],
            })
    raise RuntimeError("calculate_niche_cellcharter not found")


def post_cases() -> dict:
    """name -> (labels int64[n], obs names, mask values | None, mask index | None, min_niche_size | None, prefix | None)."""
    rng = np.random.default_rng(77)
    n = 60
    labels = rng.choice(5, size=n, p=[0.4, 0.3, 0.2, 0.07, 0.03]).astype(np.int64)
    names = np.array([f"cell{i}" for i in range(n)])
    mask = rng.random(n) < 0.7
    wide_names = np.concatenate([names[:30], [f"other{i}" for i in range(9)], names[30:]])  # obs order kept, strangers in between
    wide_mask = np.concatenate([mask[:30], rng.random(9) < 0.5, mask[30:]])
    return {
        "mask": (labels, names, mask, names, None, None),
        "min_size": (labels, names, None, None, 8, None),
        "prefix": (labels, names, None, None, None, "lib=A_"),
        "all": (labels, names, mask, names, 8, "lib=7_"),
        "superset": (labels, names, wide_mask, wide_names, None, None),
    }


def main() -> None:
    ns = literal()
    blob: dict[str, np.ndarray] = {"signature": np.array(signature())}
    post_names = []
    for name, (labels, names, mvals, mindex, min_size, prefix) in post_cases().items():
        table = _Table(pd.DataFrame({COLUMN: pd.Categorical(labels)}, index=names))
        mask = None if mvals is None else pd.Series(mvals, index=mindex)
        ns["_postprocess_niche_results"](table, [COLUMN], mask, min_size, prefix)
        blob[f"post/{name}/labels"] = labels
        blob[f"post/{name}/names"] = names
        blob[f"post/{name}/mask"] = np.zeros(0, dtype=bool) if mvals is None else mvals
        blob[f"post/{name}/mask_index"] = np.zeros(0, dtype=str) if mindex is None else mindex
        blob[f"post/{name}/min_size"] = np.array(-1 if min_size is None else min_size)
        blob[f"post/{name}/prefix"] = np.array("" if prefix is None else prefix)
        blob[f"post/{name}/expected"] = table.obs[COLUMN].to_numpy().astype(str)
        post_names.append(name)
        print(name, dict(zip(*np.unique(blob[f"post/{name}/expected"], return_counts=True))), flush=True)
    blob["post_cases"] = np.array(post_names)

    # the library loop: three libraries of sizes 25, 50 and 15 in interleaved order, labels given per row
    rng = np.random.default_rng(78)
    n = 90
    lib = rng.permutation(np.repeat(["s2", "s0", "s1"], [25, 50, 15]))
    labels = rng.choice(4, size=n, p=[0.5, 0.3, 0.15, 0.05]).astype(np.int64)
    names = np.array([f"cell{i}" for i in range(n)])
    mask = rng.random(n) < 0.8
    for tag, kw in {"plain": {}, "mask_min": {"mask": pd.Series(mask, index=names), "min_niche_size": 4}}.items():
        table = _Table(pd.DataFrame({"library": pd.Categorical(lib), "row": np.arange(n)}, index=names))
        ns["_calculate_niche_custom"](table, _RowEmbedder(), _GivenLabels(labels), library_key="library", inplace=True, **kw)
        blob[f"lib/{tag}/expected"] = table.obs[COLUMN].to_numpy().astype(str)
        print("lib", tag, dict(zip(*np.unique(blob[f"lib/{tag}/expected"], return_counts=True))), flush=True)
    blob.update({"lib/library": lib.astype(str), "lib/labels": labels, "lib/names": names, "lib/mask": mask, "lib/min_size": np.array(4)})

    # end to end: sklearn's labels of default10 through the literal post-processing
    ref = NC.reference("default10", 42)
    n = len(ref.labels)
    names = np.array([str(i) for i in range(n)])
    mask = np.random.default_rng(79).random(n) < 0.9
    min_size = int(np.sort(np.bincount(ref.labels))[2]) + 1  # the three smallest niches (before masking) fall below it
    table = _Table(pd.DataFrame({COLUMN: pd.Categorical(ref.labels)}, index=names))
    ns["_postprocess_niche_results"](table, [COLUMN], pd.Series(mask, index=names), min_size, None)
    blob.update({"e2e/mask": mask, "e2e/min_size": np.array(min_size), "e2e/expected": table.obs[COLUMN].to_numpy().astype(str)})
    print("e2e", min_size, dict(zip(*np.unique(blob["e2e/expected"], return_counts=True))), flush=True)

    path = os.path.join(HERE, "niche_reference.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
