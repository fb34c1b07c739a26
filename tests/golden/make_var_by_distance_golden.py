"""Generates tests/golden/var_by_distance_reference.npz.  Run in the build container from the repository root:
    python tests/golden/make_var_by_distance_golden.py

Per case of ``tests/var_by_distance_cases.frame_cases()``: the inputs (coordinates, the obs columns, the arguments as JSON) and the
frame the reference's LITERAL ``var_by_distance`` (tl/_var_by_distance.py, executed through ``oracle.ref_shim`` with sklearn's own
KDTree) returns for them — column names, dtypes as strings, the index, the values and their NaN masks; once with ``copy=True`` and
once through ``obsm[design_matrix_key]``, which must agree.  Per case of ``error_cases()``: the exception's type and message.
Also: the reference's signature from the AST.  Data only — none of the reference's text is stored."""

from __future__ import annotations

import ast
import json
import os
import sys
from functools import reduce
from itertools import product
from typing import Any, cast

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shim  # noqa: E402
from squidpy_amd import AnnDataLite  # noqa: E402

import var_by_distance_cases as VC  # noqa: E402


class _Adata(AnnDataLite):
    """``adata[mask]`` with a single boolean mask over the observations, as the reference slices a slide out."""

    def __getitem__(self, key: Any) -> "_Adata":
        if isinstance(key, tuple):
            sub = super().__getitem__(key)
        else:
            rows = np.nonzero(key.to_numpy() if isinstance(key, pd.Series) else np.asarray(key))[0]
            sub = AnnDataLite(obs=self.obs.iloc[rows].copy(), obsm={k: np.asarray(v)[rows] for k, v in self.obsm.items()})
        return _Adata(obs=sub.obs, obsm=sub.obsm)


class _Logg:
    @staticmethod
    def info(*_a: Any, **_k: Any) -> None:
        return None


def _save_data(adata: Any, *, attr: str, key: str, data: Any, time: Any = None) -> None:
    getattr(adata, attr)[key] = data


def literal() -> Any:
    from sklearn.metrics import DistanceMetric
    from sklearn.neighbors import KDTree

    ns = {"np": np, "pd": pd, "reduce": reduce, "product": product, "cast": cast, "Any": Any, "KDTree": KDTree, "DistanceMetric": DistanceMetric,
          "logg": _Logg, "_save_data": _save_data, "AnnData": None, "NDArrayA": None, "Iterator": None, "d": None}
    ref_shim._extract("tl/_var_by_distance.py", ["var_by_distance", "_init_design_matrix", "_get_coordinates", "_normalize_distances"], ns)
    return ns["var_by_distance"]


def signature() -> str:
    src = open(os.path.join(ref_shim.REF_SRC, "tl", "_var_by_distance.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == "var_by_distance":
            a = node.args
            pos = [x.arg for x in a.args]
            defaults = [ast.unparse(d) for d in a.defaults]
            k = len(pos) - len(defaults)
            return json.dumps({
                "positional": [{"name": n, "default": defaults[i - k] if i >= k else None} for i, n in enumerate(pos)],
                "keyword_only": [{"name": x.arg, "default": ast.unparse(d) if d is not None else None} for x, d in zip(a.kwonlyargs, a.kw_defaults)],
            })
    raise RuntimeError("var_by_distance not found")


def jsonable(kwargs: dict) -> str:
    return json.dumps({k: ({"ndarray": v.tolist()} if isinstance(v, np.ndarray) else v) for k, v in kwargs.items()})


def store_frame(blob: dict, prefix: str, df: pd.DataFrame) -> None:
    blob[f"{prefix}/columns"] = np.array([str(c) for c in df.columns])
    blob[f"{prefix}/dtypes"] = np.array([str(t) for t in df.dtypes])
    blob[f"{prefix}/index"] = np.array([str(i) for i in df.index])
    for j, c in enumerate(df.columns):
        col = df[c]
        isna = col.isna().to_numpy()
        blob[f"{prefix}/col{j}/nan"] = isna
        if isinstance(col.dtype, pd.CategoricalDtype):
            blob[f"{prefix}/col{j}/categories"] = np.array([str(x) for x in col.cat.categories])
            blob[f"{prefix}/col{j}/values"] = np.array(["" if m else str(v) for v, m in zip(col.to_numpy(dtype=object), isna)])
        elif col.dtype.kind in "fiu":
            blob[f"{prefix}/col{j}/values"] = col.to_numpy(dtype=np.float64)
        else:
            blob[f"{prefix}/col{j}/values"] = np.array(["" if m else str(v) for v, m in zip(col.to_numpy(dtype=object), isna)])


def main() -> None:
    import sklearn

    run = literal()
    blob: dict[str, np.ndarray] = {"signature": np.array(signature()), "sklearn": np.array(sklearn.__version__), "pandas": np.array(pd.__version__)}
    names = []
    for c in VC.frame_cases():
        name, kwargs = c["name"], c["kwargs"]
        adata = _Adata(obs=c["obs"].copy(), obsm={"spatial": c["coords"].copy()})
        df = run(adata, copy=True, **kwargs)
        adata2 = _Adata(obs=c["obs"].copy(), obsm={"spatial": c["coords"].copy()})
        assert run(adata2, **kwargs) is None
        pd.testing.assert_frame_equal(adata2.obsm[kwargs.get("design_matrix_key", "design_matrix")], df, check_exact=True)
        pd.testing.assert_frame_equal(adata.obs, c["obs"], check_exact=True)  # the call leaves obs alone
        blob[f"{name}/coords"] = c["coords"]
        blob[f"{name}/kwargs"] = np.array(jsonable(kwargs))
        store_frame(blob, f"{name}/obs", c["obs"])
        store_frame(blob, f"{name}/frame", df)
        names.append(name)
        print(name, df.shape, list(df.columns), flush=True)
    blob["cases"] = np.array(names)
    errors = []
    coords, obs = VC.table(120)
    for c in VC.error_cases():
        try:
            run(_Adata(obs=obs.copy(), obsm={"spatial": coords.copy()}), copy=True, **c["kwargs"])
        except Exception as e:  # noqa: BLE001
            blob[f"error/{c['name']}/type"] = np.array(type(e).__name__)
            blob[f"error/{c['name']}/message"] = np.array(str(e))
            errors.append(c["name"])
            print(c["name"], type(e).__name__, str(e)[:100], flush=True)
        else:
            raise RuntimeError(f"the reference accepts error case {c['name']}")
    blob["error_cases"] = np.array(errors)
    path = os.path.join(HERE, "var_by_distance_reference.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
