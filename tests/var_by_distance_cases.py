"""Inputs shared by tests/golden/make_var_by_distance_golden.py and the var_by_distance tests: the design-matrix cases (a few
hundred rows each), the argument-error cases, and the point sets of the search tests with their numpy brute-force restatement."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

SLIDES = ("A", "B")


def table(n: int = 240, dim: int = 2, seed: int = 0) -> tuple[np.ndarray, pd.DataFrame]:
    """Coordinates in [0, 1000)^dim, labels c0..c3 (c3 in slide A only), two interleaved slides, one numeric covariate."""
    rng = np.random.default_rng(seed)
    coords = rng.random((n, dim)) * 1000.0
    lib = np.where((np.arange(n) // 7) % 2 == 0, "A", "B")
    cluster = rng.integers(0, 3, n)
    in_a = np.nonzero(lib == "A")[0]
    cluster[in_a[:: 5]] = 3
    obs = pd.DataFrame(
        {
            "cluster": pd.Categorical([f"c{c}" for c in cluster], categories=["c0", "c1", "c2", "c3"]),
            "lib": pd.Categorical(lib, categories=list(SLIDES)),
            "cov": rng.normal(size=n),
        },
        index=[f"cell_{i}" for i in range(n)],
    )
    return coords, obs


def frame_cases() -> list[dict]:
    """name, coords, obs, kwargs of var_by_distance (without adata / copy)."""
    out = []

    def add(name, kwargs, n=240, dim=2, seed=0, edit=None):
        coords, obs = table(n, dim, seed)
        if edit is not None:
            edit(coords, obs)
        out.append(dict(name=name, coords=coords, obs=obs, kwargs=kwargs))

    def with_nans(coords, obs):
        coords[5, 1] = np.nan  # a member of some group
        coords[17] = np.nan
        first_c1 = int(np.nonzero((obs["cluster"] == "c1").to_numpy())[0][0])
        coords[first_c1, 0] = np.nan  # an anchor member without coordinates

    add("single", dict(groups="c1", cluster_key="cluster"))
    add("two_anchors", dict(groups=["c0", "c2"], cluster_key="cluster"), seed=1)
    add("two_by_two_cov", dict(groups=["c0", "c3"], cluster_key="cluster", library_key="lib", covariates="cov"), seed=2)
    add("one_slide_only", dict(groups="c3", cluster_key="cluster", library_key="lib", covariates=["cov"]), seed=3)
    add("custom", dict(groups=[[310.5, 720.25]], cluster_key="cluster"), seed=4)
    add("custom_two_slides", dict(groups=[[100.0, 200.0], [900.0, 50.0]], library_key="lib"), seed=5)
    add("ndarray_library_id", dict(groups=np.array(["c0", "c1"]), cluster_key="cluster", library_key="lib", library_id=["B"]), seed=6)
    add("ndarray_library_id_str", dict(groups=np.array(["c2"]), cluster_key="cluster", library_key="lib", library_id="A"), seed=6)
    add("nan_rows", dict(groups=["c1", "c2"], cluster_key="cluster"), seed=7, edit=with_nans)
    add("nan_rows_slides", dict(groups="c1", cluster_key="cluster", library_key="lib"), seed=8, edit=with_nans)
    add("manhattan_3d", dict(groups=["c0", "c1"], cluster_key="cluster", metric="manhattan"), dim=3, seed=9)
    add("chebyshev_3d", dict(groups="c2", cluster_key="cluster", library_key="lib", metric="chebyshev"), dim=3, seed=10)
    add("custom_3d", dict(groups=[[500.0, 400.0, 30.0]], cluster_key="cluster", metric="euclidean"), dim=3, seed=11)
    add("key_and_cov", dict(groups="c0", cluster_key="cluster", covariates="cov", design_matrix_key="dm"), n=150, seed=12)
    return out


def error_cases() -> list[dict]:
    """name, kwargs: calls on ``table(120)`` that the reference refuses."""
    return [
        dict(name="groups_int", kwargs=dict(groups=5, cluster_key="cluster")),
        dict(name="groups_2d", kwargs=dict(groups=np.array([["c0", "c1"]]), cluster_key="cluster")),
        dict(name="library_key_int", kwargs=dict(groups="c0", cluster_key="cluster", library_key=3)),
        dict(name="library_id_unknown", kwargs=dict(groups="c0", cluster_key="cluster", library_key="lib", library_id=["A", "Z"])),
        dict(name="custom_count", kwargs=dict(groups=[[1.0, 2.0]], library_key="lib")),
        dict(name="metric_unknown", kwargs=dict(groups="c0", cluster_key="cluster", metric="nope")),
        dict(name="metric_not_kdtree", kwargs=dict(groups="c0", cluster_key="cluster", metric="canberra")),
        dict(name="anchor_nowhere", kwargs=dict(groups="zz", cluster_key="cluster")),
        dict(name="anchor_nowhere_slides", kwargs=dict(groups="zz", cluster_key="cluster", library_key="lib")),
    ]


# ------------------------------------------------------------------------------------------------ the golden file

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_by_distance_reference.npz")


def load_frame(z, prefix: str) -> pd.DataFrame:
    """A frame as make_var_by_distance_golden.store_frame wrote it."""
    data = {}
    columns = [str(c) for c in z[f"{prefix}/columns"]]
    for j, (name, dtype) in enumerate(zip(columns, z[f"{prefix}/dtypes"])):
        values, isna = z[f"{prefix}/col{j}/values"], z[f"{prefix}/col{j}/nan"]
        if str(dtype) == "category":
            data[name] = pd.Categorical(np.where(isna, None, values.astype(object)), categories=[str(c) for c in z[f"{prefix}/col{j}/categories"]])
        elif values.dtype.kind == "f":
            data[name] = values.astype(str(dtype))
        else:
            data[name] = np.where(isna, np.nan, values.astype(object))
    return pd.DataFrame(data, index=[str(i) for i in z[f"{prefix}/index"]], columns=columns)


def load_golden() -> dict:
    """{"signature": ..., "cases": {name: (coords, obs, kwargs, frame)}, "errors": {name: (type name, message)}}"""
    z = np.load(GOLDEN)
    cases = {}
    for name in z["cases"]:
        kwargs = {k: (np.array(v["ndarray"]) if isinstance(v, dict) else v) for k, v in json.loads(str(z[f"{name}/kwargs"])).items()}
        cases[str(name)] = (z[f"{name}/coords"], load_frame(z, f"{name}/obs"), kwargs, load_frame(z, f"{name}/frame"))
    errors = {str(n): (str(z[f"error/{n}/type"]), str(z[f"error/{n}/message"])) for n in z["error_cases"]}
    return dict(signature=json.loads(str(z["signature"])), cases=cases, errors=errors)


# ------------------------------------------------------------------------------------------------ the search

METRIC_NAMES = ("euclidean", "manhattan", "chebyshev")


def brute(coords, slide_codes, ref_coords, ref_sets, set_of, metric):
    """The arithmetic sklearn's KDTree performs, restated: differences accumulated in dimension order, every operation rounded on
    its own; the minimum per (anchor column, query); NaN without a slide, a set or a point."""
    coords, ref_coords = np.asarray(coords, dtype=np.float64), np.asarray(ref_coords, dtype=np.float64)
    set_of = np.asarray(set_of)
    out = np.full((set_of.shape[0], len(coords)), np.nan)
    for a in range(set_of.shape[0]):
        for s in range(set_of.shape[1]):
            rows = np.nonzero(np.asarray(slide_codes) == s)[0]
            ref = ref_coords[np.asarray(ref_sets) == set_of[a, s]] if set_of[a, s] >= 0 else ref_coords[:0]
            if len(rows) == 0 or len(ref) == 0:
                continue
            d = coords[rows, None, :] - ref[None, :, :]
            if metric == "euclidean":
                acc = d[..., 0] * d[..., 0]
                for k in range(1, d.shape[2]):
                    acc = acc + d[..., k] * d[..., k]
                out[a, rows] = np.sqrt(acc.min(axis=1))
            elif metric == "manhattan":
                acc = np.abs(d[..., 0])
                for k in range(1, d.shape[2]):
                    acc = acc + np.abs(d[..., k])
                out[a, rows] = acc.min(axis=1)
            else:
                out[a, rows] = np.abs(d).max(axis=2).min(axis=1)
    return out


def sklearn_search(coords, slide_codes, ref_coords, ref_sets, set_of, metric):
    """The same through ``KDTree(...).query``: what the reference computes per (anchor, slide)."""
    from sklearn.metrics import DistanceMetric
    from sklearn.neighbors import KDTree

    coords, ref_coords, set_of = np.asarray(coords, dtype=np.float64), np.asarray(ref_coords, dtype=np.float64), np.asarray(set_of)
    out = np.full((set_of.shape[0], len(coords)), np.nan)
    for a in range(set_of.shape[0]):
        for s in range(set_of.shape[1]):
            rows = np.nonzero(np.asarray(slide_codes) == s)[0]
            ref = ref_coords[np.asarray(ref_sets) == set_of[a, s]] if set_of[a, s] >= 0 else ref_coords[:0]
            if len(rows) and len(ref):
                out[a, rows] = KDTree(ref, metric=DistanceMetric.get_metric(metric)).query(coords[rows])[0][:, 0]
    return out


def hex_lattice(nx: int = 30, ny: int = 30, pitch: float = 100.0) -> np.ndarray:
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.column_stack([((i + 0.5 * (j % 2)) * pitch).ravel(), (j * pitch * np.sqrt(3.0) / 2.0).ravel()])


def _one_set(queries, ref):
    return dict(coords=queries, slide_codes=np.zeros(len(queries), np.int32), ref_coords=ref, ref_sets=np.zeros(len(ref), np.int32),
                set_of=np.zeros((1, 1), np.int32))


def _labelled(coords, labels, slides, n_labels, n_slides):
    """Every label an anchor column, every (label, slide) with members a set of its own; the members are the queries' own rows."""
    set_of = np.full((n_labels, n_slides), -1, np.int32)
    ref, sets = [], []
    for a in range(n_labels):
        for s in range(n_slides):
            rows = np.nonzero((labels == a) & (slides == s))[0]
            if len(rows):
                set_of[a, s] = len(ref)
                sets.append(np.full(len(rows), len(ref), np.int32))
                ref.append(coords[rows])
    return dict(coords=coords, slide_codes=slides.astype(np.int32), ref_coords=np.concatenate(ref), ref_sets=np.concatenate(sets), set_of=set_of)


def search_cases(threshold: int) -> list[tuple[str, dict]]:
    """The point sets of the search tests; ``threshold``: the set size from which a set gets a cell grid."""
    rng = np.random.default_rng(42)
    out = []
    out.append(("one_point", _one_set(np.array([[3.0, 4.0]]), np.array([[3.0, 4.0]]))))
    out.append(("two_identical", _one_set(np.array([[7.5, -2.0], [7.5, -2.0]]), np.array([[7.5, -2.0], [7.5, -2.0]]))))
    out.append(("257_against_one", _one_set(rng.random((257, 2)) * 1e4, np.array([[5000.0, 5000.0]]))))
    xy = rng.random((1000, 2)) * 1e4
    labels, slides = rng.integers(0, 4, 1000), rng.integers(0, 3, 1000)
    labels[(labels == 2) & (slides == 1)] = 0  # label 2 is missing from slide 1
    case = _labelled(xy, labels, slides, 4, 3)
    case["slide_codes"][::97] = -1  # and a few rows belong to no slide
    out.append(("uniform_4x3", case))
    hexa = hex_lattice()
    hex_labels = rng.integers(0, 3, len(hexa))
    out.append(("hex_lattice", _labelled(hexa, hex_labels, np.zeros(len(hexa), np.int64), 3, 1)))
    out.append(("hex_lattice_shifted", _labelled(hexa + 1e7, hex_labels, np.zeros(len(hexa), np.int64), 3, 1)))
    corner = hexa[(hexa[:, 0] < 300.0) & (hexa[:, 1] < 300.0)]
    dense = np.concatenate([corner, rng.random((600, 2)) * 290.0])  # a gridded set confined to one corner: most queries lie outside its box
    out.append(("corner", _one_set(np.concatenate([hexa, rng.random((300, 2)) * 3000.0 - 20.0]), dense)))
    out.append(("zero_extent", _one_set(xy[:300], np.tile(np.array([[1234.5, 6789.0]]), (threshold + 5, 1)))))
    for size in (threshold - 1, threshold, threshold + 1):
        out.append((f"set_of_{size}", _one_set(xy[:400], rng.random((size, 2)) * 1e4)))
    g = np.arange(12) * 50.0
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    out.append(("cubic_lattice", _labelled(cube, rng.integers(0, 3, len(cube)), np.zeros(len(cube), np.int64), 3, 1)))
    xyz = rng.random((2000, 3)) * np.array([1e4, 1e4, 300.0])
    out.append(("uniform_3d", _labelled(xyz, rng.integers(0, 3, 2000), rng.integers(0, 2, 2000), 3, 2)))
    return out
