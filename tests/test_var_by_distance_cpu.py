"""CPU: what ``sq.tl.var_by_distance`` decides before it reaches the device — the signature, the argument errors, the assembly of
the design matrix (fed distances from sklearn through the ``search`` argument) against the reference's frames
(tests/golden/var_by_distance_reference.npz) — and the search itself: the kernel's query body is host-callable, so the grid
layout and the ring walk run here on the host (tests/anchor_host_twin.hip): the distances against brute force and sklearn, and
the walk's own counters — rings entered, cells reached, cells read — against what the geometry of each query allows."""

from __future__ import annotations

import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import squidpy_amd as sq
from squidpy_amd import _build, _lib
from squidpy_amd.tl import _var_by_distance as V
from tests import var_by_distance_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


def _adata(coords, obs):
    return sq.AnnDataLite(obs=obs.copy(), obsm={"spatial": np.array(coords, copy=True)})


def test_signature_is_the_references_plus_device(golden):
    sig = inspect.signature(sq.tl.var_by_distance)
    positional = [p for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional] == [p["name"] for p in golden["signature"]["positional"]]
    for p, ref in zip(positional, golden["signature"]["positional"]):
        assert (None if p.default is p.empty else repr(p.default).replace('"', "'")) == (None if ref["default"] is None else ref["default"].replace('"', "'")), p.name
    assert golden["signature"]["keyword_only"] == []
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY] == [("device", None)]


def test_both_entry_points_are_bound():
    assert _lib.SIGNATURES["sqgr_anchor_dist_hook"][1][:-2] == _lib.SIGNATURES["sqgr_anchor_dist"][1]
    info = _lib.anchor_dist_info()
    assert info["brute_below"] >= 2 and info["per_cell"] >= 1 and info["max_dim"] == 3


@pytest.mark.parametrize("name", [c["name"] for c in cases.error_cases()])
def test_argument_errors_come_before_any_device_call(golden, name, monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "anchor_distances", no_device)
    monkeypatch.setattr(_lib, "default_context", no_device)
    kwargs = next(c["kwargs"] for c in cases.error_cases() if c["name"] == name)
    type_name, message = golden["errors"][name]
    coords, obs = cases.table(120)
    with pytest.raises(Exception) as err:
        sq.tl.var_by_distance(_adata(coords, obs), copy=True, **kwargs)
    assert type(err.value).__name__ == type_name, err.value
    if name in ("groups_int", "groups_2d", "library_key_int", "library_id_unknown", "custom_count"):  # the reference's own checks
        assert str(err.value) == message
    else:  # sklearn's and pandas' complaints in the reference: here a message that names the problem
        assert ("metric" in str(err.value)) if name.startswith("metric") else ("zz" in str(err.value))


@pytest.mark.parametrize("shape", [(30, 4), (30, 1), (30,)])
def test_other_widths_are_refused_by_name(shape):
    with pytest.raises(ValueError, match=r"Expected coordinates of shape \(n, 2\) or \(n, 3\), found"):
        _lib.anchor_distances(None, np.zeros(shape), np.zeros(30, np.int32), np.zeros((1, 2)), np.zeros(1, np.int32), np.zeros((1, 1), np.int32))
    with pytest.raises(ValueError, match=r"Expected coordinates of shape \(n, 2\) or \(n, 3\), found"):
        sq.tl.anchor_distances(np.zeros(shape), np.zeros(30), [0])
    with pytest.raises(ValueError, match="is not valid for KDTree"):
        _lib.anchor_distances(None, np.zeros((30, 2)), np.zeros(30, np.int32), np.zeros((1, 2)), np.zeros(1, np.int32), np.zeros((1, 1), np.int32), "canberra")


def test_no_device_no_result(golden):
    """There is no CPU path for the search: without a device the call raises as every other entry point does."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    coords, obs, kwargs, _ = golden["cases"]["single"]
    with pytest.raises(_lib.SqgrError):
        sq.tl.var_by_distance(_adata(coords, obs), copy=True, **kwargs)


# ------------------------------------------------------------------------------------------------ the frame assembly


def test_golden_holds_every_case(golden):
    assert list(golden["cases"]) == [c["name"] for c in cases.frame_cases()]
    assert sorted(golden["errors"]) == sorted(c["name"] for c in cases.error_cases())
    for c in cases.frame_cases():  # the stored inputs are the generator's
        coords, obs, _, _ = golden["cases"][c["name"]]
        np.testing.assert_array_equal(coords, c["coords"])
        pd.testing.assert_frame_equal(obs, c["obs"], check_exact=True)


@pytest.mark.parametrize("name", [c["name"] for c in cases.frame_cases()])
def test_assembly_reproduces_the_reference_frames(golden, name):
    coords, obs, kwargs, want = golden["cases"][name]
    calls = []

    def search(*args):
        calls.append(1)
        return cases.sklearn_search(*args)

    kw = dict(cluster_key=None, library_key=None, library_id=None, covariates=None, metric="euclidean", spatial_key="spatial")
    kw.update({k: v for k, v in kwargs.items() if k != "design_matrix_key"})
    adata = _adata(coords, obs)
    got = V._design_matrix(adata, search=search, **kw)
    assert len(calls) == 1  # one search for all anchors and slides
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    pd.testing.assert_frame_equal(adata.obs, obs, check_exact=True)


def test_spatial_key_names_the_coordinates(golden):
    """The documented divergence: ``spatial_key`` is where the coordinates are read from, too."""
    coords, obs, kwargs, want = golden["cases"]["single"]
    adata = sq.AnnDataLite(obs=obs.copy(), obsm={"other": coords.copy()})
    got = V._design_matrix(adata, kwargs["groups"], kwargs["cluster_key"], None, None, None, "euclidean", "other", cases.sklearn_search)
    pd.testing.assert_frame_equal(got, want, check_exact=True)


# ------------------------------------------------------------------------------------ the search itself, on the CPU

f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class Twin:
    """tests/anchor_host_twin.hip: the kernel's query body over grids laid out by the library's planner, run on the host"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.twin_anchor.argtypes = [C.c_int, C.c_int, f64p, C.c_int64, f64p, i32p, C.c_int64, C.c_int32, C.c_int64, C.c_double, f64p, i64p, f64p]

    def search(self, coords, slide_codes, ref_coords, ref_sets, set_of, metric, brute_below=None, per_cell=None):
        """-> (distances (n_columns, n) as the library defines them, walks (n_sets, n, 3) = rings entered, cells of the runs the loops
        reached (pruned or not), cells read; grids (n_sets, 8) = cells per axis, points, cell side, lower corner)"""
        info = _lib.anchor_dist_info()
        q, r = np.ascontiguousarray(coords, np.float64), np.ascontiguousarray(ref_coords, np.float64)
        sets = np.ascontiguousarray(ref_sets, np.int32)
        n_sets = int(np.max(set_of)) + 1
        d, seen, grids = np.zeros((n_sets, len(q))), np.zeros((n_sets, len(q), 3), np.int64), np.zeros((n_sets, 8))
        rc = self.lib.twin_anchor(q.shape[1], _lib.METRICS[metric], q.ctypes.data_as(f64p), len(q), r.ctypes.data_as(f64p), sets.ctypes.data_as(i32p), len(r),
                                  n_sets, brute_below or info["brute_below"], float(per_cell or info["per_cell"]), d.ctypes.data_as(f64p),
                                  seen.ctypes.data_as(i64p), grids.ctypes.data_as(f64p))
        assert rc == 0
        out = np.full((set_of.shape[0], len(q)), np.nan)
        for a in range(set_of.shape[0]):
            for s in range(set_of.shape[1]):
                rows = np.nonzero(np.asarray(slide_codes) == s)[0]
                if set_of[a, s] >= 0:
                    out[a, rows] = d[set_of[a, s], rows]
        return out, seen, grids


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    lib = _build.build(verbose=False)  # set_error lives in libsqgr.so
    out = str(tmp_path_factory.mktemp("twin") / "libanchor_twin.so")
    subprocess.check_call([_build._hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           os.path.join(ROOT, "tests", "anchor_host_twin.hip"), "-I", _build.CSRC, "-I", os.path.join(ROOT, "include"),
                           "-o", out, "-L", _build.CSRC, "-lsqgr", "-Wl,-rpath," + os.path.dirname(lib), "-Wno-unused-function"])
    return Twin(out)


@pytest.fixture(scope="module")
def search_cases():
    """name -> (case, {metric: brute force}): computed once, shared, never written to"""
    out = {}
    for name, case in cases.search_cases(_lib.anchor_dist_info()["brute_below"]):
        out[name] = (case, {m: cases.brute(**case, metric=m) for m in cases.METRIC_NAMES})
    return out


CASE_NAMES = ["one_point", "two_identical", "257_against_one", "uniform_4x3", "hex_lattice", "hex_lattice_shifted", "corner", "zero_extent",
              "set_of_below", "set_of_at", "set_of_above", "cubic_lattice", "uniform_3d"]


def _case(search_cases, name):
    t = _lib.anchor_dist_info()["brute_below"]
    return search_cases[{"set_of_below": f"set_of_{t - 1}", "set_of_at": f"set_of_{t}", "set_of_above": f"set_of_{t + 1}"}.get(name, name)]


def test_case_list_is_complete(search_cases):
    assert len(search_cases) == len(CASE_NAMES)


@pytest.mark.parametrize("metric", cases.METRIC_NAMES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_twin_equals_brute_force_and_sklearn(twin, search_cases, name, metric):
    case, want = _case(search_cases, name)
    got, _, grids = twin.search(**case, metric=metric)
    np.testing.assert_array_equal(got, want[metric])
    np.testing.assert_array_equal(got, cases.sklearn_search(**case, metric=metric))
    # a grid of one cell and finer grids than the default: every route gives the same bytes
    for brute_below, per_cell in ((10**9, None), (2, 1.0), (2, 8.0)):
        np.testing.assert_array_equal(twin.search(**case, metric=metric, brute_below=brute_below, per_cell=per_cell)[0], want[metric])


def test_threshold_is_the_seam_between_one_cell_and_a_grid(twin, search_cases):
    for name, gridded in (("set_of_below", False), ("set_of_at", True), ("set_of_above", True)):
        case, _ = _case(search_cases, name)
        _, _, grids = twin.search(**case, metric="euclidean")
        assert (grids[0, :3].prod() > 1) == gridded, (name, grids)
    case, _ = _case(search_cases, "zero_extent")
    assert twin.search(**case, metric="euclidean")[2][0, :3].tolist() == [1, 1, 1]  # identical points: one cell whatever their number


def _rings_allowed(coords, grid, metric, nearest):
    """Per query of a 2-D set, from the geometry alone: the rings an exact walk needs at most, and the rings of the grid (rmax + 1).
    A cell can matter only if the gap from the query to its box, in the metric, does not exceed the distance to the nearest point
    (edge cells taken as unbounded outwards, 1e-6 cell sides of tolerance for the walk's rounding slack: both make the allowance
    larger).  Once the block of rings 0 .. R covers every such cell, the best value is final and every face of the block has only
    farther cells behind it, so the walk has to end with ring R."""
    gx, gy, h, o = int(grid[0]), int(grid[1]), grid[4], grid[5:7]
    u = coords - o
    c = np.clip(np.floor(u * (1.0 / h)), 0, [gx - 1, gy - 1]).astype(np.int64)
    gaps, rho = [], []
    for axis, g in enumerate((gx, gy)):
        k = np.arange(g)
        lo = np.where(k == 0, -np.inf, k * h)
        hi = np.where(k == g - 1, np.inf, (k + 1) * h)
        gaps.append(np.maximum(np.maximum(lo[None, :] - u[:, axis, None], u[:, axis, None] - hi[None, :]), 0.0))
        rho.append(np.abs(k[None, :] - c[:, axis, None]))
    ax, ay = gaps[0][:, :, None], gaps[1][:, None, :]
    lb = {"euclidean": np.sqrt(ax * ax + ay * ay), "manhattan": ax + ay, "chebyshev": np.maximum(ax, ay)}[metric]
    ring = np.maximum(rho[0][:, :, None], rho[1][:, None, :])
    needed = lb <= (nearest + 1e-6 * h)[:, None, None]
    rmax = np.maximum(np.maximum(c[:, 0], gx - 1 - c[:, 0]), np.maximum(c[:, 1], gy - 1 - c[:, 1]))
    return np.where(needed, ring, 0).max(axis=(1, 2)) + 1, rmax + 1


@pytest.mark.parametrize("metric", cases.METRIC_NAMES)
def test_walk_of_outside_queries_is_bounded_by_their_geometry(twin, search_cases, metric):
    """An anchor confined to one corner: most queries lie outside its bounding box.  The counters are the walk's own: rings entered
    (not cells read — pruning alone keeps those low), cells of every run the loops reach, pruned or not, and cells read.  No outside
    query may enter more rings than its geometry allows, which for most of them is fewer than the grid has (a walk without the stop
    rule enters all of them), and none may reach as many cells as the grid holds."""
    case, want = _case(search_cases, "corner")
    got, walks, grids = twin.search(**case, metric=metric, brute_below=2, per_cell=2.0)
    np.testing.assert_array_equal(got, want[metric])
    gx, gy = int(grids[0, 0]), int(grids[0, 1])
    assert gx >= 16 and gy >= 16, grids
    outside = (case["coords"] > case["ref_coords"].max(axis=0)).any(axis=1) | (case["coords"] < case["ref_coords"].min(axis=0)).any(axis=1)
    assert outside.sum() > 800
    allowed, all_rings = _rings_allowed(case["coords"], grids[0], metric, want[metric][0])
    rings, reached, read = walks[0, :, 0], walks[0, :, 1], walks[0, :, 2]
    print(metric, "rings max", int(rings[outside].max()), "allowed max", int(allowed[outside].max()), "of", int(all_rings[outside].max()),
          "| reached max", int(reached[outside].max()), "read max", int(read[outside].max()), "of", gx * gy, "cells",
          "| share of outside queries allowed fewer rings than the grid has:", float((allowed < all_rings)[outside].mean()))
    assert (allowed < all_rings)[outside].sum() >= 100  # the case has teeth: a walk that never stops early enters every ring and fails the next line on these
    assert (rings <= allowed)[outside].all(), np.nonzero(outside & (rings > allowed))[0][:10]
    assert (rings <= allowed).all()  # (inside queries too)
    assert reached[outside].max() < gx * gy and read[outside].max() < gx * gy
    assert (read <= reached).all()


def test_odd_clouds_in_the_host_twin(twin):
    """Scales from 1e-3 to 1e5 per axis, large offsets, rounded coordinates (ties), queries far away from the set."""
    for seed in range(6):
        rng = np.random.default_rng(200 + seed)
        dim = 2 + seed % 2
        ref = rng.random((int(rng.integers(70, 900)), dim)) * 10.0 ** rng.integers(-3, 6, dim) + 10.0 ** rng.integers(0, 7)
        q = np.concatenate([ref[::3], ref.mean(axis=0) + (rng.random((200, dim)) - 0.5) * 4.0 * np.ptp(ref, axis=0), ref[:20] * 1e3])
        if seed % 3 == 0:
            ref, q = np.round(ref, 1), np.round(q, 1)
        case = dict(coords=q, slide_codes=np.zeros(len(q), np.int32), ref_coords=ref, ref_sets=np.zeros(len(ref), np.int32), set_of=np.zeros((1, 1), np.int32))
        for metric in cases.METRIC_NAMES:
            np.testing.assert_array_equal(twin.search(**case, metric=metric)[0], cases.brute(**case, metric=metric))
