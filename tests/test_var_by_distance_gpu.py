"""GPU tests of ``sq.tl.var_by_distance``: the device search of ``csrc/sqgr_anchor.hip`` against a numpy brute-force restatement of
sklearn's KD-tree arithmetic and against ``KDTree.query`` itself — every (row, anchor) compared, every comparison an equality — and
the whole function against the reference's frames (tests/golden/var_by_distance_reference.npz)."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

from tests import var_by_distance_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


@pytest.fixture(scope="module")
def search_cases(L):
    """name -> (case, {metric: brute force}): computed once, shared, never written to"""
    out = {}
    for name, case in cases.search_cases(L.anchor_dist_info()["brute_below"]):
        out[name] = (case, {m: cases.brute(**case, metric=m) for m in cases.METRIC_NAMES})
    return out


CASE_NAMES = ["one_point", "two_identical", "257_against_one", "uniform_4x3", "hex_lattice", "hex_lattice_shifted", "corner", "zero_extent",
              "set_of_below", "set_of_at", "set_of_above", "cubic_lattice", "uniform_3d"]


def _case(L, search_cases, name):
    t = L.anchor_dist_info()["brute_below"]
    return search_cases[{"set_of_below": f"set_of_{t - 1}", "set_of_at": f"set_of_{t}", "set_of_above": f"set_of_{t + 1}"}.get(name, name)]


def _adata(coords, obs):
    import squidpy_amd as sq

    return sq.AnnDataLite(obs=obs.copy(), obsm={"spatial": np.array(coords, copy=True)})


def test_case_list_is_complete(search_cases):
    assert len(search_cases) == len(CASE_NAMES)


@pytest.mark.parametrize("metric", cases.METRIC_NAMES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_search_equals_brute_force_and_sklearn(L, ctx, search_cases, name, metric):
    case, want = _case(L, search_cases, name)
    got, stats = L.anchor_distances(ctx, **case, metric=metric, return_stats=True)
    np.testing.assert_array_equal(got, want[metric])
    assert stats["launches"] == 1 and stats["ref_points"] == len(case["ref_coords"])
    if name in ("set_of_below", "one_point", "257_against_one", "zero_extent"):
        assert stats["gridded_sets"] == 0, stats
    if name in ("set_of_at", "set_of_above", "corner"):
        assert stats["gridded_sets"] == 1, stats
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return
    np.testing.assert_array_equal(got, cases.sklearn_search(**case, metric=metric))


@pytest.mark.parametrize("name", ["uniform_4x3", "hex_lattice_shifted", "corner", "uniform_3d"])
def test_every_grid_gives_the_same_bytes(L, ctx, search_cases, name):
    """One cell per set (the brute-force sweep) and finer and coarser grids than the default, through the hook."""
    case, want = _case(L, search_cases, name)
    for brute_below, per_cell in ((10**9, 0.0), (2, 1.0), (2, 8.0)):
        got, stats = L.anchor_distances(ctx, **case, metric="euclidean", brute_below=brute_below, per_cell=per_cell, return_stats=True)
        np.testing.assert_array_equal(got, want["euclidean"])
        assert (stats["gridded_sets"] == 0) == (brute_below > 2), stats


def test_public_anchor_distances(L, search_cases):
    import squidpy_amd as sq

    rng = np.random.default_rng(3)
    xy = rng.random((700, 2)) * 5000.0
    labels, slides = rng.integers(0, 3, 700), np.array(["s0", "s1"])[rng.integers(0, 2, 700)]
    labels[(labels == 1) & (slides == "s1")] = 2  # label 1 does not occur in s1
    xy[11, 0], xy[40] = np.nan, np.inf
    got = sq.tl.anchor_distances(xy, labels, [0, 1, 2], slides, metric="manhattan")
    assert got.shape == (700, 3)
    ok = np.isfinite(xy).all(axis=1)
    case = cases._labelled(xy[ok], labels[ok], (slides[ok] == "s1").astype(np.int64), 3, 2)
    np.testing.assert_array_equal(got[ok], cases.brute(**case, metric="manhattan").T)
    assert np.isnan(got[~ok]).all() and np.isnan(got[ok & (slides == "s1"), 1]).all() and not np.isnan(got[ok & (slides == "s0")]).any()


@pytest.mark.parametrize("name", [c["name"] for c in cases.frame_cases()])
def test_var_by_distance_reproduces_the_reference_frames(golden, name):
    import squidpy_amd as sq

    coords, obs, kwargs, want = golden["cases"][name]
    got = sq.tl.var_by_distance(_adata(coords, obs), copy=True, **kwargs)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    adata = _adata(coords, obs)
    assert sq.tl.var_by_distance(adata, **kwargs) is None
    pd.testing.assert_frame_equal(adata.obsm[kwargs.get("design_matrix_key", "design_matrix")], want, check_exact=True)
    pd.testing.assert_frame_equal(adata.obs, obs, check_exact=True)


def test_two_calls_return_the_same_bytes(L, ctx, search_cases):
    for name in ("uniform_4x3", "hex_lattice", "uniform_3d"):
        case, _ = _case(L, search_cases, name)
        a, b = L.anchor_distances(ctx, **case), L.anchor_distances(ctx, **case)
        assert a.tobytes() == b.tobytes()


def test_forty_anchors_and_five_slides_are_one_launch(L, ctx):
    rng = np.random.default_rng(5)
    xy = rng.random((4000, 2)) * 1e4
    case = cases._labelled(xy, rng.integers(0, 40, 4000), rng.integers(0, 5, 4000), 40, 5)
    assert (case["set_of"] >= 0).sum() == 200
    ctx.timer_enable(True)
    ctx.timer_reset()
    try:
        got = L.anchor_distances(ctx, **case)
        ctx.sync()
        launches = {k: ctx.timer_get(k)[1] for k in ("anchor_query", "anchor_count", "anchor_scan", "anchor_scatter")}
    finally:
        ctx.timer_enable(False)
    assert launches == {"anchor_query": 1, "anchor_count": 1, "anchor_scan": 1, "anchor_scatter": 1}, launches
    np.testing.assert_array_equal(got, cases.brute(**case, metric="euclidean"))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates_are_refused(L, ctx, bad):
    q, r = np.random.default_rng(1).random((50, 2)), np.random.default_rng(2).random((20, 2))
    args = (np.zeros(50, np.int32), r, np.zeros(20, np.int32), np.zeros((1, 1), np.int32))
    qq = q.copy()
    qq[7, 1] = bad
    with pytest.raises(L.SqgrError, match="not finite"):
        L.anchor_distances(ctx, qq, *args)
    rr = r.copy()
    rr[3, 0] = bad
    with pytest.raises(L.SqgrError, match="not finite"):
        L.anchor_distances(ctx, q, args[0], rr, args[2], args[3])
    with pytest.raises(L.SqgrError, match="slide"):
        L.anchor_distances(ctx, q, np.full(50, 1, np.int32), *args[1:])
    with pytest.raises(L.SqgrError, match="set"):
        L.anchor_distances(ctx, q, args[0], r, np.full(20, 5, np.int32), args[3])
