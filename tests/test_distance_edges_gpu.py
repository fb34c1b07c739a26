"""GPU tests of the distance kernels at real coordinate scales and on rounding boundaries.

Every result is compared with ``assert_array_equal`` — indices, distances and counts — against sklearn (what the reference
calls) or the oracle:
  * a translation / scale matrix: one clustered + lattice + random pattern at spacings 1, 10, 100, placed at offsets 0, 1e4,
    1e5, 1e7 (x positive, y negative), through knn_self, radius_self, knn_dist / knn_hist (three metrics, both sides of
    KNN_GRID_MIN_REFS), pair_counts and cooccur_counts (dense, fast and near routes, fused and unfused);
  * planted boundary pairs (tests/test_distance_edges_cpu.py proves where each one lies): pairs exactly on a threshold and
    their nearest neighbours either side, points on build_grid cell edges and one ulp either side, k-th neighbours just
    outside the finished ring and ties across it, clouds with |x0| / h >= 1e7, and degenerate extents;
  * the front ends on a cloud offset by 1e5.
The route every call takes is read back from the context's kernel timers."""

from __future__ import annotations

import math

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import restate as O
from tests.test_distance_edges_cpu import boundary_pair, decimal_point, fma_split_pairs, occur_count_fma

pytestmark = pytest.mark.gpu

SPACINGS = (1.0, 10.0, 100.0)
OFFSETS = (0.0, 1e4, 1e5, 1e7)
METRICS = ("euclidean", "manhattan", "chebyshev")


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def pattern(spacing: float, offset: float, seed: int = 0) -> np.ndarray:
    """2 000 points: three Gaussian clusters, a 30 x 25 lattice (exact ties) and uniform noise, ~60 spacings wide, at
    (offset, -offset) in decimal microns (4 decimals: not representable in binary)."""
    rng = np.random.default_rng(seed)
    parts = [rng.normal(c, 2.0, (300, 2)) for c in ((10, 12), (45, 30), (20, 45))]
    g = np.stack(np.meshgrid(np.arange(30.0), np.arange(25.0)), -1).reshape(-1, 2) * 2.0
    parts += [g, rng.random((350, 2)) * 60.0]
    xy = np.concatenate(parts) * spacing
    return np.round(xy + np.array([offset, -offset]), 4)


def kernels(ctx, fn):
    """run fn() with the kernel timers on -> (result, names of the kernels that ran)"""
    ctx.timer_enable(True)
    ctx.timer_reset()
    try:
        out = fn()
        rep = ctx.timer_report()
    finally:
        ctx.timer_enable(False)
    return out, {name for name, (cnt, _) in rep.items() if cnt > 0}


def d2_rows(q: np.ndarray, r: np.ndarray) -> np.ndarray:
    """float64 fl(fl(dx*dx) + fl(dy*dy)) of every (query, reference) pair, as the kernels and sklearn compute it"""
    dx = q[:, None, 0] - r[None, :, 0]
    dy = q[:, None, 1] - r[None, :, 1]
    return dx * dx + dy * dy


def check_knn_self(L, ctx, xy: np.ndarray, ks=(1, 6, 15, 40, 64)):
    """knn_self == sklearn's KD-tree distances, and the indices follow the documented order: ascending (d2, index)"""
    from sklearn.neighbors import NearestNeighbors

    d2 = d2_rows(xy, xy)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, : max(ks)]
    nn = NearestNeighbors(n_neighbors=max(ks), algorithm="kd_tree").fit(xy)
    for k in ks:
        (dist, idx), names = kernels(ctx, lambda: L.knn_self(ctx, xy, k))
        assert "neighbors_knn_grid" in names, names
        rd, _ = nn.kneighbors(n_neighbors=k)
        np.testing.assert_array_equal(dist, rd, err_msg=f"k={k}")
        np.testing.assert_array_equal(idx, order[:, :k], err_msg=f"k={k}")


def check_radius_self(L, ctx, xy: np.ndarray, r: float):
    from sklearn.neighbors import NearestNeighbors

    (indptr, idx, dist), names = kernels(ctx, lambda: L.radius_self(ctx, xy, r))
    assert "neighbors_radius_count" in names, names
    rd, ri = NearestNeighbors(radius=r, algorithm="kd_tree").fit(xy).radius_neighbors()
    n = len(xy)
    np.testing.assert_array_equal(np.diff(indptr), [len(a) for a in ri])
    rows = np.repeat(np.arange(n), np.diff(indptr))
    got = sp.csr_matrix((dist + 1.0, (rows, idx)), shape=(n, n))
    ref = sp.csr_matrix((np.concatenate(rd) + 1.0, (rows, np.concatenate(ri).astype(np.int64))), shape=(n, n))
    assert (got != ref).nnz == 0
    return indptr, idx


def check_knn_dist_hist(L, ctx, qry: np.ndarray, refs: np.ndarray, k: int, metric: str, edges: np.ndarray):
    """knn_dist == sklearn's distances; DevicePoints.knn_hist == np.histogram of them; the cell list runs from
    KNN_GRID_MIN_REFS references on, the brute-force sweep below"""
    from sklearn.neighbors import NearestNeighbors

    grid = len(refs) >= 512
    exp, _ = NearestNeighbors(n_neighbors=k, metric=metric, algorithm="kd_tree").fit(refs).kneighbors(qry)
    got, names = kernels(ctx, lambda: L.knn_dist(ctx, qry, refs, k, metric))
    assert ("ripley_knn_cells" if grid else "ripley_knn") in names, names
    np.testing.assert_array_equal(got, exp, err_msg=metric)
    pts = L.DevicePoints(ctx, qry)
    try:
        h, names = kernels(ctx, lambda: pts.knn_hist(refs, k, edges, metric))
    finally:
        pts.close()
    assert ("ripley_knn_hist_cells" if grid else "ripley_knn_hist") in names, names
    np.testing.assert_array_equal(h, np.histogram(exp.ravel(), bins=edges)[0], err_msg=metric)


def check_pair_counts(L, ctx, xy: np.ndarray, support: np.ndarray, metric: str):
    from sklearn.neighbors import KDTree

    got, names = kernels(ctx, lambda: L.pair_counts(ctx, xy, support, metric))
    ref = KDTree(xy, metric=metric).two_point_correlation(xy, support, dualtree=True) - len(xy)
    np.testing.assert_array_equal(got, ref, err_msg=metric)
    return names


def crowd(t: np.ndarray) -> np.ndarray:
    """t and its next three float32 neighbours above: too close for the lookup table's fast kernel (k_cooccur runs)"""
    out = [t]
    for _ in range(3):
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    return np.concatenate(out).astype(np.float32)


def route_calls(thr_fast: np.ndarray, thr_crowded: np.ndarray) -> list:
    """(thresholds, SQGR_COOCCUR_SPARSE, kernel): the dense exact-compare kernel (crowded thresholds), the dense fast kernel
    and the near route (candidate tile lists)"""
    return [(thr_crowded, "0", "cooccur_pairs"), (thr_fast, "0", "cooccur_pairs_fast"), (thr_fast, "1", "cooccur_pairs_near")]


def check_cooccur_routes(L, ctx, monkeypatch, x, y, labs, k, calls) -> tuple[set, np.ndarray, np.ndarray]:
    """every call fused and unfused: fma=False == oracle.occur_count, fma=True == the exact fmaf emulation (both computed
    once over all thresholds: a threshold's count depends on its own value only); the named kernel must have run"""
    thr_all = np.concatenate([t for t, _, _ in calls]).astype(np.float32)
    ref_all = O.occur_count(x, y, thr_all, labs, k)
    fma_all = occur_count_fma(x, y, thr_all, labs, k)
    seen, c0 = set(), 0
    for thr, sparse, want in calls:
        sl = slice(c0, c0 + len(thr))
        c0 += len(thr)
        monkeypatch.setenv("SQGR_COOCCUR_SPARSE", sparse)
        for fma, exp in ((False, ref_all[..., sl]), (True, fma_all[..., sl])):
            got, names = kernels(ctx, lambda: L.cooccur_counts(ctx, x, y, labs, k, thr, fma=fma))
            name = want + ("_fma" if fma else "")
            assert name in names, (name, names)
            seen.add(name)
            np.testing.assert_array_equal(got, exp, err_msg=name)
    monkeypatch.delenv("SQGR_COOCCUR_SPARSE")
    return seen, ref_all, fma_all


# ------------------------------------------------------------------------------------------- translation x scale matrix

@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_graph_builders_at_every_offset_and_scale(L, ctx, spacing, offset):
    xy = pattern(spacing, offset)
    check_knn_self(L, ctx, xy)
    for r in (spacing * 2.0, spacing * 3.7):   # (the lattice step is 2 spacings: many pairs near the first radius)
        check_radius_self(L, ctx, xy, r)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_ripley_kernels_at_every_offset_and_scale(L, ctx, spacing, offset):
    xy = pattern(spacing, offset, seed=1)
    qry = np.concatenate([xy[1500:], np.round(xy[:200] + spacing * np.array([0.37, -0.61]), 4)])
    edges = np.arange(0.0, 9.0) * spacing
    for metric in METRICS:
        for refs in (xy[:400], xy[:1500]):       # brute force below KNN_GRID_MIN_REFS = 512, the cell list above
            check_knn_dist_hist(L, ctx, qry, refs, 3, metric, edges)
    support = np.linspace(0.0, 6.0, 25) * spacing
    names = set()
    for metric in METRICS:
        names |= check_pair_counts(L, ctx, xy, support, metric)
        names |= check_pair_counts(L, ctx, xy, np.sort(np.concatenate([support[:3], np.nextafter(support[2], np.inf) + [0.0, 0.0]])), metric)
    assert {"ripley_pair_hist_fast"} <= names, names


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_cooccur_at_every_offset_and_scale(L, ctx, monkeypatch, spacing, offset):
    xy = pattern(spacing, offset, seed=2)[::2]
    x, y = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    labs = np.random.default_rng(3).integers(0, 4, len(x)).astype(np.int32)
    thr = (np.linspace(0.5, 6.0, 9, dtype=np.float32) * np.float32(spacing)) ** 2
    seen, _, _ = check_cooccur_routes(L, ctx, monkeypatch, x, y, labs, 4, route_calls(thr, crowd(thr[3:5])))
    assert len(seen) == 6, seen


# --------------------------------------------------------------------------------------------------- planted boundaries

def planted_cloud(offset: float, seed: int, n: int = 1500, width: float = 300.0):
    rng = np.random.default_rng(seed)
    return np.round(rng.random((n, 2)) * width + np.array([offset, -offset - width]), 4)


@pytest.mark.parametrize("offset", OFFSETS)
def test_planted_boundary_pairs_graph_and_ripley(L, ctx, offset):
    """Pairs whose float64 d2 IS fl(r*r) (radius_self) or sqrt_thresholds(r) (pair_counts), with their nearest twins inside
    and outside, planted in a 1 500-point cloud: the neighbour on the boundary and the inside twin are found, the outside
    twin is not, and the whole graph / count equals sklearn's."""
    rng = np.random.default_rng(11)
    base = planted_cloud(offset, 12)
    for j, radius in enumerate((0.7, 3.3, 12.3, 47.9)):
        c = decimal_point(rng, offset, 250.0)
        c = (c[0] + 20.0, c[1] - 20.0)
        bp = boundary_pair("radius64", c, radius, theta=0.5 + j)
        xy = np.concatenate([base, [bp["c"], bp["p"], bp["inside"], bp["outside"]]])
        n0 = len(base)
        indptr, idx = check_radius_self(L, ctx, xy, bp["r"])
        row = set(idx[indptr[n0] : indptr[n0 + 1]].tolist())
        assert {n0 + 1, n0 + 2} <= row and n0 + 3 not in row, row
        rp = boundary_pair("ripley64", c, radius, theta=1.1 + j)
        xy = np.concatenate([base, [rp["c"], rp["p"], rp["inside"], rp["outside"]]])
        support = np.array([0.0, rp["r"], 2.0 * rp["r"]])
        with_p = L.pair_counts(ctx, xy, support)
        check_pair_counts(L, ctx, xy, support, "euclidean")
        # moving p and its inside twin onto the outside twin drops exactly the 4 ordered pairs they form with c
        moved = xy.copy()
        moved[n0 + 1] = rp["outside"]
        moved[n0 + 2] = rp["outside"]
        assert with_p[1] - L.pair_counts(ctx, moved, support)[1] == 4
        check_pair_counts(L, ctx, moved, support, "euclidean")


@pytest.mark.parametrize("offset", OFFSETS)
def test_planted_boundary_pairs_cooccur_fused_and_unfused(L, ctx, monkeypatch, offset):
    """float32 pairs exactly on a threshold (and their twins), and pairs whose fused and unfused d2 straddle one, planted in
    a 1 500-point cloud: fma=False == oracle.occur_count, fma=True == the exact fmaf emulation — on every route.  The
    fused and unfused expectations differ where split pairs exist, so the comparison is exact, not a tolerance."""
    rng = np.random.default_rng(21)
    base = planted_cloud(offset, 22).astype(np.float32)
    pts, thr = [], []
    for j, radius in enumerate((3.3, 12.3, 47.9)):
        c = decimal_point(rng, offset, 250.0)
        c = (c[0] + 20.0, c[1] - 20.0)
        bp = boundary_pair("cooc32", c, radius, theta=0.3 + j)
        pts += [bp["c"], bp["p"], bp["inside"], bp["outside"]]
        thr.append(bp["thr"])
    splits = []
    if offset < 1e7:   # (at 1e7 the float32 grid is the integers: no d2 below 2**24 rounds, fused or not)
        for radius in (37.3, 91.1):   # (a rounded dx*dx: |dx| > 32 at 1e5, where the float32 grid is 2**-7)
            c = decimal_point(rng, offset, 250.0)
            found = fma_split_pairs((c[0] + 20.0, c[1] - 20.0), radius, n_want=2)
            assert found
            for s in found:
                pts += [s["c"], s["p"]]
                thr.append(s["thr"])
                splits.append(s)
    xy = np.concatenate([base, np.array(pts, np.float32)])
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    labs = np.random.default_rng(23).integers(0, 3, len(x)).astype(np.int32)
    thr = np.array(thr, np.float32)
    calls = []
    for t in thr:   # one threshold per fast call: the lookup table is always fine enough for the fast kernels
        calls += route_calls(np.array([t], np.float32), crowd(np.array([t], np.float32)))
    seen, ref, ref_fma = check_cooccur_routes(L, ctx, monkeypatch, x, y, labs, 3, calls)
    assert len(seen) == 6, seen
    if splits:   # the planted split pairs make the fused and the unfused expectations differ
        assert (ref != ref_fma).any()


def grid_h(xy: np.ndarray, target: float = 2.0, min_h: float = 0.0):
    """build_grid's cell side and origin (sqgr_neighbors.hip), with the same float64 operations"""
    x0, y0 = xy[:, 0].min(), xy[:, 1].min()
    w = max(xy[:, 0].max() - x0, 1e-300)
    hgt = max(xy[:, 1].max() - y0, 1e-300)
    h = math.sqrt(w * hgt * target / float(len(xy)))
    h = max(h, max(w, hgt) / 4096.0, min_h)
    return float(x0), float(y0), h


def ring_cloud(offset: float, spread: float, seed: int) -> np.ndarray:
    """Points in the lower half of a box, the upper half empty, cells on build_grid's grid: in the empty half, queries
    at cell centres with their k-th neighbour just outside the ring-0 block (one ulp past the cell edge), or tied with one
    across it, or one ulp inside; and points exactly on cell edges and one ulp either side."""
    rng = np.random.default_rng(seed)
    n_bg, n_q = 1600, 24
    n_edge = 60
    n = n_bg + 2 + n_q * 5 + n_edge
    bg = rng.random((n_bg, 2)) * np.array([spread, spread * 0.5])
    corners = np.array([[0.0, 0.0], [spread, spread]])
    xy = np.round(np.concatenate([bg, corners]) + np.array([offset, -offset - spread]), 4)
    # the grid of the final cloud: its box is the corners', its size n
    x0, y0 = xy[:, 0].min(), xy[:, 1].min()
    w, hgt = xy[:, 0].max() - x0, xy[:, 1].max() - y0
    h = max(math.sqrt(w * hgt * 2.0 / n), max(w, hgt) / 4096.0)
    gx, gy = int(math.floor(w / h)) + 1, int(math.floor(hgt / h)) + 1
    extra, ties = [], 0
    cells = rng.permutation([(cx, cy) for cx in range(2, gx - 2, 3) for cy in range(gy // 2 + 3, gy - 2, 3)])[:n_q]
    assert len(cells) == n_q
    for j, (cx, cy) in enumerate(cells):
        xl = x0 + float(cx) * h
        qx, qy = x0 + (float(cx) + 0.5) * h, y0 + (float(cy) + 0.5) * h
        qx, qy = round(qx, 4), round(qy, 4)
        out_x = np.nextafter(xl, -np.inf)          # one ulp left of the cell edge: in cell cx - 1, outside ring 0
        da = qx - out_x
        variant = j % 3
        db = da if variant == 0 else (np.nextafter(da, 0.0) if variant == 1 else np.nextafter(da, np.inf))
        iy = qy + db
        near = [(qx + 0.05 * h, qy - 0.07 * h), (qx - 0.11 * h, qy + 0.02 * h)]
        pts = [(qx, qy), (out_x, qy), (qx, iy)] + near
        ties += (out_x - qx) ** 2 == (iy - qy) ** 2
        if j % 2:                                  # ties go to the smaller index: both orders
            pts[1], pts[2] = pts[2], pts[1]
        extra += pts
    for j in range(n_edge // 6):                   # cell edges x0 + c*h (the device's own expression) and one ulp either side
        cx, cy = int(rng.integers(1, gx - 1)), int(rng.integers(1, gy - 1))
        ex, ey = x0 + float(cx) * h, y0 + float(cy) * h
        ry, rx = y0 + (0.01 + 0.98 * rng.random()) * hgt, x0 + (0.01 + 0.98 * rng.random()) * w
        extra += [(ex, ry), (np.nextafter(ex, -np.inf), ry + 1e-3 * h), (np.nextafter(ex, np.inf), ry - 1e-3 * h),
                  (rx, ey), (rx + 1e-3 * h, np.nextafter(ey, -np.inf)), (rx - 1e-3 * h, np.nextafter(ey, np.inf))]
    xy = np.concatenate([xy, np.array(extra)])
    assert len(xy) == n and ties >= 2
    assert grid_h(xy)[2] == h
    return xy


@pytest.mark.parametrize("offset,spread", [(0.0, 400.0), (1e4, 400.0), (1e5, 40.0), (1e7, 25.0), (-3e7, 60.0)])
def test_planted_ring_edges_and_ties(L, ctx, offset, spread):
    """k-th neighbours one ulp outside the ring the search has finished, ties across it (both index orders) and one-ulp
    wins inside it, points on cell edges; |x0| / h reaches 1e7 and more at the last offsets (spread 40 -> h ~ 0.7)."""
    xy = ring_cloud(offset, spread, seed=int(abs(offset)) % 1000 + 5)
    x0, _, h = grid_h(xy)
    if abs(offset) >= 1e7:
        assert abs(x0) / h >= 1e7
    check_knn_self(L, ctx, xy, ks=(1, 3, 6, 40))
    qry = np.round(xy[::7] + np.array([0.013, -0.029]) * h, 4)
    for metric in METRICS:
        check_knn_dist_hist(L, ctx, np.concatenate([xy[-180:], qry]), xy, 3, metric, np.linspace(0.0, 2.0 * h, 17))
    check_radius_self(L, ctx, xy, 0.5 * h)


@pytest.mark.parametrize("offset", [0.0, 1e5, 1e7])
def test_degenerate_extents(L, ctx, monkeypatch, offset):
    """All points on one line (zero height: a 1-row grid), and two far clusters whose box forces the 4096-cell cap (many
    points per cell)."""
    rng = np.random.default_rng(31)
    line = np.round(np.stack([offset + rng.random(1200) * 500.0, np.full(1200, -offset - 7.25)], 1), 4)
    line[::10, 0] = line[1::10, 0]                                     # duplicates
    blob = lambda: np.stack([rng.normal(0.0, 5.0, 700), rng.random(700) * 4.0], 1)   # (flat: the box is 2e5 x 4)
    far = np.concatenate([blob(), blob() + np.array([2e5, 0.0])])
    far = np.round(far + np.array([offset, -offset]), 4)
    assert max(np.ptp(far, 0)) / grid_h(far)[2] == pytest.approx(4096.0)
    for xy in (line, far):
        check_knn_self(L, ctx, xy, ks=(1, 6, 40))
        check_radius_self(L, ctx, xy, 2.5)
        for metric in METRICS:
            check_knn_dist_hist(L, ctx, xy[::5] + 0.3, xy, 2, metric, np.linspace(0.0, 5.0, 11))
        check_pair_counts(L, ctx, xy, np.linspace(0.0, 6.0, 13), "euclidean")
        x, y = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
        labs = rng.integers(0, 3, len(x)).astype(np.int32)
        thr = np.linspace(0.5, 6.0, 6, dtype=np.float32) ** 2
        assert len(check_cooccur_routes(L, ctx, monkeypatch, x, y, labs, 3, route_calls(thr, crowd(thr[2:3])))[0]) == 6


# ------------------------------------------------------------------------------------------------------------ front ends

def _offset_adata(offset: float = 1e5):
    import squidpy_amd as sq

    rng = np.random.default_rng(41)
    xy = np.round(rng.random((900, 2)) * 400.0 + np.array([offset, -offset]), 4)
    lab = rng.integers(0, 3, len(xy))
    xy[lab == 0] = np.round((xy[lab == 0] - np.array([offset, -offset])) * 0.5 + np.array([offset + 100.0, -offset + 100.0]), 4)
    obs = pd.DataFrame({"cl": pd.Categorical.from_codes(lab, ["a", "b", "c"])})
    return sq.AnnDataLite(X=np.ones((len(xy), 3)), obs=obs, obsm={"spatial": xy}), xy, lab


def test_front_ends_at_offset_coordinates(L):
    import squidpy_amd as sq

    adata, xy, lab = _offset_adata()

    def same(a, b):
        a, b = sp.csr_matrix(a), sp.csr_matrix(b)
        return a.shape == b.shape and (a != b).nnz == 0

    res = sq.gr.spatial_neighbors_knn(adata, n_neighs=8, percentile=90.0, copy=True)
    ref_adj, ref_dst = O.spatial_graph(xy, "knn", n_neighs=8, percentile=90.0)
    assert same(res.connectivities, ref_adj) and same(res.distances, ref_dst)
    res = sq.gr.spatial_neighbors_radius(adata, radius=(10.0, 35.0), copy=True)
    ref_adj, ref_dst = O.spatial_graph(xy, "radius", radius=(10.0, 35.0))
    assert same(res.connectivities, ref_adj) and same(res.distances, ref_dst)
    occ, interval = sq.gr.co_occurrence(adata, "cl", interval=12, copy=True)
    occ_ref, interval_ref = O.co_occurrence(xy, lab, interval=12)
    np.testing.assert_array_equal(interval, interval_ref)
    np.testing.assert_allclose(occ, occ_ref, rtol=1e-12, atol=0)   # float64 ratios of exact counts
    for mode in ("L", "G"):
        res = sq.gr.ripley(adata, "cl", mode=mode, n_simulations=8, n_observations=150, n_steps=20, seed=3, copy=True)
        ref = O.ripley(xy, adata.obs["cl"].values, mode=mode, n_simulations=8, n_observations=150, n_steps=20, seed=3)
        np.testing.assert_array_equal(res["bins"], ref["bins"])
        np.testing.assert_allclose(res[f"{mode}_stat"]["stats"].to_numpy().reshape(3, 20), ref["obs"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["sims_stat"]["stats"].to_numpy().reshape(8, 20), ref["sims"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(res["pvalues"], ref["pvalues"])
