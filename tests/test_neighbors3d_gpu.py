"""GPU parity tests of spatial graph construction on 3-D coordinates: the device cell-list kNN / radius search of
``csrc/sqgr_neighbors3d.hip`` vs sklearn's KD-tree (what the reference's builders call, gr/neighbors.py:157-419, for
coordinates of any width) and whole graphs vs the oracle's restatement of gr/neighbors.py.  Every comparison is an
equality; only ``transform="cosine"`` keeps the tolerance of the 2-D test."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import restate as O
from tests.neighbors3d_cases import lattice, lex_order as _lex_order, sk_knn as _sk_knn, sk_radius_csr, stacked_sections

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _same(a, b):
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    return a.shape == b.shape and (a != b).nnz == 0


def _adata(xyz, **obs):
    import squidpy_amd as sq

    return sq.AnnDataLite(X=np.ones((len(xyz), 3)), obs=pd.DataFrame(obs) if obs else None, obsm={"spatial": np.asarray(xyz)})


# ------------------------------------------------------------------------------------------------ 1. generic clouds


@pytest.mark.parametrize("n,k", [(50, 3), (1000, 6), (3000, 15), (2500, 40)])
def test_knn_equals_sklearn_on_generic_clouds(L, ctx, n, k):
    rng = np.random.default_rng(n + k)
    xyz = rng.random((n, 3)) * np.array([1000.0, 30.0, 200.0])  # anisotropic cloud
    dist, idx = L.knn_self(ctx, xyz, k)
    rd, ri = _sk_knn(xyz, k)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist, rd)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and dist.shape == idx.shape == (n, k)
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 4, n_samples_fit = 3, n_samples = 3"):
        L.knn_self(ctx, xyz[:3], 3)


# ------------------------------------------------------------------------------------------- 2. ties and duplicates


def test_knn_ties_and_duplicates(L, ctx):
    """Unit lattice + coincident points: distances equal sklearn's; ties go to the smaller index (documented policy)."""
    g = lattice()
    xyz = np.concatenate([g, g[:7]])  # duplicates
    dist, idx = L.knn_self(ctx, xyz, 5)
    rd, _ = _sk_knn(xyz, 5)
    np.testing.assert_array_equal(dist, rd)
    bd, order = _lex_order(xyz, 5)
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_array_equal(dist, bd)
    assert (dist[:7, 0] == 0.0).all() and (idx[:7, 0] == len(g) + np.arange(7)).all()  # the coincident twin comes first


# ---------------------------------------------------------------------------------------------- 3. degenerate extents


def test_constant_z_equals_the_2d_search(L, ctx):
    rng = np.random.default_rng(21)
    xy = rng.random((2000, 2)) * np.array([800.0, 90.0])
    xyz = np.column_stack([xy, np.full(len(xy), 12.5)])
    dist, idx = L.knn_self(ctx, xyz, 6)
    d2, i2 = L.knn_self(ctx, xy, 6)
    np.testing.assert_array_equal(dist, d2)
    np.testing.assert_array_equal(idx, i2)
    rd, ri = _sk_knn(xyz, 6)
    np.testing.assert_array_equal(dist, rd)
    np.testing.assert_array_equal(idx, ri)
    ip3, c3, l3 = L.radius_self(ctx, xyz, 20.0)
    ip2, c2, l2 = L.radius_self(ctx, xy, 20.0)
    n = len(xy)
    assert _same(sp.csr_matrix((l3 + 1.0, c3, ip3), shape=(n, n)), sp.csr_matrix((l2 + 1.0, c2, ip2), shape=(n, n)))


def test_collinear_points(L, ctx):
    rng = np.random.default_rng(22)
    xyz = np.column_stack([rng.random(1500) * 1e4, np.full(1500, -3.0), np.full(1500, 7.0)])
    dist, idx = L.knn_self(ctx, xyz, 6)
    rd, ri = _sk_knn(xyz, 6)
    np.testing.assert_array_equal(dist, rd)
    np.testing.assert_array_equal(idx, ri)


def test_all_points_coincident(L, ctx):
    xyz = np.tile(np.array([[3.0, -1.0, 2.5]]), (40, 1))
    dist, idx = L.knn_self(ctx, xyz, 3)
    rd, _ = _sk_knn(xyz, 3)
    np.testing.assert_array_equal(dist, rd)
    assert (dist == 0.0).all()
    want = np.array([[j for j in range(4) if j != i][:3] for i in range(40)])  # the three smallest other indices
    np.testing.assert_array_equal(idx, want)
    indptr, cols, length = L.radius_self(ctx, xyz, 0.0)
    assert (np.diff(indptr) == 39).all() and (length == 0.0).all()


# ---------------------------------------------------------------------------------------------- 4. stacked sections


def _radius_csr(n, indptr, idx, dist):
    return sp.csr_matrix((dist + 1.0, idx, indptr), shape=(n, n))  # + 1: a zero distance stays a stored entry


@pytest.mark.parametrize("r", [0.0, 7.5, 50.0, 60.0, 1e4])
def test_radius_equals_sklearn_on_stacked_sections(L, ctx, r):
    xyz, first, twin = stacked_sections(50.0)
    n = len(xyz)
    indptr, idx, dist = L.radius_self(ctx, xyz, r)
    assert indptr.dtype == np.int64 and idx.dtype == np.int32 and dist.dtype == np.float64
    ref = sk_radius_csr(xyz, r)
    got = _radius_csr(n, indptr, idx, dist)
    assert _same(got, ref)
    if r == 50.0:  # the planted pairs are exactly 50 apart: the boundary is inclusive
        assert (np.asarray(got[first, twin]).ravel() == 51.0).all() and (np.asarray(got[twin, first]).ravel() == 51.0).all()


@pytest.mark.parametrize("z_step", [50.0, 0.01])
def test_knn_on_stacked_sections(L, ctx, z_step):
    """Few distinct z values, wider apart than the in-plane spacing (~19) and far closer."""
    xyz, _, _ = stacked_sections(z_step)
    dist, idx = L.knn_self(ctx, xyz, 6)
    rd, ri = _sk_knn(xyz, 6)
    np.testing.assert_array_equal(dist, rd)
    bd, order = _lex_order(xyz, 7)
    np.testing.assert_array_equal(idx, order[:, :6])
    untied = (np.diff(bd, axis=1) > 0).all(axis=1)  # where no two candidates are equally far sklearn's order is the only one
    assert untied.sum() > len(xyz) // 2
    np.testing.assert_array_equal(idx[untied], ri[untied])


# --------------------------------------------------------------------------------------------------- 5. front ends


def _cloud700():
    return np.random.default_rng(11).random((700, 3)) * np.array([400.0, 400.0, 60.0])


@pytest.mark.parametrize("kw", [
    dict(kind="knn", n_neighs=6), dict(kind="knn", n_neighs=4, set_diag=True), dict(kind="knn", n_neighs=8, percentile=90.0),
    dict(kind="knn", n_neighs=6, transform="spectral"), dict(kind="knn", n_neighs=5, transform="cosine"),
    dict(kind="radius", radius=35.0), dict(kind="radius", radius=(10.0, 35.0), set_diag=True),
    dict(kind="radius", radius=(10.0, 35.0), percentile=80.0), dict(kind="radius", radius=30.0, transform="spectral"),
])
def test_generic_builders_equal_reference_restatement(L, kw):
    import squidpy_amd as sq

    xyz = _cloud700()
    kw = dict(kw)
    kind = kw.pop("kind")
    fn = sq.gr.spatial_neighbors_knn if kind == "knn" else sq.gr.spatial_neighbors_radius
    res = fn(_adata(xyz), copy=True, **kw)
    ref_adj, ref_dst = O.spatial_graph(xyz, kind, **kw)
    assert res.connectivities.dtype == ref_adj.dtype and res.distances.dtype == ref_dst.dtype
    if kw.get("transform") == "cosine":
        np.testing.assert_allclose(res.connectivities.toarray(), ref_adj.toarray(), rtol=1e-6, atol=1e-7)
    else:
        assert _same(res.connectivities, ref_adj)
    assert _same(res.distances, ref_dst)


@pytest.mark.parametrize("n_rings,set_diag", [(1, False), (2, True)])
def test_grid_builder_on_a_cubic_lattice(L, n_rings, set_diag):
    import squidpy_amd as sq

    xyz = lattice() * 100.0
    res = sq.gr.spatial_neighbors_grid(_adata(xyz), n_neighs=6, n_rings=n_rings, set_diag=set_diag, copy=True)
    ref_adj, ref_dst = O.spatial_graph(xyz, "grid", n_neighs=6, n_rings=n_rings, set_diag=set_diag)
    assert res.connectivities.dtype == ref_adj.dtype and res.distances.dtype == ref_dst.dtype
    assert _same(res.connectivities, ref_adj) and _same(res.distances, ref_dst)
    if n_rings == 1:  # the 6-neighbour lattice: 2 (8*8*7 + 9*7*7 + 9*8*6) directed edges, whichever way the kNN ties fall
        assert res.connectivities.nnz == 2642
        deg = np.diff(res.connectivities.indptr)
        assert deg.min() == 3 and deg.max() == 6


def test_builder_classes_through_from_builder(L):
    import squidpy_amd as sq
    from squidpy_amd.gr import neighbors as nb

    xyz = _cloud700()
    for builder, kind, kw in ((nb.KNNBuilder(n_neighs=7, set_diag=True), "knn", dict(n_neighs=7, set_diag=True)),
                              (nb.RadiusBuilder(radius=(10.0, 35.0), percentile=80.0), "radius", dict(radius=(10.0, 35.0), percentile=80.0))):
        res = sq.gr.spatial_neighbors_from_builder(_adata(xyz), builder, copy=True)
        ref_adj, ref_dst = O.spatial_graph(xyz, kind, **kw)
        assert res.connectivities.dtype == ref_adj.dtype and res.distances.dtype == ref_dst.dtype
        assert _same(res.connectivities, ref_adj) and _same(res.distances, ref_dst)
    grid = lattice() * 100.0
    ad = _adata(grid)
    assert sq.gr.spatial_neighbors_from_builder(ad, nb.GridBuilder(n_neighs=6, n_rings=2)) is None
    ref_adj, ref_dst = O.spatial_graph(grid, "grid", n_neighs=6, n_rings=2)
    assert _same(ad.obsp["spatial_connectivities"], ref_adj) and _same(ad.obsp["spatial_distances"], ref_dst)
    assert ad.uns["spatial_neighbors"]["params"]["coord_type"] == "grid"


def test_legacy_dispatcher_takes_3d(L):
    import squidpy_amd as sq

    xyz = _cloud700()
    ad = _adata(xyz)
    with pytest.warns(FutureWarning, match="deprecated"):
        sq.gr.spatial_neighbors(ad, n_neighs=5, coord_type="generic")
    ref_adj, ref_dst = O.spatial_graph(xyz, "knn", n_neighs=5)
    assert _same(ad.obsp["spatial_connectivities"], ref_adj) and _same(ad.obsp["spatial_distances"], ref_dst)


def test_library_key_gives_block_diagonal_graph(L):
    import squidpy_amd as sq

    rng = np.random.default_rng(5)
    xyz = rng.random((300, 3)) * np.array([100.0, 100.0, 25.0])
    lib = rng.integers(0, 2, 300)  # interleaved libraries
    ad = _adata(xyz, library=pd.Categorical.from_codes(lib, ["a", "b"]))
    res = sq.gr.spatial_neighbors_knn(ad, n_neighs=5, library_key="library", copy=True)
    for c in (0, 1):
        sel = np.where(lib == c)[0]
        ref_adj, ref_dst = O.spatial_graph(xyz[sel], "knn", n_neighs=5)
        assert _same(res.connectivities[sel, :][:, sel], ref_adj)
        assert _same(res.distances[sel, :][:, sel], ref_dst)
    assert res.connectivities[np.where(lib == 0)[0], :][:, np.where(lib == 1)[0]].nnz == 0


# ---------------------------------------------------------------------------------------- 6. edges of the contract


def test_edges_of_the_contract(L, ctx):
    import squidpy_amd as sq

    rng = np.random.default_rng(9)
    for fn, kw in ((sq.gr.spatial_neighbors_knn, {}), (sq.gr.spatial_neighbors_radius, dict(radius=0.2)), (sq.gr.spatial_neighbors_grid, {})):
        with pytest.raises(NotImplementedError, match="2-D or 3-D coordinates"):
            fn(_adata(rng.random((30, 4))), copy=True, **kw)
        with pytest.raises(NotImplementedError, match="2-D or 3-D coordinates"):
            fn(_adata(rng.random((30, 1))), copy=True, **kw)
    for bad in (rng.random((30, 4)), rng.random((30, 1)), rng.random(30)):
        with pytest.raises(ValueError, match=r"\(n, 2\) or \(n, 3\)"):
            L.knn_self(ctx, bad, 3)
        with pytest.raises(ValueError, match=r"\(n, 2\) or \(n, 3\)"):
            L.radius_self(ctx, bad, 0.1)
    xyz = rng.random((100, 3))
    xyz[41, 2] = np.nan
    with pytest.raises(L.SqgrError, match="coordinate 41 is not finite"):
        L.knn_self(ctx, xyz, 3)
    with pytest.raises(L.SqgrError, match="coordinate 41 is not finite"):
        L.radius_self(ctx, xyz, 0.1)
    xy = rng.random((100, 2))
    xy[41, 1] = np.nan
    with pytest.raises(L.SqgrError, match="coordinate 41 is not finite"):  # the 2-D message
        L.knn_self(ctx, xy, 3)
    with pytest.raises(L.SqgrError, match="n_neighbors=65 > 64 is not supported"):
        L.knn_self(ctx, rng.random((200, 3)), 65)
    dist, idx = L.knn_self(ctx, rng.random((200, 3)), 64)  # the largest supported k
    assert dist.shape == (200, 64) and (np.diff(dist, axis=1) >= 0).all()


# ------------------------------------------------------------------------------------------------- 7. downstream


def test_nhood_enrichment_consumes_the_3d_graph(L):
    import squidpy_amd as sq

    rng = np.random.default_rng(3)
    xyz = rng.random((2000, 3)) * np.array([500.0, 500.0, 80.0])
    cluster = pd.Categorical.from_codes(rng.integers(0, 5, 2000), list("abcde"))
    ad = _adata(xyz, cluster=cluster)
    sq.gr.spatial_neighbors_knn(ad, n_neighs=6)
    got = sq.gr.nhood_enrichment(ad, "cluster", n_perms=50, seed=0, copy=True)
    ref = _adata(xyz, cluster=cluster)
    ref_adj, ref_dst = O.spatial_graph(xyz, "knn", n_neighs=6)
    assert _same(ad.obsp["spatial_connectivities"], ref_adj) and _same(ad.obsp["spatial_distances"], ref_dst)
    ref.obsp["spatial_connectivities"], ref.obsp["spatial_distances"] = ref_adj, ref_dst
    want = sq.gr.nhood_enrichment(ref, "cluster", n_perms=50, seed=0, copy=True)
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.zscore, want.zscore)
    assert got.zscore.shape == (5, 5) and np.isfinite(got.zscore).all()
