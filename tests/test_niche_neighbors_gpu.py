"""GPU: ``csrc/sqgr_knn_nd.hip`` and ``sq.gr.niche_neighbors`` on the cases of tests/niche_neighbors_cases.py.

- Search kernel: indices and ``d2`` ``==`` the numpy restatement (tests/niche_neighbors_oracle.py) on every case, tied ones included —
  the ``(d2, index)`` order makes the answer unique; ``sqrt(d2)`` ``==`` sklearn's KD-tree distances; float32 input ``==`` its float64
  widening; two calls, the same bytes.
- Bandwidth kernel: ``rho``, ``iters`` and ``sigma`` ``==`` the restatement bit for bit (no decision of the search is closer than 1e-11
  to flipping, tests/test_niche_neighbors_cpu.py); ``vals`` within ``DEVICE_EXP_ULP + LIBM_EXP_ULP`` units of the last place of the
  restatement's value.  The installed HIP documentation states no bound for the device's float64 ``exp``, so ``DEVICE_EXP_ULP`` is twice
  the worst error observed against ``exp`` in extended precision over a sweep of 2.52e7 arguments in [-745, 0]: 0.881 ulp
  (``tools/niche_neighbors_time.py``, leg ``exp_sweep``; profiles/niche_neighbors_time.json).  ``LIBM_EXP_ULP`` is the bound
  the C library's manual lists for ``exp`` (the restatement calls ``math.exp``).
- Front end: ``obsp["distances"]`` ``==`` sklearn's ``kneighbors_graph(mode="distance")`` from the KD-tree; connectivities ``==`` the scipy
  formula on the device's ``vals``.
- Limits: each limit ``sqgr_knn_nd_info`` reports, at the limit and one past it."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import squidpy_amd as sq
from squidpy_amd import AnnDataLite, _lib
from squidpy_amd._lib import SqgrError, default_context

from tests import niche_neighbors_cases as NC
from tests import niche_neighbors_oracle as O

pytestmark = pytest.mark.gpu

DEVICE_EXP_ULP = 2 * 0.881  # twice the worst observed: see the module docstring
LIBM_EXP_ULP = 1.0


@functools.lru_cache(maxsize=None)
def device_knn(name: str):
    """The case's ``(indices, d2)`` from the device, twice."""
    ctx = default_context(None)
    k = NC.CASES[name].n_neighbors - 1
    return _lib.knn_nd(ctx, NC.data(name), k), _lib.knn_nd(ctx, NC.data(name), k)


@functools.lru_cache(maxsize=None)
def device_fuzzy(name: str):
    dist = np.sqrt(NC.oracle_knn(name)[1])
    mean_all = float(dist.sum() / (dist.shape[0] * NC.CASES[name].n_neighbors))
    return _lib.fuzzy_knn(default_context(None), dist, mean_all)


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_knn_equals_oracle(name):
    (idx, d2), _ = device_knn(name)
    ref_idx, ref_d2 = NC.oracle_knn(name)
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(d2, ref_d2)
    assert np.array_equal(idx, ref_idx)


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_knn_distances_equal_kdtree(name):
    (_, d2), _ = device_knn(name)
    assert np.array_equal(np.sqrt(d2), NC.kdtree(name)[0])


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_knn_twice_the_same_bytes(name):
    (idx, d2), (idx2, d22) = device_knn(name)
    assert idx.tobytes() == idx2.tobytes() and d2.tobytes() == d22.tobytes()


def test_float32_equals_its_widening_and_strided_input():
    x = NC.data("float32")
    assert x.dtype == np.float32
    (idx, d2), _ = device_knn("float32")
    idx64, d264 = _lib.knn_nd(default_context(None), x.astype(np.float64), 14)
    assert np.array_equal(idx, idx64) and np.array_equal(d2, d264)
    for dtype in (np.float32, np.float64):  # rows ld > D values apart
        wide = np.zeros((x.shape[0], x.shape[1] + 5), dtype=dtype)
        wide[:, : x.shape[1]] = x
        idx_w, d2_w = _lib.knn_nd(default_context(None), wide[:, : x.shape[1]], 14)
        assert np.array_equal(idx_w, idx) and np.array_equal(d2_w, d2)


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_fuzzy_equals_oracle(name):
    rho, sigma, iters, vals = device_fuzzy(name)
    f = NC.oracle_fuzzy(name)
    assert np.array_equal(rho, f.rho)
    assert np.array_equal(iters, f.iters)
    assert np.array_equal(sigma, f.sigma)
    err = np.abs(vals - f.vals) / np.spacing(f.vals)  # in units of the last place of the value (subnormal values included)
    print(f"{name}: vals differ by at most {float(err.max()):.3f} ulp")
    assert (err <= DEVICE_EXP_ULP + LIBM_EXP_ULP).all()


def test_fuzzy_twice_the_same_bytes():
    dist = np.sqrt(NC.oracle_knn("profiles")[1])
    a = _lib.fuzzy_knn(default_context(None), dist, 0.25)
    b = device_fuzzy.__wrapped__("profiles")
    c = device_fuzzy("profiles")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(b, c))
    assert a[0].tobytes() == b[0].tobytes()  # rho does not depend on mean_all


@pytest.mark.parametrize("name", ["n1000_d30_m15", "profiles", "duplicates", "float32"])
def test_front_end(name):
    from sklearn.neighbors import NearestNeighbors

    c = NC.CASES[name]
    adata = AnnDataLite(X=np.zeros((c.n, 1)), obsm={"X_emb": NC.data(name)})
    assert sq.gr.niche_neighbors(adata, c.n_neighbors, use_rep="X_emb") is None
    ref = NearestNeighbors(n_neighbors=c.n_neighbors - 1, algorithm="kd_tree").fit(NC.data(name)).kneighbors_graph(mode="distance")
    ref.sort_indices()
    got = adata.obsp["distances"]
    assert got.has_canonical_format and got.nnz == c.n * (c.n_neighbors - 1)
    assert np.array_equal(got.indptr, ref.indptr)
    if name in NC.CONTINUOUS:  # tied rows: sklearn's choice among equal distances is its own
        assert np.array_equal(got.indices, ref.indices) and np.array_equal(got.data, ref.data)
    else:
        assert np.array_equal(np.sort(got.data.reshape(c.n, -1), axis=1), np.sort(ref.data.reshape(c.n, -1), axis=1))
    res = sq.gr.niche_neighbors(NC.data(name), c.n_neighbors)
    assert np.array_equal(res.distances.toarray(), got.toarray())
    idx, _ = NC.oracle_knn(name)
    assert np.array_equal(res.knn_indices, idx)
    rho, sigma, _, vals = device_fuzzy(name)
    assert np.array_equal(res.rho, rho) and np.array_equal(res.sigma, sigma)
    conn = adata.obsp["connectivities"]
    assert np.array_equal(conn.toarray(), O.connectivities(idx, vals).toarray())
    assert np.array_equal(res.connectivities.toarray(), conn.toarray())
    assert adata.uns["neighbors"]["params"] == {"n_neighbors": c.n_neighbors, "method": "umap", "metric": "euclidean", "use_rep": "X_emb"}


def test_limits():
    info = _lib.knn_nd_info()
    ctx = default_context(None)
    rng = np.random.default_rng(5)
    max_d, max_k = info["max_features"], info["max_neighbors"]
    x = rng.normal(size=(max_k + 1, max_d))
    idx, d2 = _lib.knn_nd(ctx, x, max_k)  # both limits at once, k = n - 1
    ref_idx, ref_d2 = O.knn(x, max_k)
    assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)
    y = rng.normal(size=(max_k + 3, 3))
    for bad_x, bad_k in ((np.zeros((max_k + 3, max_d + 1)), 3), (y, max_k + 1), (y[:5], 5)):
        with pytest.raises(SqgrError) as exc:
            _lib.knn_nd(ctx, bad_x, bad_k)
        assert exc.value.status == -4
    with pytest.raises(NotImplementedError):
        sq.gr.niche_knn(np.zeros((max_k + 3, max_d + 1)))
    with pytest.raises(NotImplementedError):
        sq.gr.niche_knn(y, max_k + 2)
    assert sq.gr.niche_knn(y, max_k + 1)[0].shape == (max_k + 3, max_k)
    with pytest.raises(SqgrError) as exc:
        _lib.fuzzy_knn(ctx, np.ones((4, max_k + 1)), 1.0)
    assert exc.value.status == -4
    assert _lib.fuzzy_knn(ctx, np.ones((4, max_k)), 1.0)[3].shape == (4, max_k)
