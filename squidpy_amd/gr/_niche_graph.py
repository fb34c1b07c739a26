"""``sc.pp.neighbors(adata_embedding, n_neighbors=15, use_rep="X")`` — the call the reference's ``neighborhood`` and ``utag`` niche flavours
make between their embedding and ``sc.tl.leiden`` (gr/_niche.py:1417) — with the neighbour search and UMAP's fuzzy weights on the GPU
(``csrc/sqgr_knn_nd.hip``) and the symmetrisation on the host, and ``niche_scale``, the ``sc.pp.scale`` the ``neighborhood`` flavour
applies to its profile first (gr/_niche.py:1225).  Neither this module nor the library imports scanpy, umap-learn or sklearn."""

from __future__ import annotations

import numbers
from typing import Any, NamedTuple

import numpy as np
from scipy import sparse

from .._lib import SqgrError, default_context
from .._lib import fuzzy_knn as _fuzzy_knn
from .._lib import knn_nd as _knn_nd
from .._utils import _save_data

__all__ = ["niche_knn", "niche_neighbors", "niche_scale", "NicheNeighborsResult", "connectivities_from_memberships",
           "KNN_MAX_FEATURES", "KNN_MAX_NEIGHBORS"]

KNN_MAX_FEATURES = 256   # KN_MAX_D of csrc/sqgr_knn_nd.hip
KNN_MAX_NEIGHBORS = 64   # KN_MAX_K: neighbours besides the point itself


class NicheNeighborsResult(NamedTuple):
    """What ``niche_neighbors`` returns for an array or with ``copy=True``: scanpy's ``obsp["distances"]`` and
    ``obsp["connectivities"]`` (float64 CSR here), the ``(n, n_neighbors - 1)`` neighbour indices and distances they were built from, and
    UMAP's per-row ``rho`` and ``sigma``."""

    distances: sparse.csr_matrix
    connectivities: sparse.csr_matrix
    knn_indices: np.ndarray
    knn_distances: np.ndarray
    rho: np.ndarray
    sigma: np.ndarray


def _check_n_neighbors(n_neighbors: Any) -> int:
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, numbers.Integral):
        raise TypeError(f"Expected `n_neighbors` to be of type `int`, found `{type(n_neighbors).__name__}`.")
    if n_neighbors < 2:
        raise ValueError(f"Expected `n_neighbors` to be at least 2 (it counts the point itself), found `{n_neighbors}`.")
    return int(n_neighbors)


def _validated(X: Any, n_neighbors: Any) -> tuple[np.ndarray, int]:
    """``X`` as a float32 or float64 matrix with unit stride along a row and ``k = n_neighbors - 1``; every refusal is raised here."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected a 2-D array, found shape `{X.shape}`.")
    k = _check_n_neighbors(n_neighbors) - 1
    n, d = X.shape
    if not (1 <= d <= KNN_MAX_FEATURES) or k > KNN_MAX_NEIGHBORS or n >= 2**31:
        raise NotImplementedError(
            f"The feature-space neighbour search supports 1 to {KNN_MAX_FEATURES} features, `n_neighbors` up to {KNN_MAX_NEIGHBORS + 1} and "
            f"2**31 - 1 rows; found {d} features, n_neighbors={k + 1} and {n} rows."
        )
    if k > n - 1:
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {k + 1}")
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    if X.strides[1] != X.itemsize or X.strides[0] % X.itemsize or X.strides[0] < d * X.itemsize:
        X = np.ascontiguousarray(X)
    if not np.isfinite(X).all():
        raise ValueError("Input X contains NaN or infinity.")
    return X, k


def niche_knn(X: Any, n_neighbors: int = 15, *, device: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """The ``n_neighbors - 1`` nearest other rows of every row of ``X (n, D)`` under the euclidean metric, exactly, at every size:
    ``(indices int32 (n, n_neighbors - 1), distances float64 (n, n_neighbors - 1))``, ascending by ``(distance, index)`` — ties go to
    the smaller index.  ``n_neighbors`` counts the point itself, as scanpy's does; the point itself is excluded by index, so a
    duplicate row is a neighbour at distance 0.

    The distances are ``sqrt(sum_j (x_ij - x_cj)**2)`` with ``j`` ascending and every operation rounded on its own, in float64 (a
    float32 ``X`` is widened exactly, other dtypes are cast): what sklearn's ``NearestNeighbors(algorithm="kd_tree")`` returns, bit for
    bit.  All pairs are computed on the GPU (``csrc/sqgr_knn_nd.hip``).  Supported are ``1 <= D <= 256``, ``2 <= n_neighbors <= 65`` and
    ``n < 2**31`` (``NotImplementedError`` beyond); NaN or infinity is a ``ValueError``.  Two calls return the same bytes."""
    X, k = _validated(X, n_neighbors)
    try:
        idx, d2 = _knn_nd(default_context(device), X, k)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        raise
    return idx, np.sqrt(d2)


def niche_scale(X: Any) -> np.ndarray:
    """``(X - X.mean(0)) / s`` in float64 with ``s = X.std(0, ddof=1)`` and ``s[s == 0] = 1``: what ``sc.pp.scale(zero_center=True)``
    is documented to do, and what the reference's ``neighborhood`` flavour applies to its profile in front of ``sc.pp.neighbors``
    (gr/_niche.py:1225) — ``niche_neighbors(niche_scale(niche_nhood_profile(...)))`` is that flavour's whole Leiden input.  Runs on
    the host with numpy (one pass over the matrix, milliseconds next to the search).  scanpy's own variance formula is not pinned:
    scanpy cannot be imported where this library is tested, so the last digits may differ from ``sc.pp.scale``'s."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(f"Expected a 2-D array, found shape `{X.shape}`.")
    if X.shape[0] < 2:
        raise ValueError(f"Expected at least 2 rows, found `{X.shape[0]}`.")
    s = X.std(0, ddof=1)
    s[s == 0] = 1.0
    return (X - X.mean(0)) / s


def connectivities_from_memberships(knn_indices: np.ndarray, vals: np.ndarray) -> sparse.csr_matrix:
    """UMAP's fuzzy union with ``set_op_mix_ratio = 1``: ``W + W.T - W * W.T`` for the CSR matrix ``W`` of ``vals`` (zeros eliminated)."""
    n, k = knn_indices.shape
    W = sparse.csr_matrix((vals.ravel(), knn_indices.ravel().astype(np.int32), np.arange(0, n * k + 1, k, dtype=np.int64)), shape=(n, n))
    W.eliminate_zeros()
    Wt = W.T.tocsr()
    conn = (W + Wt - W.multiply(Wt)).tocsr()
    conn.eliminate_zeros()
    conn.sort_indices()
    return conn


def _distance_graph(knn_indices: np.ndarray, knn_distances: np.ndarray) -> sparse.csr_matrix:
    """Canonical CSR with ``k`` stored entries per row; stored zeros (duplicate rows) are kept."""
    n, k = knn_indices.shape
    order = np.argsort(knn_indices, axis=1, kind="stable")
    return sparse.csr_matrix(
        (np.take_along_axis(knn_distances, order, 1).ravel(), np.take_along_axis(knn_indices, order, 1).ravel(),
         np.arange(0, n * k + 1, k, dtype=np.int64)), shape=(n, n))


def niche_neighbors(
    data: Any,
    n_neighbors: int = 15,
    *,
    use_rep: str | None = None,
    key_added: str | None = None,
    copy: bool = False,
    device: int | None = None,
) -> NicheNeighborsResult | None:
    """``sc.pp.neighbors(adata, n_neighbors, use_rep=...)`` with ``method="umap"`` and the euclidean metric — the call the reference's
    ``neighborhood`` and ``utag`` flavours make on their embedding (gr/_niche.py:1417); the call the reference makes next is
    ``sc.tl.leiden``, which reads only the two sparse matrices written here and can run directly on the result wherever scanpy is
    installed.

    ``data`` is an ``(n, D)`` array or an AnnData-like object (``use_rep=None`` selects ``X``, otherwise ``obsm[use_rep]``).

    - The neighbours are exact at every size: all pairs on the GPU, ties to the smaller index (``niche_knn``).  scanpy's own are exact
      below 4096 rows only (above it falls back to an approximate descent whose result depends on its seed), and there it uses the
      norm-expansion formula ``|x|^2 - 2 x.y + |y|^2``, so its distances differ from these in the last digits.
    - ``distances``: canonical CSR with ``n_neighbors - 1`` stored entries per row; stored zeros (duplicate rows) are kept.
    - ``connectivities``: UMAP's documented algorithm restated in float64 — per row ``rho`` (the first positive distance,
      ``local_connectivity = 1``) and ``sigma`` (64 bisection sweeps at most, towards ``sum_j exp(-(d_j - rho) / sigma) =
      log2(n_neighbors)`` within 1e-5, then the ``1e-3 * mean`` floor) on the GPU, memberships ``exp(-(d_j - rho) / sigma)``, and the
      fuzzy union ``W + W.T - W * W.T`` (``set_op_mix_ratio = 1``) with scipy on the host.  scanpy and umap-learn store float32.
    - Neither scanpy nor umap-learn can be imported where this library is tested, so parity with them is unpinned, like Moran's I
      against scanpy; the search itself is pinned bit for bit to sklearn's KD-tree.

    With ``copy=True``, or for an array, returns a ``NicheNeighborsResult``.  Otherwise writes scanpy's slots:
    ``obsp["distances"]``, ``obsp["connectivities"]`` and ``uns["neighbors"] = {"connectivities_key", "distances_key", "params":
    {"n_neighbors", "method": "umap", "metric": "euclidean"[, "use_rep"]}}``; with ``key_added`` the keys are
    ``f"{key_added}_distances"`` and ``f"{key_added}_connectivities"`` under ``uns[key_added]``.  Limits and refusals are those of
    ``niche_knn``.  Under a process group every rank computes the whole result."""
    is_array = isinstance(data, np.ndarray) or not hasattr(data, "obsp")
    if is_array:
        if use_rep is not None:
            raise ValueError("`use_rep` selects a representation of an AnnData-like object; found an array.")
        X = data
    elif use_rep is None or use_rep == "X":
        X = data.X
        if sparse.issparse(X):
            X = X.toarray()
    else:
        if use_rep not in data.obsm:
            raise KeyError(f"Representation `{use_rep}` not found in `adata.obsm`.")
        X = data.obsm[use_rep]
    X, k = _validated(X, n_neighbors)
    ctx = default_context(device)
    try:
        idx, d2 = _knn_nd(ctx, X, k)
        dist = np.sqrt(d2)
        mean_all = float(dist.sum() / (dist.shape[0] * (k + 1)))
        rho, sigma, _, vals = _fuzzy_knn(ctx, dist, mean_all)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        raise
    res = NicheNeighborsResult(_distance_graph(idx, dist), connectivities_from_memberships(idx, vals), idx, dist, rho, sigma)
    if copy or is_array:
        return res
    if key_added is None:
        uns_key, dist_key, conn_key = "neighbors", "distances", "connectivities"
    else:
        uns_key, dist_key, conn_key = key_added, f"{key_added}_distances", f"{key_added}_connectivities"
    params: dict[str, Any] = {"n_neighbors": k + 1, "method": "umap", "metric": "euclidean"}
    if use_rep is not None:
        params["use_rep"] = use_rep
    _save_data(data, attr="obsp", key=dist_key, data=res.distances)
    _save_data(data, attr="obsp", key=conn_key, data=res.connectivities)
    _save_data(data, attr="uns", key=uns_key, data={"connectivities_key": conn_key, "distances_key": dist_key, "params": params})
    return None
