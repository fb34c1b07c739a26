"""``sc.tl.leiden`` as the reference's ``neighborhood`` and ``utag`` niche flavours call it (gr/_niche.py:1412-1438), and the two flavours
as drop-ins on top of it: ``niche_leiden`` (``csrc/sqgr_leiden.hip``: a deterministic synchronous Leiden on exact integer weights),
``calculate_niche_neighborhood`` and ``calculate_niche_utag``.  Neither this module nor the library imports scanpy, igraph or
leidenalg; leidenalg is randomised, so parity with it is unpinned — what is pinned is in DESIGN §3.10."""

from __future__ import annotations

import numbers
from fractions import Fraction
from typing import Any, NamedTuple

import numpy as np
import pandas as pd
from scipy import sparse

from .._lib import SqgrError, default_context
from .._lib import leiden as _leiden
from .._utils import _save_data, extract_adata_if_sdata, logg
from . import _niche as N
from ._niche_graph import NicheNeighborsResult, _check_n_neighbors, niche_neighbors, niche_scale

__all__ = ["niche_leiden", "quantise_weights", "LeidenResult", "calculate_niche_neighborhood", "calculate_niche_utag", "LEIDEN_WEIGHT_BITS"]

LEIDEN_WEIGHT_BITS = 24  # LD_WEIGHT_BITS of csrc/sqgr_leiden.hip


class LeidenResult(NamedTuple):
    """What ``niche_leiden`` returns for a matrix or with ``copy=True``: ``labels`` int32 in ``[0, n_communities)`` with 0 the largest
    community (ties by smallest member), ``quality`` ``Q = sum_c (in_c / 2m - resolution (tot_c / 2m)**2)`` of the quantised graph as
    a float formed from exact integers, and how many iterations, levels and sweeps the run took."""

    labels: np.ndarray
    n_communities: int
    quality: float
    iterations: int
    levels: int
    sweeps: int


def quantise_weights(conn: Any) -> sparse.csr_matrix:
    """The host step in front of ``sqgr_leiden``: ``conn`` as a canonical CSR matrix (rows ascending, duplicates summed, stored zeros
    dropped) whose values are ``max(1, rint(w / w_max * 2**24))`` as int32.  Every weight sum on the device is then an exact integer.
    A weight below ``w_max * 2**-25`` counts as ``w_max * 2**-24``.  ``ValueError`` for a matrix that is not square, has a negative,
    NaN or infinite value, a non-zero diagonal, or is not symmetric (values included).  The caller's matrix is not changed."""
    a = sparse.csr_matrix(conn, copy=True)
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"Expected a square matrix, found shape `{a.shape}`.")
    a.sum_duplicates()
    data = np.asarray(a.data, dtype=np.float64)
    if not np.isfinite(data).all():
        raise ValueError("The graph contains NaN or infinity.")
    if (data < 0).any():
        raise ValueError("The graph contains a negative weight.")
    a = sparse.csr_matrix((data, a.indices, a.indptr), shape=a.shape)
    a.eliminate_zeros()
    a.sort_indices()
    if a.diagonal().any():
        raise ValueError("The graph has a self loop (a non-zero diagonal entry).")
    if (a != a.T).nnz:
        raise ValueError("The graph is not symmetric.")
    q = np.zeros(0, dtype=np.int32)
    if a.nnz:
        q = np.maximum(1, np.rint(a.data / a.data.max() * float(2**LEIDEN_WEIGHT_BITS))).astype(np.int32)
    return sparse.csr_matrix((q, a.indices.astype(np.int32), a.indptr.astype(np.int64)), shape=a.shape)


def _check_two_m(two_m: int) -> None:
    if two_m >= 2**62:
        raise NotImplementedError(f"The sum of all quantised weights is {two_m}; the kernels' 64-bit sums hold less than 2**62.")


def _check_resolution(resolution: Any) -> float:
    if isinstance(resolution, bool) or not isinstance(resolution, numbers.Real):
        raise TypeError(f"Expected `resolution` to be a number, found `{type(resolution).__name__}`.")
    if not np.isfinite(resolution) or resolution <= 0:
        raise ValueError(f"Expected `resolution` to be finite and positive, found `{resolution}`.")
    return float(resolution)


def _check_n_iterations(n_iterations: Any) -> int:
    if isinstance(n_iterations, bool) or not isinstance(n_iterations, numbers.Integral):
        raise TypeError(f"Expected `n_iterations` to be of type `int`, found `{type(n_iterations).__name__}`.")
    if n_iterations == 0 or n_iterations >= 2**31:
        raise ValueError(f"Expected `n_iterations` to be positive, or negative for 'until an iteration changes nothing'; found `{n_iterations}`.")
    return int(n_iterations)


def _connectivities(data: Any, neighbors_key: str | None) -> tuple[Any, bool]:
    """(matrix, is_object)."""
    if isinstance(data, NicheNeighborsResult):
        return data.connectivities, False
    if sparse.issparse(data) or isinstance(data, np.ndarray):
        if neighbors_key is not None:
            raise ValueError("`neighbors_key` selects a slot of an AnnData-like object; found a matrix.")
        return data, False
    key = "neighbors" if neighbors_key is None else neighbors_key
    if key not in data.uns:
        raise KeyError(f"No `adata.uns[{key!r}]`: run `niche_neighbors` first (or pass `neighbors_key`).")
    conn_key = data.uns[key]["connectivities_key"]
    if conn_key not in data.obsp:
        raise KeyError(f"`adata.uns[{key!r}]` names `adata.obsp[{conn_key!r}]`, which does not exist.")
    conn = data.obsp[conn_key]
    if conn.shape != (data.n_obs, data.n_obs):
        raise ValueError(f"Expected `adata.obsp[{conn_key!r}]` of shape `{(data.n_obs, data.n_obs)}`, found `{conn.shape}`.")
    return conn, True


def _quality(q: sparse.csr_matrix, labels: np.ndarray, sum_in: int, resolution: float) -> float:
    k = np.asarray(q.sum(axis=1, dtype=np.int64)).ravel()
    two_m = int(k.sum())
    if two_m == 0:
        return 0.0
    tot = np.zeros(int(labels.max()) + 1, dtype=np.int64)
    np.add.at(tot, labels, k)
    sum_sq = sum(t * t for t in tot.tolist())
    return float(Fraction(sum_in, two_m) - Fraction(resolution) * Fraction(sum_sq, two_m * two_m))


def niche_leiden(
    data: Any,
    resolution: float = 1.0,
    *,
    neighbors_key: str | None = None,
    key_added: str = "leiden",
    n_iterations: int = -1,
    copy: bool = False,
    device: int | None = None,
) -> LeidenResult | None:
    """``sc.tl.leiden(adata, resolution, key_added=..., neighbors_key=..., n_iterations=...)`` with scanpy's defaults — the quality
    function of ``leidenalg.RBConfigurationVertexPartition`` on the weighted, undirected connectivities — on the GPU
    (``csrc/sqgr_leiden.hip``).

    ``data`` is a ``NicheNeighborsResult``, a symmetric scipy sparse matrix, or an AnnData-like object; for an object scanpy's lookup
    applies: ``obsp[uns[neighbors_key or "neighbors"]["connectivities_key"]]``.

    The algorithm is Leiden as a deterministic, synchronous variant (``include/sqgr.h`` states it operation by operation):

    - the weights are quantised once, ``max(1, rint(w / w_max * 2**24))`` (``quantise_weights``), so every sum is an exact integer;
    - local moving runs in synchronous sweeps in which the vertices that move are pairwise non-adjacent (a vertex that wants to move
      yields to a neighbour of better hashed priority), and of the vertices that want into the same community only those move whose
      gain survives all of them joining;
    - refinement is greedy where leidenalg draws at random (``theta = 0.01``); communities are connected by construction;
    - ``n_iterations=-1`` runs until an iteration changes nothing, at most 16 iterations.

    leidenalg is randomised — another seed gives other labels — so parity with it is not claimed.  Pinned are: the device against a
    numpy restatement bit for bit, the restatement against planted partitions, Leiden's connectivity guarantee, node stability, and
    its quality against networkx's Louvain.  Two calls return the same bytes.

    With ``copy=True``, or for a matrix, returns a ``LeidenResult``.  Otherwise writes ``obs[key_added]``, a ``pd.Categorical`` of
    ``"0"``, ``"1"``, … with the categories in numeric order and ``"0"`` the largest community, and ``uns[key_added] = {"params":
    {"resolution", "n_iterations"}}``.  ``ValueError`` for a resolution that is not finite and positive and for a graph
    ``quantise_weights`` refuses; ``NotImplementedError`` when the quantised weights sum to 2**62 or more.  Under a process group
    every rank computes the whole result."""
    # every refusal first: nothing has touched the device or the caller's object when one is raised
    conn, is_object = _connectivities(data, neighbors_key)
    resolution = _check_resolution(resolution)
    n_iterations = _check_n_iterations(n_iterations)
    q = quantise_weights(conn)
    n = q.shape[0]
    if n == 0:
        raise ValueError("Expected at least one observation.")
    _check_two_m(int(q.data.sum(dtype=np.int64)) if q.nnz < 2**31 else sum(q.data.tolist()))
    try:
        labels, stats = _leiden(default_context(device), q.indptr, q.indices, q.data, resolution, n_iterations)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        raise
    res = LeidenResult(labels, stats["n_communities"], _quality(q, labels, stats["sum_in"], resolution), stats["iterations"],
                       stats["levels"], stats["sweeps"])
    if copy or not is_object:
        return res
    categories = [str(c) for c in range(res.n_communities)]
    data.obs[key_added] = pd.Categorical(labels.astype(str), categories=categories)
    logg.info("Adding `adata.obs[%r]`", key_added)
    _save_data(data, attr="uns", key=key_added, data={"params": {"resolution": resolution, "n_iterations": n_iterations}})
    return None


# ---- the two flavours ------------------------------------------------------------------------------------------------------------------
def _resolution_list(resolutions: Any) -> list:
    """``_LeidenClusterer.__init__`` (gr/_niche.py:1409): a list is taken as it is, anything else is one resolution."""
    res = resolutions if isinstance(resolutions, list) else [resolutions]
    if not res:
        raise ValueError("Expected at least one resolution.")
    for r in res:
        _check_resolution(r)
    return res


def _leiden_cluster(obs: pd.DataFrame, embedding: np.ndarray, n_neighbors: int, resolutions: list, base: str, device: int | None) -> list[str]:
    """``_LeidenClusterer.cluster`` (gr/_niche.py:1412-1438): one column of ``str`` labels per resolution."""
    graph = niche_neighbors(embedding, n_neighbors, device=device)
    keys = []
    for res in resolutions:
        key = f"{base}_res={res}"
        keys.append(key)
        if key in obs.columns:
            logg.info("Overwriting existing column '%s'", key)
        obs[key] = list(niche_leiden(graph, res, device=device).labels.astype(str))
    return keys


def _library_sizes(adata: Any, library_key: str | None) -> list[int]:
    if library_key is None:
        return [adata.n_obs]
    N._assert_key_in_adata(adata, library_key, "obs")
    return [int(c) for c in adata.obs[library_key].value_counts(sort=False) if c > 0]


def _check_rows(sizes: list[int], n_neighbors: int, least: int = 1) -> None:
    for n in sizes:
        if n < max(n_neighbors, least):
            raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {n_neighbors}")


def calculate_niche_neighborhood(
    data: Any,
    groups: str,
    resolutions: float | list[float],
    n_neighbors: int = 15,
    spatial_connectivities_key: str = "spatial_connectivities",
    scale: bool = True,
    distance: int = 1,
    abs_nhood: bool = False,
    n_hop_weights: list[float] | None = None,
    min_niche_size: int | None = None,
    mask: pd.Series | None = None,
    library_key: str | None = None,
    inplace: bool = True,
    table_key: str | None = None,
    *,
    device: int | None = None,
) -> Any:
    """Compute niche assignments with the neighborhood flavour (drop-in for ``squidpy.gr.calculate_niche_neighborhood``,
    gr/_niche.py:275-348): ``niche_nhood_profile`` → ``niche_scale`` (when ``scale``) → ``niche_neighbors(n_neighbors)`` →
    ``niche_leiden`` per resolution, every stage on the GPU.  ``obs[f"nhood_niche_res={res}"]`` gets the labels as ``str``, one column
    per resolution (``resolutions`` is a float or a list).

    ``mask``, ``min_niche_size`` and ``library_key`` follow ``_postprocess_niche_results`` and ``_calculate_niche_custom``: masked or
    too-small niches become ``"not_a_niche"``; with ``library_key`` every library runs on its own rows and its own sub-graph (the
    reference's ``adata[lib_indices].copy()``), in ``obs[library_key].unique()`` order, and its labels are prefixed ``lib={id}_``.
    Where the stages differ from scanpy's they say so themselves (``niche_neighbors``: exact neighbours at every size, float64;
    ``niche_leiden``: a deterministic Leiden, parity with leidenalg unpinned).  Every refusal is raised before anything runs.

    Returns ``None`` if ``inplace=True``, else a copy of ``adata`` with the columns added."""
    orig_adata = extract_adata_if_sdata(data, table_key=table_key)
    if not isinstance(groups, str):
        raise TypeError(f"Expected `groups` to be of type `str`, found `{type(groups).__name__}`.")
    N._assert_key_in_adata(orig_adata, groups, "obs")
    res = _resolution_list(resolutions)
    n_neighbors = _check_n_neighbors(n_neighbors)
    distance = N._check_distance(distance)
    N.hop_weights(n_hop_weights, distance)
    N._canonical_graph(orig_adata, spatial_connectivities_key)
    _check_rows(_library_sizes(orig_adata, library_key), n_neighbors, 2 if scale else 1)

    def cluster(adata: Any, obs: pd.DataFrame, rows: np.ndarray | None) -> list[str]:
        part = adata if rows is None else adata[rows, :]
        profile = N.niche_nhood_profile(part, groups, spatial_connectivities_key, distance, abs_nhood, n_hop_weights, device=device)
        return _leiden_cluster(obs, niche_scale(profile) if scale else profile, n_neighbors, res, "nhood_niche", device)

    return N.calculate_niche_custom(orig_adata, cluster, min_niche_size, mask, library_key, inplace)


def calculate_niche_utag(
    data: Any,
    resolutions: float | list[float],
    n_neighbors: int = 15,
    spatial_connectivities_key: str = "spatial_connectivities",
    min_niche_size: int | None = None,
    mask: pd.Series | None = None,
    library_key: str | None = None,
    inplace: bool = True,
    table_key: str | None = None,
    *,
    device: int | None = None,
) -> Any:
    """Compute niche assignments with the utag flavour (drop-in for ``squidpy.gr.calculate_niche_utag``, gr/_niche.py:352-399):
    ``niche_utag_embedding`` (the row-normalised graph times ``adata.X``, then the default PCA) → ``niche_neighbors(n_neighbors)`` →
    ``niche_leiden`` per resolution, every stage on the GPU.  ``obs[f"utag_niche_res={res}"]`` gets the labels as ``str``.
    ``mask``, ``min_niche_size``, ``library_key``, ``inplace`` and the refusals are those of ``calculate_niche_neighborhood``."""
    orig_adata = extract_adata_if_sdata(data, table_key=table_key)
    res = _resolution_list(resolutions)
    n_neighbors = _check_n_neighbors(n_neighbors)
    N._canonical_graph(orig_adata, spatial_connectivities_key)
    n_vars = N._feature_matrix(orig_adata).shape[1]
    sizes = _library_sizes(orig_adata, library_key)
    _check_rows(sizes, n_neighbors)
    for n in sizes:
        N._check_pca_shape(n, n_vars, None)

    def cluster(adata: Any, obs: pd.DataFrame, rows: np.ndarray | None) -> list[str]:
        part = adata if rows is None else adata[rows, :]
        embedding = N.niche_utag_embedding(part, spatial_connectivities_key, device=device)
        return _leiden_cluster(obs, embedding, n_neighbors, res, "utag_niche", device)

    return N.calculate_niche_custom(orig_adata, cluster, min_niche_size, mask, library_key, inplace)
