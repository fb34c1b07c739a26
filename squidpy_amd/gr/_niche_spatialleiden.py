"""The reference's fourth niche flavour, ``calculate_niche_spatialleiden`` (gr/_niche.py:466-620): multiplex Leiden on a latent and a
spatial graph over the same cells, as ``spatialleiden`` runs it through leidenalg's ``optimise_partition_multiplex``.  Here:
``quantise_layers`` (the host step), ``niche_spatialleiden`` (``csrc/sqgr_leiden_multiplex.hip``: the deterministic synchronous Leiden
of ``niche_leiden`` on two layers) and the drop-in on top of it.  Neither this module nor the library imports spatialleiden, leidenalg
or igraph; leidenalg is randomised, so parity with it is unpinned — what is pinned is in DESIGN §3.11."""

from __future__ import annotations

import numbers
from fractions import Fraction
from typing import Any, NamedTuple

import numpy as np
import pandas as pd
from scipy import sparse

from .._lib import SqgrError, default_context
from .._lib import leiden_multiplex as _leiden_multiplex
from .._utils import _save_data, extract_adata_if_sdata, logg
from . import _niche as N
from ._niche_leiden import LEIDEN_WEIGHT_BITS, _check_n_iterations, _check_resolution, _check_two_m

__all__ = ["niche_spatialleiden", "quantise_layers", "MultiplexLeidenResult", "calculate_niche_spatialleiden"]

LAYERS = ("latent", "spatial")


class MultiplexLeidenResult(NamedTuple):
    """What ``niche_spatialleiden`` returns for a pair of matrices or with ``copy=True``: ``labels`` int32 in ``[0, n_communities)`` with 0
    the largest community (ties by smallest member); ``quality``, the multiplex objective ``sum_l a_l sum_c (in^l_c - resolution_l
    (tot^l_c)**2 / 2m_l)`` (``a = (1, layer_ratio)``) of the quantised layers as a float formed from exact integers; per layer
    ``(latent, spatial)`` the inner weight ``sum_in`` and the total weight ``two_m``; and how many iterations, levels and sweeps the
    run took."""

    labels: np.ndarray
    n_communities: int
    quality: float
    sum_in: tuple[int, int]
    two_m: tuple[int, int]
    iterations: int
    levels: int
    sweeps: int


def _pair(value: Any, name: str, check: Any) -> tuple:
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"Expected `{name}` to be one value or a `(latent, spatial)` pair, found {len(value)} values.")
        return check(value[0]), check(value[1])
    return check(value), check(value)


def _check_bool(value: Any) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise TypeError(f"Expected `use_weights` to be a `bool` or a pair of them, found `{type(value).__name__}`.")
    return bool(value)


def _check_ratio(layer_ratio: Any) -> float:
    if isinstance(layer_ratio, bool) or not isinstance(layer_ratio, numbers.Real):
        raise TypeError(f"Expected `layer_ratio` to be a number, found `{type(layer_ratio).__name__}`.")
    if not np.isfinite(layer_ratio) or layer_ratio <= 0:
        raise ValueError(f"Expected `layer_ratio` to be finite and positive, found `{layer_ratio}`.")
    return float(layer_ratio)


def _undirected(conn: Any, name: str, use_weights: bool) -> sparse.csr_matrix:
    """``W = A + A^T`` in float64 of one layer, canonical: an undirected igraph built from a stored adjacency has one edge per entry."""
    a = sparse.csr_matrix(conn, copy=True)
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"Expected the {name} layer to be a square matrix, found shape `{a.shape}`.")
    a.sum_duplicates()
    data = np.asarray(a.data, dtype=np.float64)
    if not np.isfinite(data).all():
        raise ValueError(f"The {name} layer contains NaN or infinity.")
    if (data < 0).any():
        raise ValueError(f"The {name} layer contains a negative weight.")
    a = sparse.csr_matrix((data, a.indices, a.indptr), shape=a.shape)
    a.eliminate_zeros()
    if a.diagonal().any():
        raise ValueError(f"The {name} layer has a self loop (a non-zero diagonal entry).")
    if not use_weights:
        a.data[:] = 1.0
    w = sparse.csr_matrix(a + a.T)
    w.sum_duplicates()
    w.sort_indices()
    return w


def quantise_layers(latent: Any, spatial: Any, use_weights: bool | tuple[bool, bool] = True) -> tuple[sparse.csr_matrix, sparse.csr_matrix]:
    """The host step in front of ``sqgr_leiden_multiplex``.  Each layer is taken as a canonical CSR matrix (duplicates summed, stored
    zeros dropped), its values replaced by 1 where ``use_weights`` is false for it, and made undirected as ``W = A + A^T`` in float64 —
    an asymmetric spatial kNN graph is accepted, unlike in ``quantise_weights``.  Both layers are then quantised with ONE common scale,
    ``max(1, rint(w / w_max * 2**24))`` as int32 with ``w_max`` the largest value of the two ``W``: the layers keep their relative
    weight, so ``layer_ratio`` is the only float coefficient of the objective.  A layer may be empty.  ``ValueError`` for a matrix
    that is not square, layers of different shapes, a negative, NaN or infinite value, and a non-zero diagonal.  The caller's matrices
    are not changed."""
    use = _pair(use_weights, "use_weights", _check_bool)
    ws = [_undirected(conn, name, u) for conn, name, u in zip((latent, spatial), LAYERS, use)]
    if ws[0].shape != ws[1].shape:
        raise ValueError(f"Expected two layers over the same observations, found shapes `{ws[0].shape}` and `{ws[1].shape}`.")
    w_max = max([float(w.data.max()) for w in ws if w.nnz], default=1.0)
    out = []
    for w in ws:
        q = np.maximum(1, np.rint(w.data / w_max * float(2**LEIDEN_WEIGHT_BITS))).astype(np.int32)
        out.append(sparse.csr_matrix((q, w.indices.astype(np.int32), w.indptr.astype(np.int64)), shape=w.shape))
    return out[0], out[1]


def _layers_of(data: Any, latent_key: str, spatial_key: str) -> tuple[Any, Any, bool]:
    """(latent, spatial, is_object)."""
    if isinstance(data, (tuple, list)):
        if len(data) != 2:
            raise ValueError(f"Expected a `(latent, spatial)` pair of matrices, found {len(data)} items.")
        return data[0], data[1], False
    out = []
    for key in (latent_key, spatial_key):
        N._assert_key_in_adata(data, key, "obsp")
        conn = data.obsp[key]
        if conn.shape != (data.n_obs, data.n_obs):
            raise ValueError(f"Expected `adata.obsp[{key!r}]` of shape `{(data.n_obs, data.n_obs)}`, found `{conn.shape}`.")
        out.append(conn)
    return out[0], out[1], True


def _two_m(q: sparse.csr_matrix) -> int:
    return int(q.data.sum(dtype=np.int64)) if q.nnz < 2**31 else sum(q.data.tolist())


def _quality(layers: tuple, labels: np.ndarray, sum_in: tuple, resolutions: tuple, layer_ratio: float) -> float:
    total = Fraction(0)
    for q, s_in, gamma, a in zip(layers, sum_in, resolutions, (Fraction(1), Fraction(layer_ratio))):
        k = np.asarray(q.sum(axis=1, dtype=np.int64)).ravel()
        two_m = int(k.sum())
        if two_m == 0:
            continue
        tot = np.zeros(int(labels.max()) + 1, dtype=np.int64)
        np.add.at(tot, labels, k)
        total += a * (s_in - Fraction(gamma) * Fraction(sum(t * t for t in tot.tolist()), two_m))
    return float(total)


def _run(layers: tuple, resolutions: tuple, layer_ratio: float, n_iterations: int, device: int | None) -> MultiplexLeidenResult:
    try:
        labels, stats = _leiden_multiplex(default_context(device), *((q.indptr, q.indices, q.data) for q in layers), resolutions, layer_ratio,
                                          n_iterations)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        raise
    sum_in = (stats["sum_in_0"], stats["sum_in_1"])
    return MultiplexLeidenResult(labels, stats["n_communities"], _quality(layers, labels, sum_in, resolutions, layer_ratio), sum_in,
                                 (stats["two_m_0"], stats["two_m_1"]), stats["iterations"], stats["levels"], stats["sweeps"])


def _quantised(latent: Any, spatial: Any, use_weights: Any) -> tuple:
    layers = quantise_layers(latent, spatial, use_weights)
    if layers[0].shape[0] == 0:
        raise ValueError("Expected at least one observation.")
    for q in layers:
        _check_two_m(_two_m(q))
    return layers


def niche_spatialleiden(
    data: Any,
    resolution: float | tuple[float, float] = 1.0,
    *,
    latent_connectivities_key: str = "connectivities",
    spatial_connectivities_key: str = "spatial_connectivities",
    layer_ratio: float = 1.0,
    use_weights: bool | tuple[bool, bool] = True,
    n_iterations: int = -1,
    key_added: str = "spatialleiden",
    copy: bool = False,
    device: int | None = None,
) -> MultiplexLeidenResult | None:
    """``spatialleiden.spatialleiden(adata, resolution, directed=False, layer_ratio=..., use_weights=..., n_iterations=...)`` on the GPU
    (``csrc/sqgr_leiden_multiplex.hip``): one partition of the cells that maximises

        ``Q = sum_l a_l sum_c (in^l_c - resolution_l (tot^l_c)**2 / 2m_l)``,  ``a = (1, layer_ratio)``

    over the latent layer ``obsp[latent_connectivities_key]`` (what ``niche_neighbors`` writes) and the spatial layer
    ``obsp[spatial_connectivities_key]`` (what the graph builders write) — leidenalg's multiplex optimisation of one unnormalised
    ``RBConfigurationVertexPartition`` per layer, so a layer counts in proportion to its total weight.

    ``data`` is an AnnData-like object or a ``(latent, spatial)`` pair of matrices; ``resolution`` a number or a ``(latent, spatial)``
    pair; ``use_weights`` a bool or a pair of them.  The layers go through ``quantise_layers`` (``W = A + A^T``, one common scale).
    The algorithm is ``niche_leiden``'s deterministic synchronous Leiden with the two-layer changes ``include/sqgr.h`` states: the
    gain is ``g_latent + layer_ratio * g_spatial``, candidates and the independent set span both neighbourhoods, the community graph
    is aggregated per layer.  leidenalg is randomised and spatialleiden is not installed where this library is tested: parity with
    spatialleiden is unpinned.  Pinned are the device against a numpy restatement bit for bit, and the restatement against the
    single-layer algorithm (an empty second layer, the same graph twice), planted partitions, connectivity, node stability and the
    objective itself.  Two calls return the same bytes.

    With ``copy=True``, or for a pair of matrices, returns a ``MultiplexLeidenResult``.  Otherwise writes ``obs[key_added]`` as
    ``niche_leiden`` does and ``uns[key_added] = {"params": {"resolution", "layer_ratio", "use_weights", "n_iterations"}}``.
    ``ValueError`` / ``TypeError`` for arguments and layers ``quantise_layers`` refuses, ``NotImplementedError`` when a layer's
    quantised weights sum to 2**62 or more; every refusal is raised before the device is touched.  Under a process group every rank
    computes the whole result."""
    latent, spatial, is_object = _layers_of(data, latent_connectivities_key, spatial_connectivities_key)
    resolutions = _pair(resolution, "resolution", _check_resolution)
    layer_ratio = _check_ratio(layer_ratio)
    use = _pair(use_weights, "use_weights", _check_bool)
    n_iterations = _check_n_iterations(n_iterations)
    res = _run(_quantised(latent, spatial, use), resolutions, layer_ratio, n_iterations, device)
    if copy or not is_object:
        return res
    data.obs[key_added] = pd.Categorical(res.labels.astype(str), categories=[str(c) for c in range(res.n_communities)])
    logg.info("Adding `adata.obs[%r]`", key_added)
    _save_data(data, attr="uns", key=key_added,
               data={"params": {"resolution": resolutions, "layer_ratio": layer_ratio, "use_weights": use, "n_iterations": n_iterations}})
    return None


def calculate_niche_spatialleiden(
    data: Any,
    resolutions: float | tuple[float, float] | list[float | tuple[float, float]],
    latent_connectivities_key: str = "connectivities",
    spatial_connectivities_key: str = "spatial_connectivities",
    layer_ratio: float = 1.0,
    n_iterations: int = -1,
    use_weights: bool | tuple[bool, bool] = True,
    random_state: int = 42,
    min_niche_size: int | None = None,
    mask: pd.Series | None = None,
    prefix: str | None = None,
    library_key: str | None = None,
    inplace: bool = True,
    table_key: str | None = None,
    *,
    device: int | None = None,
) -> Any:
    """Compute niche assignments with the SpatialLeiden flavour (drop-in for ``squidpy.gr.calculate_niche_spatialleiden``,
    gr/_niche.py:466-620): ``niche_spatialleiden`` per resolution on ``obsp[latent_connectivities_key]`` and
    ``obsp[spatial_connectivities_key]``.  ``obs[f"spatialleiden_res={res}"]`` gets the labels as ``str``, one column per resolution;
    ``resolutions`` is a float, a ``(latent, spatial)`` tuple, or a list of them, and ``res`` is formatted as Python formats it.

    ``mask`` and ``min_niche_size`` follow ``_postprocess_niche_results``; ``prefix`` goes in front of the labels where there is no
    ``library_key``; with ``library_key`` every library runs on its own rows and on its own sub-blocks of both matrices (the
    reference's ``adata[lib_indices].copy()``) and its labels are prefixed ``lib={id}_``.  ``random_state`` is validated as an ``int``
    and has no effect: the algorithm is deterministic.  Parity with spatialleiden is unpinned (see ``niche_spatialleiden``).  Every
    refusal is raised before anything runs and leaves the object untouched.

    Returns ``None`` if ``inplace=True``, else a copy of ``adata`` with the columns added."""
    orig_adata = extract_adata_if_sdata(data, table_key=table_key)
    res_list = resolutions if isinstance(resolutions, list) else [resolutions]
    if not res_list:
        raise ValueError("Expected at least one resolution.")
    pairs = [_pair(r, "resolutions", _check_resolution) for r in res_list]
    layer_ratio = _check_ratio(layer_ratio)
    n_iterations = _check_n_iterations(n_iterations)
    use = _pair(use_weights, "use_weights", _check_bool)
    if isinstance(random_state, bool) or not isinstance(random_state, numbers.Integral):
        raise TypeError(f"Expected `random_state` to be of type `int`, found `{type(random_state).__name__}`.")
    if prefix is not None and not isinstance(prefix, str):
        raise TypeError(f"Expected `prefix` to be of type `str`, found `{type(prefix).__name__}`.")
    if library_key is not None:
        N._assert_key_in_adata(orig_adata, library_key, "obs")
    latent, spatial, _ = _layers_of(orig_adata, latent_connectivities_key, spatial_connectivities_key)
    whole = _quantised(latent, spatial, use)  # a sub-block of layers that pass passes too

    def cluster(adata: Any, obs: pd.DataFrame, rows: np.ndarray | None) -> list[str]:
        layers = whole
        if rows is not None:
            layers = _quantised(sparse.csr_matrix(latent)[rows][:, rows], sparse.csr_matrix(spatial)[rows][:, rows], use)
        keys = []
        for res, pair in zip(res_list, pairs):
            key = f"spatialleiden_res={res}"
            keys.append(key)
            if key in obs.columns:
                logg.info("Overwriting existing column '%s'", key)
            obs[key] = list(_run(layers, pair, layer_ratio, n_iterations, device).labels.astype(str))
        return keys

    return N.calculate_niche_custom(orig_adata, cluster, min_niche_size, mask, library_key, inplace, prefix)
