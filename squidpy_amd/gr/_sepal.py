"""``sepal`` with the reference's signature on the MI355X path.

Reference: squidpy src/squidpy/gr/_sepal.py — ``sepal`` :30-162, ``_diffusion_genes`` :165-205, ``_diffusion`` :208-254,
``_entropy`` :290-305, ``_compute_idxs`` :308-322 (``_get_sat_unsat_idx`` :325-333, ``_get_nhood_idx`` :336-363); the expression
extraction of gr/_utils.py:89-125 (``_extract_expression``).
The host builds the lattice (O(nnz), plus an exact L1 search for the few unsaturated spots without a saturated neighbour); the
diffusion of every gene runs in ``libsqgr.so`` (``sqgr_sepal_run``)."""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np
import pandas as pd
from scipy import sparse

from .. import _dist
from .._constants import Key
from .._lib import DeviceMatrix, SepalPlan, default_context
from .._utils import (
    _assert_connectivity_key,
    _assert_spatial_basis,
    _save_data,
    deprecated_params,
    extract_adata_if_sdata,
    logg,
)

__all__ = ["sepal"]


def _non_empty_sequence(seq: Any, *, name: str) -> list[Any]:
    """_validators.py:46-58 (``assert_non_empty_sequence``): a scalar or string becomes a list of one; duplicates go, order stays."""
    if isinstance(seq, str) or not hasattr(seq, "__iter__"):
        seq = (seq,)
    res = list(dict.fromkeys(seq))
    if len(res) == 0:
        raise ValueError(f"No {name} have been selected.")
    return res


def _l1_argmin(a: np.ndarray, b: np.ndarray, chunk_elems: int = 1 << 24) -> np.ndarray:
    """``np.argmin(pairwise_distances(a, b, metric="l1"), axis=1)``: exact float64 L1 distances (summed over the coordinates in
    order, like scipy's cityblock), brute force in chunks of rows; ties go to the lowest column."""
    out = np.empty(len(a), dtype=np.int64)
    step = max(1, chunk_elems // max(len(b), 1))
    for r0 in range(0, len(a), step):
        blk = a[r0 : r0 + step]
        d = np.abs(blk[:, None, 0] - b[None, :, 0])
        for k in range(1, a.shape[1]):
            d += np.abs(blk[:, None, k] - b[None, :, k])
        out[r0 : r0 + step] = np.argmin(d, axis=1)
    return out


def sepal_lattice(g: sparse.csr_matrix, spatial: np.ndarray, max_neighs: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``_compute_idxs(g, spatial, max_neighs, "l1")`` (gr/_sepal.py:308-363): ``(sat, sat_idx, unsat, nearest)`` with ``sat_idx`` the
    saturated rows' indices in their stored order and ``nearest[q]`` the spot (not the position) of unsat[q]'s nearest saturated spot —
    its first stored saturated neighbour, else the saturated spot at the smallest L1 distance (ties: the lowest position in ``sat``).
    Unlike the reference, a lattice whose unsaturated spots all have a saturated neighbour is no error (the reference's distance query
    on zero rows fails in sklearn)."""
    indptr, indices = g.indptr.astype(np.int64), g.indices.astype(np.int64)
    deg = np.diff(indptr)
    sat = np.flatnonzero(deg == max_neighs)
    unsat = np.flatnonzero(deg < max_neighs)
    sat_idx = indices[indptr[sat][:, None] + np.arange(max_neighs)[None, :]].astype(np.int32) if len(sat) else np.zeros((0, max_neighs), np.int32)
    is_sat = deg == max_neighs
    nearest = np.full(len(unsat), -1, dtype=np.int64)
    lens = deg[unsat]
    if lens.sum():
        row = np.repeat(np.arange(len(unsat)), lens)
        pos = np.repeat(indptr[unsat], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
        nb = indices[pos]
        hit = np.flatnonzero(is_sat[nb])  # ascending: the rows' entries are contiguous and in stored order
        rows_hit, first = np.unique(row[hit], return_index=True)
        nearest[rows_hit] = nb[hit[first]]
    rest = np.flatnonzero(nearest < 0)
    if len(rest):
        nearest[rest] = sat[_l1_argmin(spatial[unsat[rest]], spatial[sat])]
    return sat.astype(np.int32), sat_idx, unsat.astype(np.int32), nearest.astype(np.int32)


def _expression(adata: Any, genes: list[Any], use_raw: bool, layer: str | None) -> tuple[Any, np.ndarray, list[Any]]:
    """gr/_utils.py:89-125 (``_extract_expression``): the matrix the genes are columns of, their column indices, and the genes."""
    if use_raw and getattr(adata, "raw", None) is None:
        logg.warning("AnnData object has no attribute `raw`. Setting `use_raw=False`")
        use_raw = False
    if use_raw:
        genes = _non_empty_sequence(list(set(adata.raw.var_names) & set(genes)), name="genes")
        base, names = adata.raw.X, adata.raw.var_names
    else:
        genes = _non_empty_sequence(genes, name="genes")
        if layer is None:
            base = adata.X
        elif layer not in adata.layers:
            raise KeyError(f"Layer `{layer}` not found in `adata.layers`.")
        else:
            base = adata.layers[layer]
        names = adata.var_names
    cols = pd.Index(names).get_indexer(pd.Index(genes))
    if (cols < 0).any():
        missing = [gn for gn, c in zip(genes, cols) if c < 0]
        raise KeyError(f"Values {missing} not found in `var_names`.")
    return base, cols.astype(np.int32), genes


@deprecated_params({"backend": "1.10.0"})
def sepal(
    adata: Any,
    max_neighs: int,
    genes: str | Sequence[str] | None = None,
    n_iter: int | None = 30000,
    dt: float = 0.001,
    thresh: float = 1e-8,
    connectivity_key: str = Key.obsp.spatial_conn(),
    spatial_key: str = Key.obsm.spatial,
    layer: str | None = None,
    use_raw: bool = False,
    copy: bool = False,
    n_jobs: int | None = None,
    show_progress_bar: bool = True,
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> pd.DataFrame | None:
    """Identify spatially variable genes with *Sepal* (drop-in for ``squidpy.gr.sepal``, gr/_sepal.py:30-162).

    Same parameters, checks, gene selection (HVG default, ``genes``, ``layer``, ``use_raw``), scores (``dt * i`` for the first sweep
    ``i`` whose entropy change is at most ``thresh``, NaN when none within ``n_iter``), sort order and ``adata.uns['sepal_score']``
    slot as the reference.  The diffusion of every gene runs on the GPU; its concentrations follow the reference's bit for bit.
    ``n_jobs`` and ``show_progress_bar`` are accepted and have no effect.  Extra keyword-only parameter: ``device``.
    With a process group the genes are split across ranks and the stop sweeps all-reduced: every rank returns the same frame.

    Differences: the caller's graph is not changed (the reference's ``eliminate_zeros()`` works in place on a CSR
    input); a lattice where every unsaturated spot has a saturated neighbour is scored (sklearn raises on the reference's empty
    distance query)."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    _assert_connectivity_key(adata, connectivity_key)
    _assert_spatial_basis(adata, key=spatial_key)
    if max_neighs not in (4, 6):
        raise ValueError(f"Expected `max_neighs` to be either `4` or `6`, found `{max_neighs}`.")

    spatial = np.asarray(adata.obsm[spatial_key]).astype(np.float64)

    if genes is None:
        genes = np.asarray(adata.var_names.values)
        if "highly_variable" in adata.var.columns:
            genes = genes[np.asarray(adata.var["highly_variable"].values)]
    genes = _non_empty_sequence(genes, name="genes")

    g = adata.obsp[connectivity_key]
    g = g.copy() if sparse.isspmatrix_csr(g) else sparse.csr_matrix(g)
    g.eliminate_zeros()

    max_n = np.diff(g.indptr).max()
    if max_n != max_neighs:
        raise ValueError(f"Expected `max_neighs={max_neighs}`, found node with `{max_n}` neighbors.")

    sat, sat_idx, unsat, nearest = sepal_lattice(g, spatial, max_neighs)
    base, cols, genes = _expression(adata, genes, use_raw, layer)

    position = np.empty(g.shape[0], dtype=np.int64)
    position[sat] = np.arange(len(sat))
    rank, world = _dist.world()
    lo, hi = _dist.shard_range(len(cols), rank, world)
    enc = np.zeros(len(cols), dtype=np.int64)  # stop sweep + 1, 0 = none (and 0 for the other ranks' genes)
    if hi > lo:
        ctx = default_context(device)
        plan = SepalPlan(ctx, g.shape[0], max_neighs, sat, sat_idx, unsat, position[nearest] if len(unsat) else np.zeros(0, np.int32))
        matrix = DeviceMatrix(ctx, base)
        try:
            enc[lo:hi] = plan.run(matrix, cols[lo:hi], int(n_iter), float(dt), float(thresh)).astype(np.int64) + 1
        finally:
            matrix.close()
            plan.close()
    (enc,) = _dist.allreduce_sum_([enc])
    it = enc - 1
    score = np.where(it >= 0, dt * it.astype(np.float64), np.nan)  # dt * float(i), gr/_sepal.py:200

    key_added = "sepal_score"
    sepal_score = pd.DataFrame(score, index=genes, columns=[key_added])

    if sepal_score[key_added].isna().any():
        logg.warning("Found `NaN` in sepal scores, consider increasing `n_iter` to a higher value")
    sepal_score = sepal_score.sort_values(by=key_added, ascending=False)

    if copy:
        return sepal_score

    _save_data(adata, attr="uns", key=key_added, data=sepal_score)
    return None
