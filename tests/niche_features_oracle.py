"""TEST INFRASTRUCTURE — a numpy / scipy restatement of ``csrc/sqgr_niche.hip`` in the kernels' documented order: every sum over a
row's stored entries runs in ascending column order, products and sums are rounded separately (numpy never fuses two array
operations), variance is ``m2 - m1 * m1``.  tests/test_niche_features_cpu.py pins it to the reference's literal code
(tests/golden/niche_features_reference.npz); the GPU must reproduce it bit for bit.

Also the rounding bounds between two evaluation orders that the tests derive from their inputs (``U`` = 2^-53)."""

from __future__ import annotations

import numpy as np
from scipy import sparse

U = 2.0**-53
COUNT_LIMIT = 1 << 24


def canonical(a: sparse.spmatrix) -> sparse.csr_matrix:
    a = sparse.csr_matrix(a).copy()
    a.sum_duplicates()
    return a


def ordered_spmm(indptr: np.ndarray, indices: np.ndarray, coef: np.ndarray, dense: np.ndarray) -> np.ndarray:
    """``out[i] = sum over the entries e of row i, in storage order, of coef[e] * dense[indices[e]]``: round t adds the t-th entry of
    every row that has one, so every row's sum runs entry by entry with its own rounding per product and per sum."""
    n = len(indptr) - 1
    out = np.zeros((n, dense.shape[1]), dtype=np.float64)
    lens = np.diff(indptr)
    for t in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > t)
        e = indptr[rows] + t
        out[rows] = out[rows] + coef[e][:, None] * dense[indices[e]]
    return out


# ---- CellCharter shells -------------------------------------------------------------------------------------------------------------
def shells(a: sparse.spmatrix, distance: int, limit: int = COUNT_LIMIT) -> list[tuple[sparse.csr_matrix, sparse.csr_matrix]]:
    """``[(hop_k, vis_k)]`` for k = 1 .. distance in exact integers: ``hop_k`` of ones, ``vis_k`` of visit counts, both sorted CSR
    (int32 values).  Raises ``OverflowError`` when a path count reaches ``limit``."""
    a = canonical(a)
    n = a.shape[0]
    ones = sparse.csr_matrix((np.ones(a.nnz, dtype=np.int64), a.indices, a.indptr), shape=a.shape)
    eye = sparse.identity(n, dtype=np.int64, format="csr")
    hop = (ones - ones.multiply(eye)).tocsr()
    hop.eliminate_zeros()
    vis = (ones - ones.multiply(eye) + eye).tocsr()
    out = []
    for k in range(1, distance + 1):
        if k > 1:
            paths = (hop @ ones).tocsr()
            if paths.nnz and paths.data.max() >= limit:
                raise OverflowError(f"a path count of shell {k} reaches {limit}")
            diff = (paths - vis.multiply(paths > 0)).tocsr()  # on the columns the expansion reached: paths - visits
            hop = (diff > 0).astype(np.int64).tocsr()
            hop.eliminate_zeros()
            vis = (vis + hop).tocsr()
        for m in (hop, vis):
            m.sum_duplicates()
            m.sort_indices()
        out.append((hop.astype(np.int32), vis.astype(np.int32)))
    return out


def shell_block(hop: sparse.csr_matrix, x: np.ndarray, aggregation: str) -> np.ndarray:
    lens = np.diff(hop.indptr).astype(np.float64)
    with np.errstate(divide="ignore"):
        dinv = np.where(lens > 0, 1.0 / lens, 0.0)
    coef = np.repeat(dinv, np.diff(hop.indptr))
    m1 = ordered_spmm(hop.indptr, hop.indices, coef, x)
    if aggregation == "mean":
        return m1
    m2 = ordered_spmm(hop.indptr, hop.indices, coef, x * x)
    return m2 - m1 * m1


def dense64(x) -> np.ndarray:
    return np.ascontiguousarray(x.toarray() if sparse.issparse(x) else x, dtype=np.float64)


def cellcharter(a: sparse.spmatrix, x, distance: int, aggregation: str) -> np.ndarray:
    x = dense64(x)
    return np.ascontiguousarray(np.hstack([x] + [shell_block(hop, x, aggregation) for hop, _ in shells(a, distance)]))


# ---- UTAG ---------------------------------------------------------------------------------------------------------------------------
def utag_coefficients(a: sparse.csr_matrix) -> np.ndarray:
    """``a_ij / (L1 norm of row i)``, the norm summed in ascending column order; a row of norm 0 keeps its entries."""
    norm = ordered_spmm(a.indptr, a.indices, np.abs(a.data.astype(np.float64)), np.ones((a.shape[1], 1)))[:, 0]
    per_entry = np.repeat(norm, np.diff(a.indptr))
    return np.where(per_entry != 0.0, a.data.astype(np.float64) / np.where(per_entry != 0.0, per_entry, 1.0), a.data.astype(np.float64))


def utag(a: sparse.spmatrix, x) -> np.ndarray:
    a = canonical(a)
    return ordered_spmm(a.indptr, a.indices, utag_coefficients(a), dense64(x))


# ---- neighbourhood profile ----------------------------------------------------------------------------------------------------------
def label_hops(a: sparse.spmatrix, codes: np.ndarray, n_categories: int, distance: int, normalise: bool) -> np.ndarray:
    a = canonical(a)
    w = a.data.astype(np.float64)
    panel = (np.asarray(codes)[:, None] == np.arange(n_categories)[None, :]).astype(np.float64)
    hops = []
    for _ in range(distance):
        panel = ordered_spmm(a.indptr, a.indices, w, panel)
        hops.append(panel)
    hops = np.stack(hops)
    if normalise:
        total = np.zeros(hops.shape[:2])
        for c in range(n_categories):
            total = total + hops[:, :, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            hops = hops / total[:, :, None]
        hops[np.isnan(hops)] = 0.0
    return hops


def hop_weights(n_hop_weights, distance: int):
    if n_hop_weights is None:
        return [1.0] * distance
    if len(n_hop_weights) < distance:
        return n_hop_weights + [n_hop_weights[-1]] * (distance - len(n_hop_weights))
    return n_hop_weights


def nhood_profile(a, codes, n_categories: int, distance: int, abs_nhood: bool, n_hop_weights) -> np.ndarray:
    hops = label_hops(a, codes, n_categories, distance, not abs_nhood)
    if distance == 1:
        return hops[0]
    weights = hop_weights(n_hop_weights, distance)
    profile = weights[0] * hops[0]
    for h in range(1, distance):
        profile += weights[h] * hops[h]
    return profile if abs_nhood else profile / sum(weights)


# ---- bounds between two evaluation orders -------------------------------------------------------------------------------------------
def sum_bound(indptr: np.ndarray, indices: np.ndarray, coef: np.ndarray, dense: np.ndarray) -> np.ndarray:
    """Two roundings-to-nearest evaluations of ``sum_e coef_e * x_e`` over the same m rounded products, summed in two different orders,
    differ by at most ``2 (m - 1) U sum |coef_e x_e|`` per element (each order is within ``(m - 1) U sum |.|`` of the exact sum of the
    rounded products, to first order; the factor's slack covers the second order for the m used here)."""
    m = np.diff(indptr)
    mass = ordered_spmm(indptr, indices, np.abs(coef), np.abs(dense))
    return 2.0 * np.maximum(m - 1, 0)[:, None] * U * mass


def variance_bound(indptr, indices, coef, x: np.ndarray, m1: np.ndarray, m2: np.ndarray) -> np.ndarray:
    """``m2 - m1 * m1`` evaluated twice on sums that differ by at most b1 = sum_bound(x) and b2 = sum_bound(x * x): the squares differ by
    at most (2 |m1| + b1) b1, and each side rounds its square and its difference once: U (|m1| + b1)^2 and U (|m2| + b2 + (|m1| + b1)^2)
    per side."""
    b1 = sum_bound(indptr, indices, coef, x)
    b2 = sum_bound(indptr, indices, coef, x * x)
    sq = (np.abs(m1) + b1) ** 2
    return b2 + (2.0 * np.abs(m1) + b1) * b1 + 2.0 * U * sq + 2.0 * U * (np.abs(m2) + b2 + sq)


def shell_bound(hop: sparse.csr_matrix, x: np.ndarray, aggregation: str) -> np.ndarray:
    """The bound of one shell block of the CellCharter features between this order and another."""
    lens = np.diff(hop.indptr).astype(np.float64)
    coef = np.repeat(np.where(lens > 0, 1.0 / np.where(lens > 0, lens, 1.0), 0.0), np.diff(hop.indptr))
    if aggregation == "mean":
        return sum_bound(hop.indptr, hop.indices, coef, x)
    m1 = ordered_spmm(hop.indptr, hop.indices, coef, x)
    m2 = ordered_spmm(hop.indptr, hop.indices, coef, x * x)
    return variance_bound(hop.indptr, hop.indices, coef, x, m1, m2)


def profile_relative_bound(a: sparse.csr_matrix, distance: int, abs_nhood: bool, n_categories: int) -> float:
    """Relative bound between two evaluations of a neighbourhood profile on NON-NEGATIVE weights (every sum is then a sum of
    non-negative terms and rounding errors are relative).  Multi-hop: 4 distance (max row nnz of A^distance + 1) U.  It covers both
    evaluations: with m = max row nnz of A and M = max row nnz of A^distance, the kernels nest `distance` sums of at most m products,
    (m + 1) U each; the reference forms A^distance in distance - 1 such levels and then sums up to M entries, M U; a proportion divides
    two such values, (K - 1) U more for the row total, and the hop combination adds distance + 2 roundings:
    (4 distance - 2)(m + 1) + 2 M + K + distance + 2 <= 4 distance (M + 1), asserted here for the graph at hand.  A single hop has no
    power: 2 m U per raw sum, (4 m + K + 2) U per proportion."""
    assert (a.data >= 0).all()
    m = int(np.diff(a.indptr).max())
    if distance == 1:
        return (2 * m if abs_nhood else 4 * m + n_categories + 2) * U
    big = max_row_nnz_of_power(a, distance)
    assert (4 * distance - 2) * (m + 1) + 2 * big + n_categories + distance + 2 <= 4 * distance * (big + 1)
    return 4 * distance * (big + 1) * U


def max_row_nnz_of_power(a: sparse.spmatrix, distance: int) -> int:
    s = sparse.csr_matrix((np.ones(a.nnz, dtype=np.int64), a.indices, a.indptr), shape=a.shape)
    p = s.copy()
    for _ in range(distance - 1):
        p = (p @ s).tocsr()
    return int(np.diff(p.indptr).max())
