"""Host-side model of the segment list of the permutation test's count kernel (sqgr_graph::ensure_seg) and the small graphs its tests
share.  The half list (r < c) of a structurally symmetric graph is cut by (r >> 4, c - r) into entries (r0, d, mask); entries with
at least SEG_MIN_FILL edges (and d < 2**16) are segments, every other half edge is residual."""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

SEG_MIN_FILL = 8


def half_edges(adj) -> np.ndarray:
    """(m, 2) int64: the edges r < c of ``adj``, in CSR order."""
    t = sp.triu(sp.csr_matrix(adj), 1).tocoo()
    o = np.lexsort((t.col, t.row))
    return np.stack([t.row[o], t.col[o]], axis=1).astype(np.int64)


def segment_model(adj) -> tuple[np.ndarray, np.ndarray]:
    """-> (entries (s, 3) = (r0, d, mask) ordered by (r0, d), residual half edges (m, 2))."""
    he = half_edges(adj)
    r, d = he[:, 0], he[:, 1] - he[:, 0]
    key = (r >> 4) * (1 << 32) + d
    uniq, inv = np.unique(key, return_inverse=True)
    mask = np.zeros(len(uniq), dtype=np.int64)
    np.bitwise_or.at(mask, inv, 1 << (r & 15))
    fill = np.array([bin(m).count("1") for m in mask], dtype=np.int64)
    dense = (fill >= SEG_MIN_FILL) & ((uniq & 0xFFFFFFFF) < 65536)
    entries = np.stack([(uniq >> 32) << 4, uniq & 0xFFFFFFFF, mask], axis=1)
    return entries[dense], he[~dense[inv]]


def all_entries(adj) -> np.ndarray:
    """Every entry (r0, d, mask), dense or not."""
    he = half_edges(adj)
    key = (he[:, 0] >> 4) * (1 << 32) + (he[:, 1] - he[:, 0])
    uniq, inv = np.unique(key, return_inverse=True)
    mask = np.zeros(len(uniq), dtype=np.int64)
    np.bitwise_or.at(mask, inv, 1 << (he[:, 0] & 15))
    return np.stack([(uniq >> 32) << 4, uniq & 0xFFFFFFFF, mask], axis=1)


def expand(entries: np.ndarray) -> np.ndarray:
    """The half edges (r0 + j, r0 + j + d) an entry list stands for, (m, 2)."""
    out = [(r0 + j, r0 + j + d) for r0, d, m in entries.tolist() for j in range(16) if (m >> j) & 1]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def sorted_edges(e: np.ndarray) -> np.ndarray:
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def square_grid_graph(rows: int, cols: int, diagonals: bool = False) -> sp.csr_matrix:
    """4- (or 8-) neighbour square grid in scan order."""
    idx = np.arange(rows * cols).reshape(rows, cols)
    pairs = [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]
    if diagonals:
        pairs += [(idx[:-1, :-1], idx[1:, 1:]), (idx[:-1, 1:], idx[1:, :-1])]
    a = np.concatenate([p[0].ravel() for p in pairs])
    b = np.concatenate([p[1].ravel() for p in pairs])
    n = rows * cols
    g = sp.csr_matrix((np.ones(2 * len(a), np.float32), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))
    g.sort_indices()
    return g


def with_extra_edges(adj, count: int, seed: int) -> sp.csr_matrix:
    """``adj`` plus ``count`` random symmetric edges (no self loops), binary."""
    n = adj.shape[0]
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, count), rng.integers(0, n, count)
    keep = a != b
    a, b = a[keep], b[keep]
    extra = sp.csr_matrix((np.ones(2 * len(a), np.float32), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))
    g = sp.csr_matrix(((sp.csr_matrix(adj) + extra) != 0).astype(np.float32))
    g.sort_indices()
    return g


def renumber(adj, order: np.ndarray) -> sp.csr_matrix:
    """P A P^T for order[new] = old."""
    g = sp.csr_matrix(adj)[order][:, order].tocsr()
    g.sort_indices()
    return g


def counts_reference(adj, labels: np.ndarray, k: int) -> np.ndarray:
    """np.add.at over the FULL edge list: (P, k, k) uint32 for label vectors (P, n)."""
    coo = sp.csr_matrix(adj).tocoo()
    out = np.zeros((labels.shape[0], k, k), dtype=np.uint32)
    for p, lab in enumerate(labels):
        np.add.at(out[p], (lab[coo.row], lab[coo.col]), 1)
    return out
