"""A numpy restatement of ``sq.gr.sepal``'s lattice and diffusion (gr/_sepal.py:208-363), written for the tests: the lattice of
``_compute_idxs``, one Jacobi sweep of ``_diffusion`` with the same float64 operations in the same order, the stop test, and the
whole trajectory when asked.  tests/test_sepal_cpu.py pins it to the reference's literal source through the committed goldens."""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

EPS = np.finfo(np.float64).eps


def compute_idxs(g: sp.csr_matrix, spatial: np.ndarray, max_neighs: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(sat, sat_idx, unsat, nearest spot) with a loop per spot: the first stored saturated neighbour, else the saturated spot at
    the smallest L1 distance (first one on ties)."""
    indptr, indices = g.indptr, g.indices
    deg = np.diff(indptr)
    sat = np.flatnonzero(deg == max_neighs)
    unsat = np.flatnonzero(deg < max_neighs)
    sat_set = set(sat.tolist())
    sat_idx = np.array([indices[indptr[i] : indptr[i + 1]] for i in sat], dtype=np.int32).reshape(len(sat), max_neighs)
    nearest = []
    for i in unsat:
        u = next((int(v) for v in indices[indptr[i] : indptr[i + 1]] if int(v) in sat_set), -1)
        if u < 0:
            d = np.abs(spatial[sat, 0] - spatial[i, 0])
            for k in range(1, spatial.shape[1]):
                d = d + np.abs(spatial[sat, k] - spatial[i, k])
            u = int(sat[np.argmin(d)])
        nearest.append(u)
    return sat.astype(np.int32), sat_idx, unsat.astype(np.int32), np.array(nearest, dtype=np.int32)


def fallback_rows(g: sp.csr_matrix, max_neighs: int) -> np.ndarray:
    """The unsaturated spots with no saturated neighbour: the rows of the reference's L1 distance query (gr/_sepal.py:316)."""
    deg = np.diff(g.indptr)
    sat = deg == max_neighs
    return np.array([i for i in np.flatnonzero(deg < max_neighs) if not sat[g.indices[g.indptr[i] : g.indptr[i + 1]]].any()], dtype=np.int64)


def drop_spots(xy: np.ndarray, g: sp.csr_matrix, spots) -> tuple[np.ndarray, sp.csr_matrix]:
    """The lattice without `spots` (coordinates and graph, rows and columns renumbered in order)."""
    keep = np.setdiff1d(np.arange(g.shape[0]), np.asarray(spots, dtype=np.int64))
    h = g[keep][:, keep].tocsr()
    h.sort_indices()
    return xy[keep], h


def sweep(conc: np.ndarray, use_hex: bool, lattice: tuple, dt: float) -> np.ndarray:
    sat, sat_idx, unsat, nearest = lattice
    nb = conc[sat_idx]
    nhood = nb[:, 0].copy()
    for k in range(1, nb.shape[1]):
        nhood = nhood + nb[:, k]  # left to right, like np.sum of fewer than 8 elements
    c = conc[sat]
    d2 = (2.0 * nhood - 12.0 * c) / 3.0 if use_hex else nhood - 4.0 * c
    dcdt = np.zeros(len(conc))
    dcdt[sat] = d2
    out = conc.copy()
    out[sat] = c + d2 * dt
    out[unsat] = conc[unsat] + dcdt[nearest] * dt
    out[out < 0] = 0
    return out


def entropy(x: np.ndarray) -> float:
    xnz = x[x > 0]
    xs = np.sum(xnz)
    if xs < EPS:
        return 0.0
    xn = xnz / xs
    return float((-np.log(np.maximum(xn, EPS)) * xn).sum())


def diffusion(conc: np.ndarray, use_hex: bool, n_iter: int, lattice: tuple, dt: float, thresh: float | None,
              keep: tuple[int, ...] = ()) -> tuple[int, np.ndarray, np.ndarray, dict[int, np.ndarray]]:
    """(stop sweep or -1, delta[i], ent[i] of the sweeps run, {k: vector after k sweeps for k in keep}).  thresh=None: no stop test."""
    conc = np.array(conc, dtype=np.float64)
    n_sat = len(lattice[0])
    prev = 1.0
    deltas, ents, kept = [], [], {}
    if 0 in keep:
        kept[0] = conc.copy()
    for i in range(n_iter):
        conc = sweep(conc, use_hex, lattice, dt)
        ent = entropy(conc[lattice[0]]) / n_sat
        deltas.append(abs(ent - prev))
        ents.append(ent)
        prev = ent
        if i + 1 in keep:
            kept[i + 1] = conc.copy()
        if thresh is not None and deltas[-1] <= thresh:
            return i, np.array(deltas), np.array(ents), kept
    return -1, np.array(deltas), np.array(ents), kept


def band(deltas: np.ndarray, thresh: float, delta: float = 1e-15) -> tuple[int, int]:
    """(i_lo, i_hi): the first sweep with delta <= thresh + delta and the first with delta <= thresh - delta (-1: none)."""
    lo = np.flatnonzero(deltas <= thresh + delta)
    hi = np.flatnonzero(deltas <= thresh - delta)
    return (int(lo[0]) if len(lo) else -1), (int(hi[0]) if len(hi) else -1)


# ---- grids and genes of the tests
def hex_grid(rows: int, cols: int) -> tuple[np.ndarray, sp.csr_matrix]:
    """Hex lattice coordinates and its 6-neighbour CSR graph (sorted rows)."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    r, c = r.ravel(), c.ravel()
    xy = np.stack([(c + 0.5 * (r % 2)) * 100.0, r * (np.sqrt(3.0) / 2.0) * 100.0], axis=1)
    odd = r % 2
    rows_, cols_ = [], []
    for dr, dc in ((0, -1), (0, 1), (-1, -1), (-1, 0), (1, -1), (1, 0)):
        rr, cc = r + dr, c + dc + (odd if dr else 0)
        ok = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        rows_.append((r * cols + c)[ok])
        cols_.append((rr * cols + cc)[ok])
    i, j = np.concatenate(rows_), np.concatenate(cols_)
    g = sp.csr_matrix((np.ones(len(i), np.float32), (i, j)), shape=(rows * cols, rows * cols))
    g.sort_indices()
    return xy, g


def square_grid(rows: int, cols: int) -> tuple[np.ndarray, sp.csr_matrix]:
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    xy = np.stack([c.ravel(), r.ravel()], axis=1).astype(np.float64)
    return xy, radius_graph(xy, 1.0)


def radius_graph(xy: np.ndarray, radius: float) -> sp.csr_matrix:
    from sklearn.neighbors import NearestNeighbors

    g = NearestNeighbors(radius=radius).fit(xy).radius_neighbors_graph(xy, mode="connectivity").tocsr()
    g.setdiag(0)
    g.eliminate_zeros()
    g.sort_indices()
    return g.astype(np.float32)


def shuffle_rows(g: sp.csr_matrix, seed: int) -> sp.csr_matrix:
    """The same graph with every row's entries stored in a random order."""
    rng = np.random.default_rng(seed)
    g = g.copy()
    for i in range(g.shape[0]):
        a, b = g.indptr[i], g.indptr[i + 1]
        p = rng.permutation(b - a)
        g.indices[a:b] = g.indices[a:b][p]
        g.data[a:b] = g.data[a:b][p]
    g.has_sorted_indices = False
    return g


def mixed_genes(xy: np.ndarray, n_genes: int, seed: int) -> np.ndarray:
    """(n, n_genes) float64 of seeded mixed structure: noise, stripes and blobs of several widths."""
    rng = np.random.default_rng(seed)
    x = (xy[:, 0] - xy[:, 0].min()) / max(np.ptp(xy[:, 0]), 1e-12)
    y = (xy[:, 1] - xy[:, 1].min()) / max(np.ptp(xy[:, 1]), 1e-12)
    out = np.empty((len(xy), n_genes))
    for k in range(n_genes):
        kind = k % 3
        if kind == 0:
            v = rng.gamma(2.0, 1.0, len(xy))
        elif kind == 1:
            f = rng.uniform(1.0, 6.0)
            v = 1.0 + np.sin(2 * np.pi * f * (x if k % 2 else y) + rng.uniform(0, 6.28))
        else:
            cx, cy, w = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.05, 0.3)
            v = 5.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * w * w)) + 0.1 * rng.random(len(xy))
        out[:, k] = v
    return out


def spot_scale_genes(xy: np.ndarray, n_genes: int, seed: int) -> np.ndarray:
    """(n, n_genes) float64: noise, stripes of period 4-40 spot spacings and blobs 1.5-12 spacings wide, in turn — structure at the
    scale of spots, whatever the size of the grid (a structure as wide as the grid changes the entropy too little per sweep: such a
    gene stops after its second sweep)."""
    rng = np.random.default_rng(seed)
    d = np.sort(np.abs(xy[1:, 0] - xy[:-1, 0]))
    h = d[d > 0][0]  # spot spacing
    out = np.empty((len(xy), n_genes))
    for k in range(n_genes):
        kind = k % 3
        if kind == 0:
            out[:, k] = rng.gamma(2.0, 1.0, len(xy))
        elif kind == 1:
            ang, per = rng.uniform(0, np.pi), rng.uniform(4, 40) * h
            out[:, k] = 1.0 + np.sin(2 * np.pi * (xy[:, 0] * np.cos(ang) + xy[:, 1] * np.sin(ang)) / per)
        else:
            c, w = xy[rng.integers(len(xy))], rng.uniform(1.5, 12) * h
            out[:, k] = 5.0 * np.exp(-((xy - c) ** 2).sum(1) / (2 * w * w)) + 0.1 * rng.random(len(xy))
    return out
