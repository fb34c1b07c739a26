"""numpy / scipy restatement of ``centrality_scores`` (gr/_nhood.py:245-345 and :432-491 of the reference), and the cases the golden
file ``tests/golden/centrality_reference.npz`` is made from (``tests/golden/make_centrality_golden.py``).

- ``build_graph``: the CSR of ``_build_graph`` — ``A + A.T``, diagonal and stored zeros removed, rows sorted.
- ``group_bfs``: level-synchronous multi-source BFS of all groups at once, 64 groups per pass, one ``uint64`` word per node:
  at level L ``new = (OR of the neighbours' words) & ~own``; ``adjacent[g]`` = new bits of g at level 1, ``dist_sum[g] += L * new
  bits of g``, ``reached[g] += new bits of g``; ``levels`` = the last level that added a bit in any pass.
- ``two_triangles``: ``two_tri[v] = sum over u in N(v) of |N(v) n N(u)|`` = row sums of ``(A @ A).multiply(A)``.
- ``scores``: the three float64 columns from those integers, by the expressions networkx and the reference's kernel use."""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

COLUMNS = ("degree_centrality", "average_clustering", "closeness_centrality")


def build_graph(conn) -> sp.csr_matrix:
    adj = sp.csr_matrix(conn)
    adj = (adj + adj.T).tocsr()
    adj.setdiag(0)
    adj.eliminate_zeros()
    adj.sort_indices()
    return adj


def _neighbour_or(indptr: np.ndarray, indices: np.ndarray, mask: np.ndarray) -> np.ndarray:
    out = np.zeros(len(mask), dtype=np.uint64)
    rows = np.flatnonzero(np.diff(indptr) > 0)  # reduceat over the non-empty rows only: an empty row has no segment
    if len(rows):
        out[rows] = np.bitwise_or.reduceat(mask[indices], indptr[:-1][rows])
    return out


def group_bfs(adj: sp.csr_matrix, codes: np.ndarray, n_cls: int, in_place: bool = False):
    """``(adjacent, dist_sum, reached, levels)``; ``in_place=True`` is the WRONG sweep (one buffer, nodes in index order), kept to
    show that a case tells the two apart."""
    n = adj.shape[0]
    indptr, indices = adj.indptr.astype(np.int64), adj.indices.astype(np.int64)
    adjacent, dist_sum, reached = (np.zeros(n_cls, dtype=np.int64) for _ in range(3))
    levels = 0
    for base in range(0, n_cls, 64):
        kp = min(64, n_cls - base)
        g = codes.astype(np.int64) - base
        member = (g >= 0) & (g < 64)
        mask = np.zeros(n, dtype=np.uint64)
        mask[member] = np.uint64(1) << g[member].astype(np.uint64)
        level = 0
        while True:
            level += 1
            if in_place:
                new = np.zeros(n, dtype=np.uint64)
                for v in range(n):
                    acc = np.bitwise_or.reduce(mask[indices[indptr[v]:indptr[v + 1]]], initial=np.uint64(0))
                    new[v] = acc & ~mask[v]
                    mask[v] |= new[v]
            else:
                new = _neighbour_or(indptr, indices, mask) & ~mask
                mask = mask | new
            if not new.any():
                break
            levels = max(levels, level)
            for b in range(kp):
                c = int(((new >> np.uint64(b)) & np.uint64(1)).sum())
                reached[base + b] += c
                dist_sum[base + b] += c * level
                if level == 1:
                    adjacent[base + b] += c
    return adjacent, dist_sum, reached, levels


def two_triangles(adj: sp.csr_matrix, chunk: int = 512) -> np.ndarray:
    """Row sums of ``(A @ A).multiply(A)`` on the 0/1 structure, in row chunks (a hub row squares to a dense block)."""
    n = adj.shape[0]
    a = sp.csr_matrix((np.ones(adj.nnz, dtype=np.int64), adj.indices, adj.indptr), shape=adj.shape)
    out = np.zeros(n, dtype=np.int64)
    for r0 in range(0, n, chunk):
        rows = a[r0:r0 + chunk]
        out[r0:r0 + chunk] = np.asarray((rows @ a).multiply(rows).sum(axis=1)).ravel()
    return out


def local_clustering(adj: sp.csr_matrix, two_tri: np.ndarray) -> np.ndarray:
    k = np.diff(adj.indptr).astype(np.int64)
    cc = np.zeros(adj.shape[0], dtype=np.float64)
    ok = k >= 2
    cc[ok] = two_tri[ok] / (k[ok] * (k[ok] - 1))
    return cc


def scores(adj: sp.csr_matrix, codes: np.ndarray, n_cls: int) -> dict[str, np.ndarray]:
    """The three columns, float64[n_cls]; an empty group and a group of all nodes score 0.0."""
    n = adj.shape[0]
    adjacent, dist_sum, _, _ = group_bfs(adj, codes, n_cls)
    cc = local_clustering(adj, two_triangles(adj))
    out = {c: np.zeros(n_cls, dtype=np.float64) for c in COLUMNS}
    for g in range(n_cls):
        idx = np.flatnonzero(codes == g)
        rest = n - len(idx)
        if len(idx) == 0 or rest == 0:
            continue
        out["degree_centrality"][g] = int(adjacent[g]) / rest
        out["closeness_centrality"][g] = rest / int(dist_sum[g]) if dist_sum[g] else 0.0
        out["average_clustering"][g] = float(cc[idx].mean())
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def path_graph(n: int, order: np.ndarray | None = None) -> sp.csr_matrix:
    """Path 0 - 1 - ... - n-1; with ``order`` position p of the path is node order[p]."""
    pos = np.arange(n) if order is None else np.asarray(order)
    r, c = pos[:-1], pos[1:]
    g = sp.csr_matrix((np.ones(2 * (n - 1), np.float32), (np.r_[r, c], np.r_[c, r])), shape=(n, n))
    g.sort_indices()
    return g


def knn_directed(xy: np.ndarray, k: int, rng: np.random.Generator, self_loops: bool = True) -> sp.csr_matrix:
    """Directed kNN graph with random float weights; every third node also stores a self loop."""
    n = len(xy)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1) if n <= 4096 else None
    if d2 is None:
        raise ValueError("brute-force kNN is for test sizes")
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    rows = np.repeat(np.arange(n), k)
    cols = idx.ravel()
    if self_loops:
        loops = np.arange(0, n, 3)
        rows, cols = np.r_[rows, loops], np.r_[cols, loops]
    g = sp.csr_matrix((rng.uniform(0.1, 2.0, len(rows)), (rows, cols)), shape=(n, n))
    g.sort_indices()
    return g


def two_component_graph(seed: int = 7) -> sp.csr_matrix:
    """70 nodes: directed kNN-4 on 40 points near the origin and 29 points far away (two components), node 69 isolated; self loops
    and random weights."""
    rng = np.random.default_rng(seed)
    xy = np.r_[rng.normal(0.0, 1.0, (40, 2)), rng.normal(1000.0, 1.0, (29, 2))]
    g = knn_directed(xy, 4, rng).tolil()
    g.resize((70, 70))
    g = g.tocsr()
    g.sort_indices()
    return g


def two_component_codes(n_cls: int, seed: int = 11) -> np.ndarray:
    """Codes in [0, n_cls) with a few NaN (-1); group 0 lives in the first component only, so the second never reaches it."""
    rng = np.random.default_rng(seed + n_cls)
    codes = rng.integers(0, n_cls, 70)
    tail = codes[40:]
    tail[tail == 0] = 1
    codes[0] = 0
    codes[rng.choice(np.arange(1, 70), 5, replace=False)] = -1
    return codes.astype(np.int32)


def cancelling_graph() -> sp.csr_matrix:
    """12 nodes on a ring with chords, stored so that ``_build_graph`` has something to remove: a diagonal, stored zeros, and pairs
    (i, j) = w, (j, i) = -w whose sum cancels — no edge in the reference's graph."""
    r = [i for i in range(12)] + [i for i in range(12)] + [0, 6, 2, 9, 3, 3, 5, 5, 7]
    c = [(i + 1) % 12 for i in range(12)] + [(i + 3) % 12 for i in range(12)] + [6, 0, 9, 2, 3, 8, 5, 11, 1]
    w = [1.0] * 12 + [0.5] * 12 + [1.5, -1.5, 0.25, -0.25, 2.0, 0.0, 1.0, 0.0, 0.0]
    g = sp.csr_matrix((np.array(w), (np.array(r), np.array(c))), shape=(12, 12))
    g.sort_indices()
    return g


def hex_subgraph(rows: int, cols: int, n: int | None = None) -> sp.csr_matrix:
    """Hex lattice in scan order (the first n nodes of it)."""
    from oracle import restate as O

    g = sp.csr_matrix(O.hex_grid_graph(rows, cols))
    if n is not None:
        g = g[:n][:, :n].tocsr()
    g.sort_indices()
    return g


def hub_graph(n_leaves: int = 4960, clique: int = 40) -> sp.csr_matrix:
    """Node 0 joined to a clique (nodes 1 .. clique) and to leaves: degree clique + n_leaves."""
    n = 1 + clique + n_leaves
    others = np.arange(1, n)
    ci, cj = np.meshgrid(np.arange(1, clique + 1), np.arange(1, clique + 1), indexing="ij")
    keep = ci != cj
    r = np.r_[np.zeros(n - 1, np.int64), others, ci[keep]]
    c = np.r_[others, np.zeros(n - 1, np.int64), cj[keep]]
    g = sp.csr_matrix((np.ones(len(r), np.float32), (r, c)), shape=(n, n))
    g.sort_indices()
    return g


def cases() -> list[dict]:
    """name, conn (as the caller stores it: directed, weighted, self loops where said), codes (-1 = NaN), n_cls."""
    out = []
    ends = np.full(300, -1, np.int32)
    ends[0], ends[299], ends[149], ends[150] = 0, 1, 2, 2
    out.append(dict(name="path300_natural", conn=path_graph(300), codes=ends, n_cls=3))
    order = np.random.default_rng(3).permutation(300)
    lab = np.full(300, -1, np.int32)
    lab[order] = ends  # the same groups at the same places of the path
    out.append(dict(name="path300_random", conn=path_graph(300, order), codes=lab, n_cls=3))
    g70 = two_component_graph()
    for k in (3, 64, 65, 130):
        out.append(dict(name=f"comp70_k{k}", conn=g70, codes=two_component_codes(k), n_cls=k))
    for name, g in (("hex40x50", hex_subgraph(40, 50)), ("hex257", hex_subgraph(20, 20, 257)), ("hex1025", hex_subgraph(35, 35, 1025))):
        rng = np.random.default_rng(len(name))
        out.append(dict(name=name, conn=g, codes=rng.integers(0, 5, g.shape[0]).astype(np.int32), n_cls=5))
    out.append(dict(name="cancel12", conn=cancelling_graph(), codes=np.array([0, 0, 1, 1, -1, 0, 1, 1, 0, 0, 1, -1], np.int32), n_cls=2))
    hub = hub_graph()
    lab = np.r_[0, np.full(40, 1), 2 + np.random.default_rng(5).integers(0, 2, hub.shape[0] - 41)].astype(np.int32)
    out.append(dict(name="hub5000", conn=hub, codes=lab, n_cls=4))
    rng = np.random.default_rng(17)
    xy = rng.uniform(0, 100, (3000, 2))
    lab = rng.integers(0, 7, 3000).astype(np.int32)
    lab[rng.choice(3000, 20, replace=False)] = -1
    out.append(dict(name="knn3000", conn=knn_directed(xy, 6, rng), codes=lab, n_cls=7))
    return out


# ------------------------------------------------------------------------- the lattice above one trip of the default grid
def lattice_graph(side: int) -> sp.csr_matrix:
    """4-neighbour ``side`` x ``side`` lattice, node ``y * side + x``."""
    idx = np.arange(side * side, dtype=np.int64).reshape(side, side)
    r = np.r_[idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    c = np.r_[idx[:, 1:].ravel(), idx[1:, :].ravel()]
    adj = sp.csr_matrix((np.ones(2 * len(r), np.float32), (np.r_[r, c], np.r_[c, r])), shape=(side * side, side * side))
    adj.sort_indices()
    return adj


def lattice_codes(side: int) -> np.ndarray:
    """Group 0 = the first column, group 1 = the far corner, everything else in no group."""
    codes = np.full((side, side), -1, np.int32)
    codes[:, 0] = 0
    codes[side - 1, side - 1] = 1
    return codes.ravel()


def lattice_closed_form(side: int) -> tuple:
    """Hop distances on the lattice are Manhattan distances.  Group 0: node (x, y) lies x hops away, x = 1 .. side - 1 in each of
    ``side`` rows.  Group 1: (side - 1 - x) + (side - 1 - y) hops; with u = side - 1 - x, v = side - 1 - y the sum of u + v over the
    square is side^2 (side - 1).  The corner node itself is a member of group 1 but lies side - 1 hops from group 0; the first column
    lies u + v = (side - 1) + v hops from group 1 and is counted there."""
    s = side
    adjacent = np.array([s, 2], np.int64)
    dist_sum = np.array([s * (s * (s - 1) // 2), s * s * (s - 1)], np.int64)
    reached = np.array([s * (s - 1), s * s - 1], np.int64)
    return adjacent, dist_sum, reached, 2 * (s - 1)
