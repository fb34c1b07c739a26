"""Cases shared by tests/test_niche_leiden_cpu.py and tests/test_niche_leiden_gpu.py, built with numpy and scipy only.

Every case is a symmetric float64 scipy CSR matrix in canonical form without a diagonal; ``graph(name)`` returns what ``sqgr_leiden``
takes, ``(indptr int64, indices int32, weights int32)``, quantised by the oracle's restatement of the host step.

- Planted partitions whose optimum is unique at resolution 0.25, 0.5, 1 and 2: a ring of 8 cliques of 6; disjoint cliques of 7, 5, 5,
  3, 1, 1 (empty rows, equal sizes, components); 4 groups of two 6-cliques joined by 12 edges, one edge between consecutive groups.
- A 12 x 12 lattice of unit weights: ties everywhere.
- A star of 5 000 leaves whose hub is also in a 40-clique: a row beyond the on-chip capacity.
- Two hubs with exactly ``capacity`` and ``capacity + 1`` neighbours, each neighbour in a community of its own.
- Three kNN-15 fuzzy graphs (UMAP's weights from the host restatement of ``niche_neighbors``): eight separated blobs, six
  overlapping blobs, no structure.
- Weights spanning more than 2**24 (the clamp to 1), and the tiny inputs n = 1, n = 2 with one edge, n = 5 without edges."""

from __future__ import annotations

import functools

import numpy as np
from scipy import sparse
from scipy.spatial import cKDTree

from tests import niche_leiden_oracle as LO
from tests import niche_neighbors_oracle as NO

PLANTED_RESOLUTIONS = (0.25, 0.5, 1.0, 2.0)
RESOLUTIONS = (0.5, 1.0, 2.0)
CAPACITY_FALLBACK = 128  # LD_CAP of csrc/sqgr_leiden.hip, for generating the cases without the library


def capacity() -> int:
    try:
        from squidpy_amd import _lib

        return _lib.leiden_info()["capacity"]
    except OSError:
        return CAPACITY_FALLBACK


def _sym(n: int, r: list, c: list, w: list | None = None) -> sparse.csr_matrix:
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    w = np.ones(r.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    a = sparse.coo_matrix((np.r_[w, w], (np.r_[r, c], np.r_[c, r])), shape=(n, n)).tocsr()
    a.sort_indices()
    assert a.has_canonical_format and a.diagonal().sum() == 0 and a.nnz == 2 * r.shape[0], "an edge was listed twice"
    return a


def _clique(nodes: list) -> tuple[list, list]:
    r = [a for i, a in enumerate(nodes) for b in nodes[i + 1:]]
    c = [b for i, a in enumerate(nodes) for b in nodes[i + 1:]]
    return r, c


def _ring_of_cliques(weights: tuple[float, float] = (1.0, 1.0)) -> tuple[sparse.csr_matrix, np.ndarray]:
    r, c, w = [], [], []
    for q in range(8):
        cr, cc = _clique(list(range(6 * q, 6 * q + 6)))
        r += cr
        c += cc
        w += [weights[0]] * len(cr)
        r.append(6 * q + 5)
        c.append(6 * ((q + 1) % 8))
        w.append(weights[1])
    return _sym(48, r, c, w), np.repeat(np.arange(8), 6)


def big_ring_graph(q: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``_ring_of_cliques`` with ``q`` cliques and unit weights, built without a Python loop over the cliques, as ``graph`` returns it."""
    i, j = np.triu_indices(6, 1)
    base = 6 * np.arange(q, dtype=np.int64)[:, None]
    r = np.r_[(base + i[None, :]).ravel(), base.ravel() + 5]
    c = np.r_[(base + j[None, :]).ravel(), 6 * ((np.arange(q, dtype=np.int64) + 1) % q)]
    a = _sym(6 * q, r, c)
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), LO.quantise(a)


def _disjoint_cliques() -> tuple[sparse.csr_matrix, np.ndarray]:
    r, c, start, planted = [], [], 0, []
    for q, size in enumerate((7, 5, 5, 3, 1, 1)):
        cr, cc = _clique(list(range(start, start + size)))
        r += cr
        c += cc
        planted += [q] * size
        start += size
    return _sym(start, r, c), np.asarray(planted)


def _two_level() -> tuple[sparse.csr_matrix, np.ndarray]:
    r, c = [], []
    for g in range(4):
        a, b = list(range(12 * g, 12 * g + 6)), list(range(12 * g + 6, 12 * g + 12))
        for nodes in (a, b):
            cr, cc = _clique(nodes)
            r += cr
            c += cc
        for i in range(6):  # 12 cross edges
            r += [a[i], a[i]]
            c += [b[i], b[(i + 1) % 6]]
        r.append(12 * g + 11)
        c.append(12 * ((g + 1) % 4))
    return _sym(48, r, c), np.repeat(np.arange(4), 12)


def _lattice(side: int = 12) -> sparse.csr_matrix:
    idx = np.arange(side * side).reshape(side, side)
    r = np.r_[idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    c = np.r_[idx[:, 1:].ravel(), idx[1:, :].ravel()]
    return _sym(side * side, r.tolist(), c.tolist())


def _star() -> sparse.csr_matrix:
    leaves, clique = 5000, 40
    r, c = [0] * leaves, list(range(1, leaves + 1))
    cr, cc = _clique([0] + list(range(leaves + 1, leaves + clique)))
    return _sym(leaves + clique, r + cr, c + cc)


def _capacity_rows() -> sparse.csr_matrix:
    """Hub 0 has ``capacity`` neighbours and hub 1 ``capacity + 1``; every neighbour has a partner of its own, so it sits in a community
    of its own at every sweep: the hubs' rows hold exactly that many distinct neighbour communities."""
    cap = capacity()
    r, c, nxt = [], [], 2
    for hub, deg in ((0, cap), (1, cap + 1)):
        for _ in range(deg):
            r += [hub, nxt, nxt]
            c += [nxt, nxt + 1, nxt + 2]
            r.append(nxt + 1)
            c.append(nxt + 2)
            nxt += 3
    return _sym(nxt, r, c)


def _blobs(n: int, d: int, centres: int, spread: float, seed: int) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(seed)
    member = rng.integers(0, centres, size=n) if centres else np.zeros(n, dtype=np.int64)
    mu = rng.normal(size=(max(centres, 1), d)) * spread
    return mu[member] + rng.normal(size=(n, d)), member


@functools.lru_cache(maxsize=None)
def points(name: str) -> tuple[np.ndarray, np.ndarray]:
    return {"knn_blobs8": lambda: _blobs(2000, 10, 8, 12.0, 21), "knn_blobs6": lambda: _blobs(3000, 5, 6, 1.5, 22),
            "knn_flat": lambda: _blobs(2000, 8, 0, 0.0, 23)}[name]()


def _knn_graph(name: str) -> sparse.csr_matrix:
    x, _ = points(name)
    dist, idx = cKDTree(x).query(x, k=15)
    dist, idx = dist[:, 1:], idx[:, 1:].astype(np.int32)
    vals = NO.fuzzy(dist, float(dist.sum() / (x.shape[0] * 15))).vals
    conn = NO.connectivities(idx, vals).tocsr()
    conn.setdiag(0)
    conn.eliminate_zeros()
    conn.sort_indices()
    return conn


PLANTED = {"ring_cliques": _ring_of_cliques, "disjoint_cliques": _disjoint_cliques, "two_level": _two_level}
OTHER = {
    "lattice12": _lattice,
    "star5000": _star,
    "capacity_rows": _capacity_rows,
    "knn_blobs8": lambda: _knn_graph("knn_blobs8"),
    "knn_blobs6": lambda: _knn_graph("knn_blobs6"),
    "knn_flat": lambda: _knn_graph("knn_flat"),
    "wide_weights": lambda: _ring_of_cliques((1.0, 2.0**-30))[0],
    "n1": lambda: sparse.csr_matrix((1, 1)),
    "n2_edge": lambda: _sym(2, [0], [1]),
    "n5_empty": lambda: sparse.csr_matrix((5, 5)),
}
CASES = tuple(PLANTED) + tuple(OTHER)
NETWORKX_CASES = tuple(c for c in CASES if c not in ("n1", "n5_empty"))  # networkx has no modularity for a graph without edges


@functools.lru_cache(maxsize=None)
def matrix(name: str) -> sparse.csr_matrix:
    a = PLANTED[name]()[0] if name in PLANTED else OTHER[name]()
    a = sparse.csr_matrix(a, dtype=np.float64)
    a.data.setflags(write=False)
    return a


def planted(name: str) -> np.ndarray:
    return LO.canonical(PLANTED[name]()[1])


@functools.lru_cache(maxsize=None)
def graph(name: str) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    a = matrix(name)
    w = LO.quantise(a) if a.nnz else np.zeros(0, dtype=np.int32)
    out = (a.indptr.astype(np.int64), a.indices.astype(np.int32), w)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name: str, resolution: float) -> tuple[np.ndarray, dict]:
    """The oracle's labels and stats: computed once, shared by every test that needs them, never changed."""
    labels, stats = LO.leiden(*graph(name), resolution, -1)
    labels.setflags(write=False)
    return labels, stats


# ---- the object of the end-to-end tests ------------------------------------------------------------------------------------------------
N_DOMAINS, N_GENES = 5, 20


@functools.lru_cache(maxsize=None)
def _lattice_parts(side: int) -> tuple:
    rng = np.random.default_rng(31)
    row, col = np.divmod(np.arange(side * side), side)
    xy = np.c_[col + 0.5 * (row % 2), row * np.sqrt(3.0) / 2.0]  # hexagonal packing, nearest-neighbour distance 1
    pairs = cKDTree(xy).query_pairs(1.01, output_type="ndarray")
    adj = _sym(side * side, pairs[:, 0].tolist(), pairs[:, 1].tolist())
    centres = xy[rng.choice(side * side, size=N_DOMAINS, replace=False)]
    domain = np.argmin(((xy[:, None, :] - centres[None, :, :]) ** 2).sum(-1), axis=1)
    cell_type = np.where(rng.random(side * side) < 0.8, domain, rng.integers(0, N_DOMAINS, size=side * side))
    means = rng.gamma(2.0, 2.0, size=(N_DOMAINS, N_GENES))
    x = rng.poisson(means[cell_type]).astype(np.float64)
    library = np.where(col < side // 2, "A", "B")
    return adj, domain, cell_type, x, library


def lattice_adata(side: int = 30):
    """A ``side`` x ``side`` hexagonal lattice with 5 planted cell-type domains, 20 genes and two libraries; a fresh object per call."""
    import pandas as pd

    from squidpy_amd import AnnDataLite

    adj, domain, cell_type, x, library = _lattice_parts(side)
    obs = pd.DataFrame({"cell_type": pd.Categorical(cell_type.astype(str), categories=[str(i) for i in range(N_DOMAINS)]),
                        "domain": domain, "library": library}, index=[f"cell{i}" for i in range(side * side)])
    return AnnDataLite(X=x.copy(), obs=obs, obsp={"spatial_connectivities": adj.copy()})
