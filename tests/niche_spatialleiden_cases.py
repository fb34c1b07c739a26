"""Cases shared by tests/test_niche_spatialleiden_cpu.py and tests/test_niche_spatialleiden_gpu.py, built from the builders of
tests/niche_leiden_cases.py.  A case is a pair of float64 scipy CSR matrices (latent layer 0, spatial layer 1) over the same vertices;
``layers(name)`` returns what ``sqgr_leiden_multiplex`` takes, two ``(indptr int64, indices int32, weights int32)`` triples quantised
with one common scale by the oracle's restatement of the host step.

- ``ring_pair``: the ring of 8 cliques of 6, and the same graph relabelled by ``i -> 7 i mod 48`` — its cliques cut across layer 0's.
- ``ring_ring``, ``ring_empty``, ``empty_ring``: one ring graph, three ways.
- ``lattice900``: the fuzzy kNN-15 graph of the 30 x 30 lattice's 20-gene matrix over the hexagonal lattice itself.
- ``knn_blobs6_spatial``: ``knn_blobs6`` over a kNN-6 graph of random 2-D points, stored asymmetric (``W = A + A^T`` symmetrises it).
- ``star_lattice``: ``star5000`` in layer 1 over a sparse chain in layer 0: a row beyond the capacity whose length comes from one layer.
- ``capacity_split``: two hubs whose neighbours alternate between the layers, summed row lengths exactly ``capacity`` and
  ``capacity + 1``, every neighbour in a community of its own (its two partners are joined in both layers).
- ``layer1_only``: vertices whose rows are empty in layer 0; ``n1``, ``n2_edge`` (the edge in layer 1 only), ``n5_empty``."""

from __future__ import annotations

import functools

import numpy as np
from scipy import sparse
from scipy.spatial import cKDTree

from tests import niche_leiden_cases as LC
from tests import niche_neighbors_oracle as NO
from tests import niche_spatialleiden_oracle as MO

RESOLUTIONS = ((1.0, 1.0), (0.5, 2.0), (2.0, 0.5))
RATIOS = (2.0**-6, 1.0, 3.0, 2.0**6)
RING_PERMUTATION = (7 * np.arange(48)) % 48


def _empty(n: int) -> sparse.csr_matrix:
    return sparse.csr_matrix((n, n), dtype=np.float64)


def _ring_relabelled() -> sparse.csr_matrix:
    a = LC.matrix("ring_cliques").tocoo()
    p = RING_PERMUTATION
    out = sparse.coo_matrix((a.data, (p[a.row], p[a.col])), shape=a.shape).tocsr()
    out.sort_indices()
    return out


def _knn_of(x: np.ndarray) -> sparse.csr_matrix:
    dist, idx = cKDTree(x).query(x, k=15)
    dist, idx = dist[:, 1:], idx[:, 1:].astype(np.int32)
    conn = NO.connectivities(idx, NO.fuzzy(dist, float(dist.sum() / (x.shape[0] * 15))).vals).tocsr()
    conn.setdiag(0)
    conn.eliminate_zeros()
    conn.sort_indices()
    return conn


def _lattice900() -> tuple:
    adj, _, _, x, _ = LC._lattice_parts(30)
    return _knn_of(x), adj.copy()


def _knn_blobs6_spatial() -> tuple:
    n = LC.matrix("knn_blobs6").shape[0]
    xy = np.random.default_rng(41).random((n, 2))
    idx = cKDTree(xy).query(xy, k=7)[1][:, 1:]
    a = sparse.csr_matrix((np.ones(n * 6), (np.repeat(np.arange(n), 6), idx.ravel())), shape=(n, n))  # directed: i -> its 6 nearest
    a.sort_indices()
    assert (a != a.T).nnz > 0
    return LC.matrix("knn_blobs6"), a


def _star_lattice() -> tuple:
    star = LC.matrix("star5000")
    n = star.shape[0]
    i = np.arange(0, n - 48, 48)  # a sparse chain through hub, leaves and clique: 0 - 48 - 96 - ...
    return LC._sym(n, i.tolist(), (i + 48).tolist()), star


def _capacity_split() -> tuple:
    cap = LC.capacity()
    edges = ([], []), ([], [])
    nxt = 2
    for hub, deg in ((0, cap), (1, cap + 1)):
        for j in range(deg):
            for l in range(2):
                r, c = edges[l]
                if l == j % 2:  # the hub's entry for this neighbour is in one layer only
                    r.append(hub)
                    c.append(nxt)
                r += [nxt, nxt, nxt + 1]  # the neighbour's triangle is in both
                c += [nxt + 1, nxt + 2, nxt + 2]
            nxt += 3
    return tuple(LC._sym(nxt, r, c) for r, c in edges)


def _layer1_only() -> tuple:
    ring = LC.matrix("ring_cliques")
    n = 60  # vertices 48 .. 59 have empty rows in layer 0; in layer 1 they form two 6-cliques hung on the ring
    r, c = [], []
    for start in (48, 54):
        cr, cc = LC._clique(list(range(start, start + 6)))
        r += cr + [start]
        c += cc + [start - 48]
    l0 = sparse.csr_matrix((ring.data, ring.indices, np.r_[ring.indptr, np.full(12, ring.indptr[-1])]), shape=(n, n))
    return l0, LC._sym(n, r, c)


BUILDERS = {
    "ring_pair": lambda: (LC.matrix("ring_cliques"), _ring_relabelled()),
    "ring_ring": lambda: (LC.matrix("ring_cliques"), LC.matrix("ring_cliques")),
    "ring_empty": lambda: (LC.matrix("ring_cliques"), _empty(48)),
    "empty_ring": lambda: (_empty(48), LC.matrix("ring_cliques")),
    "lattice900": _lattice900,
    "knn_blobs6_spatial": _knn_blobs6_spatial,
    "star_lattice": _star_lattice,
    "capacity_split": _capacity_split,
    "layer1_only": _layer1_only,
    "n1": lambda: (_empty(1), _empty(1)),
    "n2_edge": lambda: (_empty(2), LC._sym(2, [0], [1])),
    "n5_empty": lambda: (_empty(5), _empty(5)),
}
CASES = tuple(BUILDERS)
COMBOS = [(name, res, ratio) for name in CASES for res in RESOLUTIONS for ratio in RATIOS]
QUALITY_CASES = ("lattice900", "knn_blobs6_spatial")


@functools.lru_cache(maxsize=None)
def matrices(name: str) -> tuple:
    out = tuple(sparse.csr_matrix(a, dtype=np.float64) for a in BUILDERS[name]())
    for a in out:
        a.data.setflags(write=False)
    return out


def _frozen(layer: tuple) -> tuple:
    for x in layer:
        x.setflags(write=False)
    return layer


@functools.lru_cache(maxsize=None)
def layers(name: str) -> tuple:
    return tuple(_frozen(layer) for layer in MO.quantise_pair(*matrices(name)))


def empty_layer(n: int) -> tuple:
    return _frozen((np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)))


def planted(name: str, layer: int) -> np.ndarray:
    """The planted cliques of ``ring_pair`` as layer ``layer`` sees them."""
    assert name == "ring_pair"
    base = np.repeat(np.arange(8), 6)
    if layer == 0:
        return LC.LO.canonical(base)
    out = np.empty(48, dtype=np.int64)
    out[RING_PERMUTATION] = base
    return LC.LO.canonical(out)


@functools.lru_cache(maxsize=None)
def expected(name: str, resolutions: tuple, ratio: float) -> tuple:
    """The oracle's labels and stats: computed once, shared by every test that needs them, never changed."""
    labels, stats = MO.leiden(*layers(name), resolutions, ratio, -1)
    labels.setflags(write=False)
    return labels, stats
