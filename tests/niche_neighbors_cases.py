"""Shared inputs of the feature-space neighbour tests (tests/test_niche_neighbors_cpu.py, tests/test_niche_neighbors_gpu.py).  Every
case is small (``n <= 3000``); the oracle's results and sklearn's KD-tree answers are computed once per process and shared.  No device
compute here.

- Continuous normal clouds ``(n, D, n_neighbors)``: every D regime of the kernel (one strip of 32 columns, a partial strip, several
  strips, the largest D), the largest ``n_neighbors`` (65: 64 neighbours), ``n_neighbors = n`` (every other row is a neighbour), one
  cloud shifted by +1e3 and one float32 cloud.
- Edge shapes read from ``sqgr_knn_nd_info``: ``n`` at the query-block and candidate-tile sizes and at each +- 1.
- Tied data: 400 multinomial profile rows (about 140 distinct rows, many exact duplicates, rows whose bandwidth search runs all 64
  sweeps), a 4-D integer lattice, and 40 rows of which 20 are identical (``rho = 0`` and the ``mean_all`` clamp)."""

from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import niche_neighbors_oracle as O

QUERY_ROWS_FALLBACK = 64  # KN_Q and KN_C of csrc/sqgr_knn_nd.hip, for generating the cases without the library
TILE_ROWS_FALLBACK = 64


class Case(NamedTuple):
    n: int
    d: int
    n_neighbors: int
    seed: int
    kind: str = "normal"  # normal | shifted | float32 | profiles | lattice | duplicates


def kernel_info() -> dict[str, int]:
    try:
        from squidpy_amd import _lib

        return _lib.knn_nd_info()
    except OSError:
        return {"query_rows": QUERY_ROWS_FALLBACK, "tile_rows": TILE_ROWS_FALLBACK, "max_features": 256, "max_neighbors": 64}


def _edge_cases() -> dict[str, Case]:
    info = kernel_info()
    sizes = sorted({s + e for s in (info["query_rows"], info["tile_rows"]) for e in (-1, 0, 1)})
    return {f"edge_n{n}": Case(n, 7, 15, 100 + n) for n in sizes}


CONTINUOUS = {
    "n50_d1_m4": Case(50, 1, 4, 1),
    "n257_d2_m2": Case(257, 2, 2, 2),
    "n1000_d30_m15": Case(1000, 30, 15, 3),
    "n1500_d50_m15": Case(1500, 50, 15, 4),
    "n600_d65_m30": Case(600, 65, 30, 5),
    "n700_d64_m65": Case(700, 64, 65, 6),
    "n300_d256_m15": Case(300, 256, 15, 7),
    "n16_d5_m16": Case(16, 5, 16, 8),
    "shifted_1e3": Case(500, 10, 15, 9, "shifted"),
    "float32": Case(400, 12, 15, 10, "float32"),
    **_edge_cases(),
}
TIED = {
    "profiles": Case(400, 5, 15, 11, "profiles"),
    "lattice": Case(625, 4, 15, 12, "lattice"),
    "duplicates": Case(40, 3, 15, 13, "duplicates"),
}
CASES = {**CONTINUOUS, **TIED}


@functools.lru_cache(maxsize=None)
def data(name: str) -> np.ndarray:
    """The case's matrix as the caller holds it (float32 for the float32 case); read-only."""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    if c.kind == "profiles":
        x = rng.multinomial(6, [0.2] * 5, size=c.n) / 6.0
    elif c.kind == "lattice":
        side = round(c.n ** (1.0 / c.d))
        assert side**c.d == c.n
        x = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * c.d, indexing="ij"), -1).reshape(c.n, c.d)
        x = x[rng.permutation(c.n)]
    elif c.kind == "duplicates":
        x = rng.normal(size=(c.n, c.d))
        rows = rng.permutation(c.n)[: c.n // 2]
        x[rows] = x[rows[0]]
    else:
        x = rng.normal(size=(c.n, c.d))
        if c.kind == "shifted":
            x = x + 1e3
        if c.kind == "float32":
            x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def data64(name: str) -> np.ndarray:
    return data(name).astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle_knn(name: str):
    """``(indices, d2)`` of the numpy restatement, ``k = n_neighbors - 1`` columns."""
    idx, d2 = O.knn(data64(name), CASES[name].n_neighbors - 1)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


@functools.lru_cache(maxsize=None)
def oracle_fuzzy(name: str) -> "O.Fuzzy":
    dist = np.sqrt(oracle_knn(name)[1])
    return O.fuzzy(dist, float(dist.sum() / (dist.shape[0] * CASES[name].n_neighbors)))


@functools.lru_cache(maxsize=None)
def kdtree(name: str):
    """sklearn's ``(distances, indices)``: ``NearestNeighbors(n_neighbors=k, algorithm="kd_tree").fit(X).kneighbors()``."""
    from sklearn.neighbors import NearestNeighbors

    dist, idx = NearestNeighbors(n_neighbors=CASES[name].n_neighbors - 1, algorithm="kd_tree").fit(data(name)).kneighbors()
    dist.setflags(write=False)
    idx.setflags(write=False)
    return dist, idx
