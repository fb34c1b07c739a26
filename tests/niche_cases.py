"""Shared case table of the niche (Gaussian mixture) tests: tests/test_niche_cpu.py proves the properties of every case on sklearn
and on the numpy restatement (tests/niche_oracle.py); tests/test_niche_gpu.py runs them on the device.  No device compute here.

Every case is planted Gaussian data from its own fixed seed, at the smallest shape at which its code path can go wrong.  The CPU
test requires of every case and both seeds that sklearn's smallest margin between the best and the second-best weighted
log-density over ALL rows is at least ``MIN_MARGIN``: label tests then leave out no row.  A case that fails is given another seed
here, never an exemption."""

from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

SEEDS = (42, 1)  # random_state of every fit
MIN_MARGIN = 1e-6
REG_COVAR, TOL = 1e-6, 1e-3


class Case(NamedTuple):
    n: int
    d: int
    k: int
    seed: int          # of the data
    spread: float      # standard deviation of the planted centres (the clusters have unit scale)
    max_iter: int = 100
    offset: float = 0.0
    dups: int = 0      # copies of row 0 written over rows 1 .. dups - 1
    why: str = ""


CASES: dict[str, Case] = {
    "k1d1": Case(50, 1, 1, 9001, 3.0, why="scalar covariance, single component, logsumexp of one term"),
    "n_eq_k": Case(3, 2, 3, 9002, 3.0, why="every row is an initial centre; covariances are reg_covar I"),
    "d2k2": Case(40, 2, 2, 9003, 4.0, why="fewer rows than one wave"),
    "d1k3": Case(777, 1, 3, 9004, 6.0, why="d = 1 with several components"),
    "d17k6": Case(1037, 17, 6, 9005, 3.0, why="d != k, d no multiple of a tile, n no multiple of a block"),
    "overlap5": Case(3000, 5, 5, 9006, 1.0, why="heavily overlapping clusters, tens of EM steps"),
    "default10": Case(5250, 10, 10, 9007, 2.5, why="the front end's default, unequal cluster sizes"),
    "d32k32": Case(6000, 32, 32, 9008, 2.0, why="many tiles per covariance"),
    "d64k64": Case(8000, 64, 64, 9009, 1.5, why="the supported limit"),
    "dups": Case(500, 3, 4, 9010, 3.0, dups=40, why="40 identical rows (a near-singular component)"),
    "offset1e3": Case(2000, 4, 4, 9011, 3.0, offset=1e3, why="data shifted by 1e3: the centred covariance form"),
    "maxiter5": Case(3000, 5, 5, 9012, 1.0, max_iter=5, why="max_iter=5 reached without convergence"),
    # launch-geometry seams of csrc/sqgr_gmm.hip (gmm_geometry; tests/test_launch_geometry_cpu.py pins what binds), each at the smallest n at
    # which its caps bind
    "cap_rows": Case(262_657, 3, 4, 9101, 8.0, max_iter=6,
                     why="an E-step block walks two tiles, the last block one tile of one row; k_gmm_sums and k_gmm_cov at their chunk caps"),
    "cap_cov_k64": Case(16_897, 4, 64, 9113, 25.0, max_iter=10,
                        why="k_gmm_cov at its cap of 2048 / 64 chunks while k_gmm_sums is not; the last tile has one row"),
}
NAMES = tuple(CASES)
GEOMETRY_CASES = ("cap_rows", "cap_cov_k64")  # stop at max_iter or not as sklearn does; their margins to tol are pinned on the CPU


@functools.lru_cache(maxsize=None)
def data(name: str) -> np.ndarray:
    """The case's rows (n x d float64, read-only): ``k`` planted Gaussian clusters of unequal size with their own random covariance,
    rows in random order."""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    share = rng.dirichlet(np.full(c.k, 4.0)) if c.k > 1 else np.ones(1)
    member = rng.choice(c.k, size=c.n, p=share)
    centres = rng.normal(0.0, c.spread, (c.k, c.d))
    mix = rng.normal(0.0, 1.0, (c.k, c.d, c.d)) / np.sqrt(c.d) + np.eye(c.d) * 0.6
    x = centres[member] + np.einsum("nij,nj->ni", mix[member], rng.normal(0.0, 1.0, (c.n, c.d)))
    if c.dups:
        x[1 : c.dups] = x[0]
    x = np.ascontiguousarray(x + c.offset, dtype=np.float64)
    x.setflags(write=False)
    return x


class Reference(NamedTuple):
    weights: np.ndarray
    means: np.ndarray
    covariances: np.ndarray
    lower_bounds: np.ndarray
    n_iter: int
    converged: bool
    labels: np.ndarray
    margin: float  # smallest (best - second best) weighted log-density over all rows; inf for one component


def sklearn_fit(x: np.ndarray, k: int, random_state: int, max_iter: int = 100) -> Reference:
    """``GaussianMixture(k, random_state=random_state, init_params="random_from_data").fit(x)`` and ``.predict(x)`` as the reference
    calls them (gr/_niche.py:1474-1480), on this machine."""
    import warnings

    from sklearn.mixture import GaussianMixture

    gmm = GaussianMixture(n_components=k, random_state=random_state, init_params="random_from_data", max_iter=max_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm.fit(x)
    wlp = gmm._estimate_weighted_log_prob(x)
    labels = gmm.predict(x)
    assert np.array_equal(labels, wlp.argmax(axis=1))
    margin = float("inf")
    if k > 1:
        top = np.sort(wlp, axis=1)
        margin = float((top[:, -1] - top[:, -2]).min())
    return Reference(gmm.weights_, gmm.means_, gmm.covariances_, np.asarray(gmm.lower_bounds_), int(gmm.n_iter_), bool(gmm.converged_), labels, margin)


@functools.lru_cache(maxsize=None)
def reference(name: str, random_state: int) -> Reference:
    """sklearn's fit of the case, computed once per process and shared by the tests that need it."""
    c = CASES[name]
    return sklearn_fit(data(name), c.k, random_state, c.max_iter)


def close(got: np.ndarray, ref: np.ndarray) -> tuple[float, float]:
    """``(max |got - ref|, bound)`` with the bound of the GPU tests: ``1e-9 * max(1, max |ref|)``.  A correct implementation differs
    from sklearn by rounding order only (<= 3e-12 against values of order 1 to 1e3; <= 2.0e-10 in a covariance of ``cap_cov_k64``,
    whose values reach 217 on that seed, where two CPU orders differ by 7e-11); the smallest effect of a real error (a dropped
    ``reg_covar``, a wrong ``nk`` guard, one EM step too many or too few) is >= 1e-6 in a covariance."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref))) if ref.size else 0.0, 1e-9 * max(1.0, float(np.max(np.abs(ref))) if ref.size else 0.0)
