"""Shared inputs of the PCA tests (tests/test_niche_pca_cpu.py, tests/test_niche_pca_gpu.py): planted matrices with a known spectrum and
the chain cases of the cellcharter flavour's ``use_rep=None`` path.  sklearn's results are computed once per process and shared.  No
device compute here.

A planted matrix: Gaussian clusters in a latent space whose axes have geometrically decaying scales (``lambda_c / lambda_1`` about
1e-3 for the ``c`` components asked for, so neighbouring eigenvalues stay a few percent of their size apart), lifted to ``D`` columns by
a random orthonormal map, plus a constant offset of 5 (one case: 1e3)."""

from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import niche_features_cases as FC

EPS = 2.0**-52
GAP_CONDITION = 1e-10  # eps * lambda_1 / gap_j of every component of every case
# The constant of tol_j = C * eps * lambda_1 / gap_j * max |scores|: 8 x the largest ratio the numpy restatement shows against sklearn
# over the committed cases (21.34, case shifted_1e3) — measured and explained in tests/test_niche_pca_cpu.py and DESIGN §3.8.
C = 171.0
CHUNK_FALLBACK = 512   # PCA_CHUNK of csrc/sqgr_pca.hip, for generating the cases without the library


class Case(NamedTuple):
    n: int
    d: int
    c: int
    seed: int
    offset: float = 5.0
    constant_column: bool = False
    float32: bool = False


CASES = {
    "n3_d2_c1": Case(3, 2, 1, 1),
    "n65_d5_c4": Case(65, 5, 4, 2),
    "n300_d12_c11": Case(300, 12, 11, 3),
    "n257_d63_c50": Case(257, 63, 50, 4),
    "n500_d64_c50": Case(500, 64, 50, 5),
    "n513_d65_c64": Case(513, 65, 64, 6),
    "n700_d130_c50": Case(700, 130, 50, 7),
    "shifted_1e3": Case(400, 40, 20, 8, offset=1e3),
    "constant_column": Case(300, 30, 12, 9, constant_column=True),
    "float32": Case(350, 33, 16, 10, float32=True),
}

# Launch-geometry seams of csrc/sqgr_pca.hip (pca_geometry): used by the moments and projection tests only — the host eigenproblem of
# a 4096 x 4096 matrix is not what they are about.  tests/test_launch_geometry_cpu.py pins what binds in each.
SEAM_CASES = {
    "mean_cap": Case(524_289, 3, 2, 21),        # column sums in chunks of 1024 rows (513 of them, the last of one row); scatter likewise
    "limit_d4096": Case(1_025, 4096, 64, 22),   # the largest D: 64 tiles, 2 080 tile pairs, one chunk whose last sub-tile has one row
    "capped_chunks": Case(5_633, 1100, 50, 23), # 171 tile pairs cap the scatter at 11 < 12 chunks: 6 chunks of 1024 rows, the last of 513
}
SEAM_NAMES = tuple(SEAM_CASES)


def chunk_rows() -> int:
    """Rows of a chunk of the scatter kernel, from the library (``sqgr_pca_info``: no device needed)."""
    from squidpy_amd._lib import pca_info

    return pca_info()["chunk_rows"]


def chunk_cases(chunk: int) -> dict[str, Case]:
    """One row past the scatter kernel's row chunk, and one row short of it."""
    return {"chunk_plus_1": Case(chunk + 1, 20, 10, 11), "chunk_minus_1": Case(chunk - 1, 20, 10, 12)}


def case(name: str) -> Case:
    if name in CASES:
        return CASES[name]
    if name in SEAM_CASES:
        return SEAM_CASES[name]
    try:
        chunk = chunk_rows()
    except OSError:
        chunk = CHUNK_FALLBACK
    return chunk_cases(chunk)[name]


NAMES = tuple(CASES) + tuple(chunk_cases(CHUNK_FALLBACK))


@functools.lru_cache(maxsize=None)
def data(name: str) -> np.ndarray:
    """The case's matrix, read-only: float64, or float32 for the float32 case."""
    c = case(name)
    rng = np.random.default_rng(c.seed)
    d_live = c.d - 1 if c.constant_column else c.d
    latent = min(d_live, c.c + 6)
    ratio = 1e-2 ** (0.5 / max(c.c, 2))  # scale of axis l: ratio^l, so lambda_c / lambda_1 ~ 1e-2 before the centres widen lambda_1
    scales = ratio ** np.arange(latent)
    centres = rng.normal(0.0, 2.0, (4, latent))
    z = (centres[rng.integers(0, 4, c.n)] + rng.normal(0.0, 1.0, (c.n, latent))) * scales
    lift, _ = np.linalg.qr(rng.normal(0.0, 1.0, (d_live, latent)))
    x = z @ lift.T + c.offset
    if c.constant_column:
        x = np.insert(x, c.d // 2, 3.25, axis=1)
    x = np.ascontiguousarray(x, dtype=np.float32 if c.float32 else np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def seam_components(name: str) -> np.ndarray:
    """``c`` orthonormal rows of length ``D`` from the case's seed (read-only): components for the projection without an eigenproblem."""
    c = SEAM_CASES[name]
    basis, _ = np.linalg.qr(np.random.default_rng(c.seed + 1000).normal(0.0, 1.0, (c.d, c.c)))
    out = np.ascontiguousarray(basis.T)
    out.setflags(write=False)
    return out


def data64(name: str) -> np.ndarray:
    """What sklearn is given: the matrix widened to float64 (exact)."""
    return np.asarray(data(name), dtype=np.float64)


class Reference(NamedTuple):
    scores: np.ndarray
    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    mean: np.ndarray
    spectrum: np.ndarray  # every eigenvalue of the covariance (sklearn's full solver), descending


def sklearn_pca(x: np.ndarray, c: int):
    """scanpy's default ``sc.tl.pca`` on a dense matrix."""
    from sklearn.decomposition import PCA

    return PCA(n_components=c, svd_solver="arpack", random_state=0)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    from sklearn.decomposition import PCA

    x, c = data64(name), case(name).c
    model = sklearn_pca(x, c)
    scores = model.fit_transform(x)
    full = PCA(svd_solver="full").fit(x)
    spectrum = np.zeros(x.shape[1])
    spectrum[: len(full.explained_variance_)] = full.explained_variance_
    return Reference(scores, model.components_, model.explained_variance_, model.explained_variance_ratio_, model.mean_, spectrum)


def tolerances(name: str, constant: float) -> np.ndarray:
    """``tol_j / max |scores| = constant * eps * lambda_1 / gap_j`` for the case's components."""
    from tests import niche_pca_oracle as O

    ref = reference(name)
    return constant * EPS * ref.spectrum[0] / O.gaps(ref.spectrum, case(name).c)


# ---- chain cases: graph + X -> features -> PCA -> mixture -----------------------------------------------------------------------------
class Chain(NamedTuple):
    graph: str          # "hex" | "knn"
    n_vars: int
    distance: int
    k: int              # mixture components
    seed: int
    libraries: int = 1
    random_state: int = 42


CHAINS = {
    "hex_d2": Chain("hex", 12, 2, 4, 31),
    "knn_d3_k4": Chain("knn", 20, 3, 4, 32),
    "knn_d3_k10": Chain("knn", 20, 3, 10, 32),
    "two_libraries": Chain("two", 12, 2, 3, 33, libraries=2),
}
CHAIN_NAMES = tuple(CHAINS)
MIN_MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def chain_inputs(name: str):
    """``(graph CSR of ones, X float64 (n, n_vars), library of every row)``: planted domains that are contiguous in space, so that the
    shell means keep them apart."""
    from scipy import sparse

    ch = CHAINS[name]
    rng = np.random.default_rng(ch.seed)
    if ch.graph == "hex":
        a = FC.hex_lattice(20, 20)
        pos = np.stack(np.divmod(np.arange(400), 20), axis=1) / 20.0
        library = np.zeros(400, dtype=np.int64)
    elif ch.graph == "knn":
        a = FC.knn_graph(1500, 6, ch.seed)
        pos = np.random.default_rng(ch.seed).random((1500, 2))  # the points knn_graph draws
        library = np.zeros(1500, dtype=np.int64)
    else:  # two lattices side by side, no edge between them, rows interleaved in blocks
        one, two = FC.hex_lattice(14, 15), FC.hex_lattice(12, 16)
        a = sparse.block_diag([one, two], format="csr")
        pos = np.concatenate([np.stack(np.divmod(np.arange(210), 15), axis=1) / 15.0, np.stack(np.divmod(np.arange(192), 16), axis=1) / 16.0])
        library = np.concatenate([np.zeros(210, dtype=np.int64), np.ones(192, dtype=np.int64)])
        order = np.argsort(rng.integers(0, 6, len(library)), kind="stable")  # mixes the two libraries' rows
        a = a[order][:, order].tocsr()
        a.sort_indices()
        pos, library = pos[order], library[order]
    n = a.shape[0]
    domain = (pos[:, 0] > 0.5).astype(np.int64) + 2 * (pos[:, 1] > 0.5).astype(np.int64)  # four quadrants
    centres = rng.normal(0.0, 3.0, (4, ch.n_vars))
    scales = 0.8 ** np.arange(ch.n_vars)
    x = np.ascontiguousarray(centres[domain] + rng.normal(0.0, 1.0, (n, ch.n_vars)) * scales + 5.0)
    a = a.astype(np.float64)
    a.sum_duplicates()
    x.setflags(write=False)
    return a, x, library


class ChainReference(NamedTuple):
    labels: np.ndarray
    n_iter: tuple
    converged: tuple
    margin: float


def sklearn_chain(features_of, name: str) -> ChainReference:
    """features (``features_of(graph, X, distance)``) -> sklearn PCA with scanpy's default number of components -> sklearn's
    ``GaussianMixture`` in float64, per library; the labels of library ``l`` land in its rows."""
    from tests import niche_cases
    from tests import niche_pca_oracle as O

    ch = CHAINS[name]
    a, x, library = chain_inputs(name)
    labels = np.full(len(library), -1, dtype=np.int64)
    n_iter, converged, margin = [], [], float("inf")
    for lib in range(ch.libraries):
        rows = np.flatnonzero(library == lib)
        sub = a[rows][:, rows].tocsr()
        sub.sort_indices()
        feats = np.asarray(features_of(sub, x[rows], ch.distance), dtype=np.float64)
        emb = sklearn_pca(feats, O.n_comps_rule(*feats.shape)).fit_transform(feats)
        fit = niche_cases.sklearn_fit(emb, ch.k, ch.random_state)
        labels[rows] = fit.labels
        n_iter.append(fit.n_iter)
        converged.append(fit.converged)
        margin = min(margin, fit.margin)
    return ChainReference(labels, tuple(n_iter), tuple(converged), margin)
