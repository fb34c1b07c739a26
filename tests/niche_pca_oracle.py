"""TEST INFRASTRUCTURE — a numpy restatement of ``niche_pca`` (squidpy_amd/gr/_niche.py, csrc/sqgr_pca.hip): centre first, then the
scatter matrix; LAPACK's symmetric eigensolver on ``scatter / (n - 1)``; eigenvalues descending and clamped at 0; sklearn's sign rule;
the projection as a loop over the columns j in ascending order, vectorised over the rows, every difference, product and sum rounded
on its own (numpy never fuses two array operations).  tests/test_niche_pca_cpu.py pins it to sklearn's ``PCA(svd_solver="arpack")``;
the GPU must reproduce ``project`` bit for bit and the moments within the order-free bound below.

Also the chain of the cellcharter flavour's ``use_rep=None`` path in restated form, and the bounds the tests derive (``U`` = 2^-53)."""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
from scipy.linalg import eigh

U = 2.0**-53
EPS = 2.0**-52


class PCA(NamedTuple):
    X_pca: np.ndarray
    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    mean: np.ndarray


def n_comps_rule(n: int, d: int) -> int:
    """scanpy's documented default: 50, or one less than the smaller side of the matrix where that is 50 or less."""
    return 50 if min(n, d) > 50 else min(n, d) - 1


def moments(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    x = np.asarray(x, dtype=np.float64)
    mean = x.sum(axis=0) / len(x)
    z = x - mean
    return mean, z.T @ z


def sign_rule(components: np.ndarray) -> np.ndarray:
    """sklearn's ``svd_flip(u_based_decision=False)``: in every row the entry of largest magnitude, the first on ties, is positive."""
    out = components.copy()
    for r, row in enumerate(out):
        pivot = 0
        for j in range(1, len(row)):
            if abs(row[j]) > abs(row[pivot]):
                pivot = j
        if row[pivot] < 0:
            out[r] = -row
    return out


def components_of(scatter: np.ndarray, n: int, c: int) -> tuple[np.ndarray, np.ndarray]:
    d = len(scatter)
    lam, vec = eigh(scatter / (n - 1), subset_by_index=[d - c, d - 1])
    order = np.argsort(-lam, kind="stable")
    return sign_rule(np.ascontiguousarray(vec[:, order].T)), np.maximum(lam[order], 0.0)


def project(x: np.ndarray, mean: np.ndarray, components: np.ndarray) -> np.ndarray:
    """``out[i][r] = sum_j (x[i][j] - mean[j]) * components[r][j]``, j ascending."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((len(components), len(x)), dtype=np.float64)  # transposed: the rows of x run along the contiguous axis
    prod = np.empty_like(out)  # one product array for all j: the same two rounded array operations per column, without 2 D allocations
    xt, ct = np.ascontiguousarray(x.T), np.ascontiguousarray(np.asarray(components, dtype=np.float64).T)  # column j of either, contiguous
    for j in range(x.shape[1]):
        diff = xt[j] - mean[j]
        np.multiply(ct[j][:, None], diff[None, :], out=prod)
        np.add(out, prod, out=out)
    return np.ascontiguousarray(out.T)


def pca(x: np.ndarray, c: int | None = None) -> PCA:
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    c = n_comps_rule(n, d) if c is None else c
    mean, scatter = moments(x)
    components, variance = components_of(scatter, n, c)
    return PCA(project(x, mean, components), components, variance, variance / (np.trace(scatter) / (n - 1)), mean)


# ---- the chain: features -> PCA -> mixture ------------------------------------------------------------------------------------------
def chain(features: np.ndarray, k: int, random_state: int):
    """The restated ``use_rep=None`` path behind the features: default PCA, then the restated mixture fit (tests/niche_oracle.py) on all
    columns of the embedding, started from the rows sklearn would draw."""
    from tests import niche_oracle

    from squidpy_amd.gr._niche import gmm_init_rows

    emb = pca(features).X_pca
    return niche_oracle.fit(emb, k, gmm_init_rows(len(emb), k, random_state))


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def exact_mean_and_bound(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Column means from exactly rounded sums (``math.fsum``) and the order-free bound of a computed one: any order of n - 1 additions
    and one division stays within ``gamma(n + 2) * sum |x_ij| / n`` of the exact quotient."""
    n = len(x)
    mean = np.array([math.fsum(col) / n for col in x.T])
    return mean, gamma(n + 2) * np.abs(x).sum(axis=0) / n


def exact_scatter_and_bound(x: np.ndarray, mean: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``sum_i z_ia z_ib`` for the rounded differences ``z = x - mean`` (the mean GIVEN: the device's own), every product formed
    exactly as a pair of doubles (error-free split: Dekker's two-product) and summed with ``math.fsum``; and the order-free bound
    ``gamma(n + 2) * sum_i |z_ia z_ib|`` — one rounding per product and n - 1 per sum, in any order."""
    z = np.asarray(x, dtype=np.float64) - mean
    d = z.shape[1]
    out, bound = np.zeros((d, d)), np.zeros((d, d))
    g = gamma(len(z) + 2)
    split = 134217729.0  # 2^27 + 1
    zs = z * split
    hi = zs - (zs - z)
    lo = z - hi
    for a in range(d):
        for b in range(a, d):
            p = z[:, a] * z[:, b]
            e = ((hi[:, a] * hi[:, b] - p) + hi[:, a] * lo[:, b] + lo[:, a] * hi[:, b]) + lo[:, a] * lo[:, b]  # p + e == the exact product
            out[a, b] = out[b, a] = math.fsum(np.concatenate([p, e]))
            bound[a, b] = bound[b, a] = g * np.abs(p).sum()
    return out, bound


def exact_scatter_pairs_and_bound(x: np.ndarray, mean: np.ndarray, pairs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``exact_scatter_and_bound`` for the entries ``pairs`` (m, 2) only: ``(exact[m], bound[m])``."""
    x = np.asarray(x, dtype=np.float64)
    g = gamma(len(x) + 2)
    split = 134217729.0  # 2^27 + 1
    cols = np.unique(pairs)
    z = {int(j): x[:, j] - mean[j] for j in cols}
    parts = {}
    for j, zj in z.items():
        zs = zj * split
        hi = zs - (zs - zj)
        parts[j] = (hi, zj - hi)
    out, bound = np.zeros(len(pairs)), np.zeros(len(pairs))
    for i, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        (ha, la), (hb, lb) = parts[a], parts[b]
        p = z[a] * z[b]
        e = ((ha * hb - p) + ha * lb + la * hb) + la * lb  # p + e == the exact product
        out[i] = math.fsum(np.concatenate([p, e]))
        bound[i] = g * np.abs(p).sum()
    return out, bound


def gaps(all_eigenvalues: np.ndarray, c: int) -> np.ndarray:
    """``gap_j``: the distance from eigenvalue j (descending, j < c) to its nearest other eigenvalue of the whole spectrum."""
    lam = np.sort(np.asarray(all_eigenvalues, dtype=np.float64))[::-1]
    out = np.empty(c)
    for j in range(c):
        others = np.delete(lam, j)
        out[j] = np.abs(others - lam[j]).min()
    return out
