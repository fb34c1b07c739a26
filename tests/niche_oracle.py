"""A numpy restatement of the Gaussian mixture fit of ``csrc/sqgr_gmm.hip`` (sklearn 1.7's ``GaussianMixture`` with
``init_params="random_from_data"``, full covariances, ``n_init=1``) in a DIFFERENT summation order from sklearn's: sums over rows
are taken block by block (``BLOCK`` rows, the partials added in block order) and the E-step subtracts the mean before it multiplies
by the precision factor (sklearn multiplies ``X`` and the mean separately and subtracts the products).  tests/test_niche_cpu.py
compares it with sklearn on every case: an implementation that differs from sklearn only in rounding order reproduces its labels,
``n_iter_`` and ``converged_`` on these inputs — which is what the GPU tests then ask of the device."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
from scipy.linalg import solve_triangular

BLOCK = 1000


class Fit(NamedTuple):
    weights: np.ndarray
    means: np.ndarray
    covariances: np.ndarray
    lower_bounds: np.ndarray
    n_iter: int
    converged: bool
    labels: np.ndarray


def _blocks(a: np.ndarray) -> np.ndarray:
    """``a`` cut into blocks of ``BLOCK`` rows (zero rows appended to the last one): shape (blocks, BLOCK, ...)."""
    pad = -len(a) % BLOCK
    if pad:
        a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], dtype=a.dtype)])
    return a.reshape((-1, BLOCK) + a.shape[1:])


def _in_block_order(partials: np.ndarray) -> np.ndarray:
    acc = np.zeros(partials.shape[1:], dtype=np.float64)
    for p in partials:
        acc = acc + p
    return acc


def blocked_sum(a: np.ndarray) -> np.ndarray:
    """Sum over axis 0, ``BLOCK`` rows at a time, the partials added in block order."""
    return _in_block_order(_blocks(a).sum(axis=1))


def blocked_gram(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """``a.T @ b`` as the sum, in block order, of the products of the row blocks."""
    return _in_block_order(np.matmul(_blocks(a).transpose(0, 2, 1), _blocks(b)))


def m_step(x: np.ndarray, resp: np.ndarray, reg_covar: float, init: bool):
    n, d = x.shape
    k = resp.shape[1]
    nk = blocked_sum(resp) + 10 * np.finfo(np.float64).eps
    means = blocked_gram(resp, x) / nk[:, None]
    cov = np.empty((k, d, d))
    prec = np.empty((k, d, d))
    for c in range(k):
        diff = x - means[c]  # centred, two passes
        cov[c] = blocked_gram(resp[:, c, None] * diff, diff) / nk[c]
        cov[c].flat[:: d + 1] += reg_covar
        try:
            chol = np.linalg.cholesky(cov[c])
        except np.linalg.LinAlgError:
            raise ValueError("ill-defined empirical covariance") from None
        prec[c] = solve_triangular(chol, np.eye(d), lower=True).T
    weights = nk / n if init else nk / nk.sum()
    return weights, means, cov, prec


def weighted_log_prob(x: np.ndarray, weights: np.ndarray, means: np.ndarray, prec: np.ndarray) -> np.ndarray:
    n, d = x.shape
    out = np.empty((n, len(weights)))
    for c in range(len(weights)):
        y = (x - means[c]) @ prec[c]  # subtract, then multiply
        out[:, c] = -0.5 * (d * np.log(2 * np.pi) + (y * y).sum(axis=1)) + np.log(np.diagonal(prec[c])).sum() + np.log(weights[c])
    return out


def fit(x: np.ndarray, k: int, init_rows: np.ndarray, reg_covar: float = 1e-6, tol: float = 1e-3, max_iter: int = 100) -> Fit:
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    resp = np.zeros((n, k))
    resp[np.asarray(init_rows), np.arange(k)] = 1.0
    weights, means, cov, prec = m_step(x, resp, reg_covar, True)
    lb, lbs, converged = -np.inf, [], False
    for _ in range(max_iter):
        prev = lb
        wlp = weighted_log_prob(x, weights, means, prec)
        top = wlp.max(axis=1)
        lpn = np.log(np.exp(wlp - top[:, None]).sum(axis=1)) + top
        resp = np.exp(wlp - lpn[:, None])
        lb = float(blocked_sum(lpn[:, None])[0] / n)
        weights, means, cov, prec = m_step(x, resp, reg_covar, False)
        lbs.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
    labels = weighted_log_prob(x, weights, means, prec).argmax(axis=1)
    return Fit(weights, means, cov, np.array(lbs), len(lbs), converged, labels)
