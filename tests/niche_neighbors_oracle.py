"""A numpy restatement of ``csrc/sqgr_knn_nd.hip`` and of the host symmetrisation of ``squidpy_amd/gr/_niche_graph.py``, written from
their specification (include/sqgr.h) and independently of both:

- ``knn``: the per-coordinate sequential sum of squared differences (one rounded subtraction, product and sum per coordinate, ``j``
  ascending — sklearn's KD-tree ``rdist``), then ``np.lexsort`` by ``(d2, index)`` per row with the row itself removed by index.
- ``fuzzy``: UMAP's ``smooth_knn_dist`` / ``compute_membership_strengths`` for ``local_connectivity = 1``, row by row, with the C
  library's ``exp`` (``math.exp``), recording how far every decision of the search was from flipping.
- ``connectivities``: the literal scipy expression ``W + W.T - W.multiply(W.T)``."""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
from scipy import sparse

TOL = 1e-5     # SMOOTH_K_TOLERANCE
N_ITER = 64
MIN_K_DIST_SCALE = 1e-3


def d2_matrix(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    acc = np.zeros((n, n))
    for j in range(d):
        diff = x[:, None, j] - x[None, :, j]
        acc = acc + diff * diff
    return acc


def knn(x: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    d2 = d2_matrix(x)
    n = d2.shape[0]
    idx = np.empty((n, k), dtype=np.int32)
    out = np.empty((n, k))
    others = np.arange(n)
    for i in range(n):
        cand = others[others != i]
        row = d2[i, cand]
        order = np.lexsort((cand, row))[:k]
        idx[i] = cand[order]
        out[i] = row[order]
    return idx, out


class Fuzzy(NamedTuple):
    rho: np.ndarray
    sigma: np.ndarray       # after the clamp
    sigma_search: np.ndarray  # before it
    iters: np.ndarray
    vals: np.ndarray
    psum_last: np.ndarray   # psum of the last sweep
    floor_: np.ndarray      # what sigma was clamped against
    margin_stop: float      # min over rows and sweeps of | |psum - target| - TOL |
    margin_side: float      # min over the sweeps that went on of |psum - target|


def fuzzy(dist: np.ndarray, mean_all: float) -> Fuzzy:
    n, k = dist.shape
    m = k + 1
    target = math.log2(m)
    rho = np.zeros(n)
    sigma = np.zeros(n)
    sigma_search = np.zeros(n)
    iters = np.zeros(n, dtype=np.int32)
    vals = np.zeros((n, k))
    psum_last = np.zeros(n)
    floor_ = np.zeros(n)
    margin_stop = margin_side = math.inf
    for i in range(n):
        row = [float(v) for v in dist[i]]
        r = next((v for v in row if v > 0.0), 0.0)
        lo, hi, mid = 0.0, math.inf, 1.0
        last = 0
        for it in range(N_ITER):
            last = it
            psum = 0.0
            for v in row:
                e = v - r
                psum = psum + (math.exp(-(e / mid)) if e > 0.0 else 1.0)
            off = abs(psum - target)
            margin_stop = min(margin_stop, abs(off - TOL))
            if off < TOL:
                break
            margin_side = min(margin_side, off)
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        sigma_search[i] = mid
        if r > 0.0:
            total = 0.0
            for v in row:
                total = total + v
            floor_[i] = MIN_K_DIST_SCALE * (total / m)
        else:
            floor_[i] = MIN_K_DIST_SCALE * mean_all
        s = max(mid, floor_[i])
        rho[i], sigma[i], iters[i], psum_last[i] = r, s, last, psum
        vals[i] = [1.0 if (v - r <= 0.0 or s == 0.0) else math.exp(-((v - r) / s)) for v in row]
    return Fuzzy(rho, sigma, sigma_search, iters, vals, psum_last, floor_, margin_stop, margin_side)


def memberships(idx: np.ndarray, vals: np.ndarray) -> sparse.csr_matrix:
    n, k = idx.shape
    rows = np.repeat(np.arange(n), k)
    w = sparse.coo_matrix((vals.ravel(), (rows, idx.ravel())), shape=(n, n)).tocsr()
    w.eliminate_zeros()
    return w


def connectivities(idx: np.ndarray, vals: np.ndarray) -> sparse.csr_matrix:
    w = memberships(idx, vals)
    t = w.T
    c = (w + t - w.multiply(t)).tocsr()
    c.eliminate_zeros()
    c.sort_indices()
    return c
