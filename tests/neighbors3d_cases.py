"""Point sets and brute-force answers shared by the 3-D neighbour-search tests (GPU: tests/test_neighbors3d_gpu.py; the
host twin of the search on a CPU: tests/test_neighbors3d_cpu.py)."""

from __future__ import annotations

import numpy as np


def sk_knn(xyz, k):
    from sklearn.neighbors import NearestNeighbors

    assert k < len(xyz) // 2  # from n // 2 on sklearn answers by brute force, whose distance formula differs
    return NearestNeighbors(n_neighbors=k).fit(xyz).kneighbors()


def sk_radius_csr(xyz, r):
    """sklearn's radius_neighbors as CSR of distance + 1 (a zero distance stays a stored entry)"""
    import scipy.sparse as sp
    from sklearn.neighbors import NearestNeighbors

    n = len(xyz)
    rd, ri = NearestNeighbors(radius=r).fit(xyz).radius_neighbors()
    return sp.csr_matrix((np.concatenate(rd) + 1.0, (np.repeat(np.arange(n), [len(x) for x in ri]), np.concatenate(ri).astype(int))), shape=(n, n))


def lex_order(xyz, k):
    """The k nearest others of every point in ascending (d2, index) order, d2 = (dx*dx + dy*dy) + dz*dz, by brute force."""
    d = xyz[:, None, :] - xyz[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    np.fill_diagonal(d2, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(len(xyz)), d2.shape), d2), axis=1)[:, :k]
    return np.sqrt(np.take_along_axis(d2, order, axis=1)), order


def lattice(nx=9, ny=8, nz=7):
    return np.stack(np.meshgrid(np.arange(float(nx)), np.arange(float(ny)), np.arange(float(nz)), indexing="ij"), -1).reshape(-1, 3)


def stacked_sections(z_step: float):
    """1 500 points on six planes z = 0, z_step, ..., 5 z_step, xy rounded to 0.1 in [0, 300]^2, and 20 planted pairs: a copy
    of each of the first 20 points, same xy, on the adjacent plane."""
    rng = np.random.default_rng(17)
    xy = np.round(rng.random((1500, 2)) * 300, 1)
    plane = rng.integers(0, 6, 1500)
    twin = np.where(plane[:20] < 5, plane[:20] + 1, plane[:20] - 1)
    xyz = np.concatenate([np.column_stack([xy, plane * z_step]), np.column_stack([xy[:20], twin * z_step])])
    return xyz, np.arange(20), 1500 + np.arange(20)
