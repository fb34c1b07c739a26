"""CPU: what the 3-D neighbour search decides before it reaches the device — the accepted coordinate widths of
``knn_self`` / ``radius_self`` and of the graph builders, the new entry points of the C ABI — and the search itself: the
kernels' query bodies are host-callable, so the cell sizing, the shell walk and its stop rule run here on the host
(tests/neighbors3d_host_twin.hip) against sklearn and brute force."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from squidpy_amd import _build, _lib
from squidpy_amd.gr._build import _build_one, _Spec
from tests import neighbors3d_cases as cases


def test_both_searches_are_bound():
    assert _lib.SIGNATURES["sqgr_knn_self3"] == _lib.SIGNATURES["sqgr_knn_self"]
    assert _lib.SIGNATURES["sqgr_radius_self3"] == _lib.SIGNATURES["sqgr_radius_self"]


@pytest.mark.parametrize("shape", [(30, 4), (30, 1), (30,), (5, 3, 2)])
def test_other_widths_are_refused_by_name(shape):
    bad = np.zeros(shape)
    with pytest.raises(ValueError, match=r"Expected coordinates of shape \(n, 2\) or \(n, 3\), found"):
        _lib.knn_self(None, bad, 3)
    with pytest.raises(ValueError, match=r"Expected coordinates of shape \(n, 2\) or \(n, 3\), found"):
        _lib.radius_self(None, bad, 1.0)
    for spec in (_Spec("knn"), _Spec("radius", radius=1.0), _Spec("grid")):
        with pytest.raises(NotImplementedError, match="handles 2-D or 3-D coordinates"):
            _build_one(None, bad, spec)


def test_too_few_samples_is_sklearns_error_for_3d():
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 4, n_samples_fit = 3, n_samples = 3"):
        _lib.knn_self(None, np.zeros((3, 3)), 3)


# ------------------------------------------------------------------------------------ the search itself, on the CPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class Twin:
    """tests/neighbors3d_host_twin.hip: the kernels' query bodies and the cell-list builder, run on the host"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.twin_knn3.argtypes = [f64p, C.c_int64, C.c_int, i32p, f64p, f64p]
        self.lib.twin_radius3.argtypes = [f64p, C.c_int64, C.c_double, i64p, i32p, f64p]
        self.lib.twin_radius3.restype = C.c_int64

    def knn(self, xyz, k):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        n = len(xyz)
        idx, d2, grid = np.zeros((n, k), np.int32), np.zeros((n, k)), np.zeros(6)
        assert self.lib.twin_knn3(xyz.ctypes.data_as(f64p), n, k, idx.ctypes.data_as(i32p), d2.ctypes.data_as(f64p), grid.ctypes.data_as(f64p)) == 0
        return np.sqrt(d2), idx, dict(h=grid[0], cells=tuple(int(g) for g in grid[1:4]), fill=n / grid[4], most=int(grid[5]))

    def radius_csr(self, xyz, r):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        n = len(xyz)
        indptr = np.zeros(n + 1, np.int64)
        nnz = self.lib.twin_radius3(xyz.ctypes.data_as(f64p), n, r, indptr.ctypes.data_as(i64p), None, None)
        assert nnz >= 0
        idx, d2 = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1))
        assert self.lib.twin_radius3(xyz.ctypes.data_as(f64p), n, r, indptr.ctypes.data_as(i64p), idx.ctypes.data_as(i32p), d2.ctypes.data_as(f64p)) == nnz
        return sp.csr_matrix((np.sqrt(d2[:nnz]) + 1.0, idx[:nnz], indptr), shape=(n, n))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    lib = _build.build(verbose=False)  # set_error lives in libsqgr.so
    out = str(tmp_path_factory.mktemp("twin") / "libneighbors3d_twin.so")
    subprocess.check_call([_build._hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           os.path.join(ROOT, "tests", "neighbors3d_host_twin.hip"), "-I", _build.CSRC, "-I", os.path.join(ROOT, "include"),
                           "-o", out, "-L", _build.CSRC, "-lsqgr", "-Wl,-rpath," + os.path.dirname(lib), "-Wno-unused-function"])
    return Twin(out)


def _same(a, b):
    return a.shape == b.shape and (a != b).nnz == 0


@pytest.mark.parametrize("n,k", [(50, 3), (1000, 6), (3000, 15), (2500, 40)])
def test_host_twin_knn_equals_sklearn(twin, n, k):
    xyz = np.random.default_rng(n + k).random((n, 3)) * np.array([1000.0, 30.0, 200.0])
    dist, idx, _ = twin.knn(xyz, k)
    rd, ri = cases.sk_knn(xyz, k)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist, rd)


def test_host_twin_ties_go_to_the_smaller_index(twin):
    g = cases.lattice()
    xyz = np.concatenate([g, g[:7]])
    for k in (5, 64):  # 64: shells beyond the first, every KMAX of the ladder is the same code
        dist, idx, _ = twin.knn(xyz, k)
        bd, order = cases.lex_order(xyz, k)
        np.testing.assert_array_equal(idx, order)
        np.testing.assert_array_equal(dist, bd)


@pytest.mark.parametrize("z_step", [0.01, 50.0, 5000.0, 1e6])
def test_cell_sizing_of_stacked_sections(twin, z_step):
    """Sections far closer than the in-plane spacing (~19), wider apart and very far apart: a few points per occupied cell every
    time — never one cell per section, never a point per column of empty cells — and the answers stay sklearn's."""
    xyz, first, second = cases.stacked_sections(z_step)
    dist, idx, grid = twin.knn(xyz, 6)
    assert 1.0 <= grid["fill"] <= 4.0 and grid["most"] <= 16, grid
    assert np.prod(grid["cells"][:2]) <= 4 * len(xyz) + 64, grid
    if z_step == 0.01:
        assert grid["cells"][2] == 1, grid  # a thin axis holds one layer of cells
    rd, _ = cases.sk_knn(xyz, 6)
    np.testing.assert_array_equal(dist, rd)
    np.testing.assert_array_equal(idx, cases.lex_order(xyz, 6)[1])
    bd, order = cases.lex_order(xyz, 40)  # more than a section's neighbourhood: the walk crosses the empty layers
    d40, i40, _ = twin.knn(xyz, 40)
    np.testing.assert_array_equal(i40, order)
    np.testing.assert_array_equal(d40, bd)


def test_cell_sizing_of_degenerate_extents(twin):
    rng = np.random.default_rng(4)
    flat = np.column_stack([rng.random((2000, 2)) * np.array([800.0, 90.0]), np.full(2000, 12.5)])
    line = np.column_stack([rng.random(1500) * 1e4, np.full(1500, -3.0), np.full(1500, 7.0)])
    for xyz, layers in ((flat, (None, None, 1)), (line, (None, 1, 1))):
        dist, idx, grid = twin.knn(xyz, 6)
        assert 1.0 <= grid["fill"] <= 4.0, grid
        assert all(want is None or got == want for got, want in zip(grid["cells"], layers)), grid
        rd, ri = cases.sk_knn(xyz, 6)
        np.testing.assert_array_equal(dist, rd)
        np.testing.assert_array_equal(idx, ri)
    site = np.tile(np.array([[3.0, -1.0, 2.5]]), (40, 1))
    dist, idx, grid = twin.knn(site, 3)
    assert grid["cells"] == (1, 1, 1) and (dist == 0.0).all()
    np.testing.assert_array_equal(idx, [[j for j in range(4) if j != i][:3] for i in range(40)])


@pytest.mark.parametrize("r", [0.0, 7.5, 50.0, 60.0, 1e4])
def test_host_twin_radius_equals_sklearn(twin, r):
    xyz, first, second = cases.stacked_sections(50.0)
    got = twin.radius_csr(xyz, r)
    assert _same(got, cases.sk_radius_csr(xyz, r))
    if r == 50.0:
        assert (np.asarray(got[first, second]).ravel() == 51.0).all()


@pytest.mark.parametrize("seed", range(8))
def test_host_twin_on_odd_clouds(twin, seed):
    """Scales from 1e-3 to 1e5 per axis, large offsets, rounded coordinates (ties), a dense cluster inside a sparse cloud."""
    rng = np.random.default_rng(100 + seed)
    n, k = int(rng.integers(130, 1200)), int(rng.integers(1, 64))
    xyz = rng.random((n, 3)) * 10.0 ** rng.integers(-3, 6, 3) + 10.0 ** rng.integers(0, 7)
    if seed % 3 == 0:
        xyz = np.round(xyz, int(rng.integers(0, 3)))
    if seed % 4 == 1:
        xyz[: n // 2] = xyz[: n // 2] * 1e-3 + xyz[0]
    dist, idx, _ = twin.knn(xyz, k)
    bd, order = cases.lex_order(xyz, k)
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_array_equal(dist, bd)
    np.testing.assert_array_equal(dist, cases.sk_knn(xyz, k)[0])
    r = float(np.median(dist[:, -1]))
    assert _same(twin.radius_csr(xyz, r), cases.sk_radius_csr(xyz, r))
