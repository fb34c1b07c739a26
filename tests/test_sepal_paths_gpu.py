"""GPU: the paths of csrc/sqgr_sepal.hip that the grids of tests/test_sepal_gpu.py do not reach — the LDS instances with 16 and 24
spots per thread (8 193-20 352 spots), the 32-bit lattice table (more than 65 536 spots), sweeps cut into several launches on both
routes (with a launch boundary on a gene's stop sweep, whose test then reads the entropy the previous launch left), and
``sq.gr.sepal`` on a lattice whose unsaturated spots all have a saturated neighbour — each against the numpy restatement."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import squidpy_amd as sq
from squidpy_amd import AnnDataLite
from squidpy_amd._lib import DeviceMatrix, SepalPlan, default_context
from squidpy_amd.gr._sepal import sepal_lattice
from tests import sepal_oracle as SO

pytestmark = pytest.mark.gpu

DT, THRESH, DELTA = 0.001, 1e-8, 1e-15
# run_batch of csrc/sqgr_sepal.hip: SEPAL_LAUNCH_BUDGET (LDS route), SEPAL_GLOBAL_BUDGET, and the 512 MB batch of expanded columns
LDS_BUDGET, GLOBAL_BUDGET, BATCH_BYTES = 6.0e10, 2.0e10, 512 << 20


def chunk_of(budget: float, genes: int, n: int, n_iter: int) -> int:
    """Sweeps per launch for a batch of `genes` genes: ``(int) max(1.0, min(n_iter, budget / (genes * n)))``, as run_batch forms it."""
    return int(max(1.0, min(float(n_iter), budget / (float(genes) * float(n)))))


def plan_for(g, xy, K):
    ctx = default_context()
    sat, sat_idx, unsat, nearest = sepal_lattice(g, xy, K)
    pos = np.empty(g.shape[0], np.int64)
    pos[sat] = np.arange(len(sat))
    return ctx, SepalPlan(ctx, g.shape[0], K, sat, sat_idx, unsat, pos[nearest] if len(unsat) else np.zeros(0, np.int32))


def adata(g, xy, X) -> AnnDataLite:
    return AnnDataLite(X=X, var=pd.DataFrame(index=[f"g{j}" for j in range(X.shape[1])]), obsm={"spatial": xy},
                       obsp={"spatial_connectivities": g})


def in_band(i: int, band: tuple[int, int]) -> bool:
    lo, hi = band
    if lo < 0:
        return i < 0
    return lo <= i <= (hi if hi >= 0 else lo)


def check_trace(g, xy, K, X, col, steps):
    ctx, plan = plan_for(g, xy, K)
    m = DeviceMatrix(ctx, X)
    lat = SO.compute_idxs(g, xy, K)
    _, _, ents, kept = SO.diffusion(X[:, col], K == 6, max(steps), lat, DT, None, keep=tuple(steps))
    for k in steps:
        conc, ent = plan.trace(m, col, k, DT)
        assert np.array_equal(conc, kept[k]), k
        assert np.all(np.abs(ent - ents[:k]) <= DELTA), k
    m.close()
    plan.close()


@pytest.mark.parametrize("rows, cols", [(120, 120), (135, 140)])
def test_lds_instances_with_16_and_24_spots_per_thread(rows, cols):
    xy, g = SO.hex_grid(rows, cols)
    n = len(xy)
    assert 8 * 1024 < n <= 20352 and ((n + 1023) // 1024 > 16) == (rows == 135)
    X = SO.spot_scale_genes(xy, 3, seed=2)
    lat = SO.compute_idxs(g, xy, 6)
    bands = [SO.band(SO.diffusion(X[:, j], True, 3000, lat, DT, THRESH)[1], THRESH) for j in range(3)]
    df = sq.gr.sepal(adata(g, xy, X), max_neighs=6, n_iter=3000, copy=True)
    for j in range(3):
        s = df.loc[f"g{j}", "sepal_score"]
        assert in_band(-1 if np.isnan(s) else int(round(s / DT)), bands[j]), (j, s, bands[j])
    check_trace(g, xy, 6, X, 1, (1, 7, 60))


@pytest.mark.parametrize("kind", ["square", "hex"])
def test_wide_table_above_65536_spots(kind):
    """260 x 260 = 67 600 spots: the global route with 32-bit lattice indices."""
    xy, g = SO.square_grid(260, 260) if kind == "square" else SO.hex_grid(260, 260)
    K = 4 if kind == "square" else 6
    X = np.random.default_rng(8).gamma(2.0, 1.0, size=(len(xy), 2))
    check_trace(g, xy, K, X, 0, (1, 3))
    lat = SO.compute_idxs(g, xy, K)
    band = SO.band(SO.diffusion(X[:, 1], K == 6, 1500, lat, DT, THRESH)[1], THRESH)
    ctx, plan = plan_for(g, xy, K)
    m = DeviceMatrix(ctx, X)
    it = plan.run(m, np.array([1], np.int32), 1500, DT, THRESH)
    assert in_band(int(it[0]), band), (it, band)
    m.close()
    plan.close()


def chunked_run(rows, cols, seed, picks, budget, n_iter):
    """Copies of the genes `picks` (columns of spot_scale_genes) as many times as make the launch chunk divide one of their stop
    sweeps; every copy must stop in its gene's band, all copies alike."""
    xy, g = SO.hex_grid(rows, cols)
    n = len(xy)
    X = np.ascontiguousarray(SO.spot_scale_genes(xy, max(picks) + 1, seed=seed)[:, picks])
    lat = SO.compute_idxs(g, xy, 6)
    runs = [SO.diffusion(X[:, j], True, n_iter, lat, DT, THRESH) for j in range(len(picks))]
    stops = [r[0] for r in runs]
    bands = [SO.band(r[1], THRESH) for r in runs]
    cap = min(max(1, BATCH_BYTES // (n * 8)), 65535)
    choice = next(((G, ch) for G in range(cap, len(picks) - 1, -1) for ch in [chunk_of(budget, G, n, n_iter)]
                   if ch < n_iter and any(s >= ch and s % ch == 0 for s in stops)), None)
    assert choice is not None, (stops, cap)
    G, ch = choice
    ctx, plan = plan_for(g, xy, 6)
    m = DeviceMatrix(ctx, X)
    cols_ = (np.arange(G) % len(picks)).astype(np.int32)
    it = plan.run(m, cols_, n_iter, DT, THRESH)
    for j in range(len(picks)):
        mine = it[cols_ == j]
        assert np.all(mine == mine[0]), j
        assert in_band(int(mine[0]), bands[j]), (j, int(mine[0]), bands[j], ch)
    m.close()
    plan.close()
    return stops, ch


def test_lds_route_sweeps_in_several_launches():
    """4 992 spots (LDS route); ~8 800 genes make the chunk 1 367 sweeps, one gene's stop sweep."""
    stops, ch = chunked_run(78, 64, 5, [4, 0], LDS_BUDGET, 6000)
    assert max(stops) >= ch  # a stop sweep in a later launch than the first (== ch: the first sweep of the second)


def test_global_route_sweeps_in_several_launches():
    """22 500 spots (global route); ~2 500 genes make the chunk 353 sweeps, one gene's stop sweep."""
    stops, ch = chunked_run(150, 150, 5, [1, 0], GLOBAL_BUDGET, 3000)
    assert max(stops) >= ch  # a stop sweep in a later launch than the first (== ch: the first sweep of the second)


def test_lattice_without_distance_query_on_the_device():
    """A hex grid without its two corner spots: no unsaturated spot lacks a saturated neighbour (the reference's sklearn call then
    raises); sq.gr.sepal scores it, in the restatement's bands."""
    xy, g = SO.hex_grid(8, 8)
    xy, g = SO.drop_spots(xy, g, SO.fallback_rows(g, 6))
    assert len(SO.fallback_rows(g, 6)) == 0
    X = SO.mixed_genes(xy, 4, seed=9)
    lat = SO.compute_idxs(g, xy, 6)
    df = sq.gr.sepal(adata(g, xy, X), max_neighs=6, copy=True)
    for j in range(4):
        band = SO.band(SO.diffusion(X[:, j], True, 30000, lat, DT, THRESH)[1], THRESH)
        s = df.loc[f"g{j}", "sepal_score"]
        assert in_band(-1 if np.isnan(s) else int(round(s / DT)), band), (j, s, band)
