"""GPU: ``csrc/sqgr_leiden.hip``, ``sq.gr.niche_leiden`` and the two niche drop-ins.

- ``sqgr_leiden`` labels and stats ``==`` the numpy restatement's (tests/niche_leiden_oracle.py) bit for bit on every case x resolution
  of tests/niche_leiden_cases.py — rows of the on-chip and of the global-memory path, the two rows at the capacity boundary, the clamp
  to weight 1, the tiny inputs — and a second call returns the same bytes.  Planted cases ``==`` the planted labels.
- ``niche_leiden`` on the ``NicheNeighborsResult`` of the eight separated blobs recovers the blobs (adjusted Rand index 1: the two
  partitions are the same).
- ``calculate_niche_neighborhood`` / ``calculate_niche_utag`` end to end on a 30 x 30 hexagonal lattice with 5 planted cell-type domains
  and 20 genes: columns written, equal to the chain run step by step through the public functions, and with ``library_key`` equal to
  two separate runs on the sub-objects.
- The device's refusals name the property that failed.
- Launch geometry: every case at its first resolution again through ``sqgr_leiden_hook`` with 1 and 3 blocks (``k_best`` then takes
  n / 4 and n / 12 trips per block and reuses its LDS tables and per-wave slots; the element kernels stride too): the bytes of the
  default call.  Without the hook, a ring of six-cliques of more rows than the default grid's waves hold in one trip, against the
  restatement."""

from __future__ import annotations

import numpy as np
import pytest

import squidpy_amd as sq
from squidpy_amd import _lib
from squidpy_amd._lib import default_context

from tests import niche_leiden_cases as LC
from tests import niche_leiden_oracle as LO

pytestmark = pytest.mark.gpu

PAIRS = [(name, r) for name in LC.CASES for r in (LC.PLANTED_RESOLUTIONS if name in LC.PLANTED else LC.RESOLUTIONS)]


@pytest.fixture(scope="module")
def ctx():
    return default_context(None)


def test_info_matches_the_restatement():
    info = _lib.leiden_info()
    assert (info["weight_bits"], info["sweep_cap"], info["iteration_cap"]) == (LO.WEIGHT_BITS, LO.SWEEP_CAP, LO.ITER_CAP)
    assert info["capacity"] == LC.capacity() and info["table_slots"] > info["capacity"] and info["n_stats"] == len(_lib.LEIDEN_STATS)
    row_lengths = np.diff(LC.graph("capacity_rows")[0])
    assert row_lengths[0] == info["capacity"] and row_lengths[1] == info["capacity"] + 1  # one row on each side of the boundary
    assert np.diff(LC.graph("star5000")[0]).max() > info["capacity"]


@pytest.mark.parametrize("name,resolution", PAIRS)
def test_device_equals_the_restatement(ctx, name, resolution):
    graph = LC.graph(name)
    labels, stats = _lib.leiden(ctx, *graph, resolution, -1)
    expected_labels, expected_stats = LC.expected(name, resolution)
    assert labels.dtype == np.int32 and np.array_equal(labels, expected_labels)
    assert stats == expected_stats
    again, stats_again = _lib.leiden(ctx, *graph, resolution, -1)
    assert labels.tobytes() == again.tobytes() and stats == stats_again
    if name in LC.PLANTED:
        assert np.array_equal(labels, LC.planted(name))


@pytest.mark.parametrize("grid_blocks", [1, 3])
@pytest.mark.parametrize("name", LC.CASES)
def test_result_does_not_depend_on_the_grid(ctx, name, grid_blocks):
    resolution = (LC.PLANTED_RESOLUTIONS if name in LC.PLANTED else LC.RESOLUTIONS)[0]
    graph = LC.graph(name)
    labels, stats = _lib.leiden(ctx, *graph, resolution, -1, grid_blocks=grid_blocks)
    expected_labels, expected_stats = LC.expected(name, resolution)
    assert labels.dtype == np.int32 and np.array_equal(labels, expected_labels)
    assert stats == expected_stats
    default, default_stats = _lib.leiden(ctx, *graph, resolution, -1)
    assert labels.tobytes() == default.tobytes() and stats == default_stats


@pytest.mark.parametrize("resolution", [1.0, 50.0])
def test_ring_above_one_trip_of_the_default_grid(ctx, resolution):
    """q six-cliques on a ring, q chosen so that n = 6 q exceeds the 4 rows x 8 x compute units blocks that ``k_best`` covers in one
    trip (n = 12 000 > 8 192 on 256 compute units).  The planted cliques are not what these resolutions return: the restatement is
    the reference."""
    cu = ctx.device_info()["cu_count"]
    q = max(2000, (4 * 8 * cu) // 6 + 300)
    graph = LC.big_ring_graph(q)
    assert graph[0].shape[0] - 1 == 6 * q > 4 * 8 * cu
    labels, stats = _lib.leiden(ctx, *graph, resolution, -1)
    expected_labels, expected_stats = LO.leiden(*graph, resolution, -1)
    print("ring", q, "resolution", resolution, stats)
    assert np.array_equal(labels, expected_labels) and stats == expected_stats


@pytest.mark.parametrize("n_iterations", [1, 2])
def test_fixed_iteration_counts(ctx, n_iterations):
    graph = LC.graph("knn_blobs6")
    labels, stats = _lib.leiden(ctx, *graph, 1.0, n_iterations)
    expected_labels, expected_stats = LO.leiden(*graph, 1.0, n_iterations)
    assert np.array_equal(labels, expected_labels) and stats == expected_stats and stats["iterations"] == n_iterations


@pytest.mark.parametrize("damage,word", [("asymmetric", "symmetric"), ("self_loop", "self loop"), ("unsorted", "sorted"), ("weight", "weight"),
                                         ("index", "index")])
def test_device_refuses_and_names_the_property(ctx, damage, word):
    indptr, indices, weights = (x.copy() for x in LC.graph("ring_cliques"))
    if damage == "asymmetric":
        weights[0] += 1
    elif damage == "self_loop":
        indices[0] = 0
    elif damage == "unsorted":
        indices[[0, 1]] = indices[[1, 0]]
    elif damage == "weight":
        weights[0] = 0
    else:
        indices[0] = 48
    with pytest.raises(_lib.SqgrError) as err:
        _lib.leiden(ctx, indptr, indices, weights, 1.0)
    assert err.value.status == -1 and word in str(err.value)
    for resolution in (0.0, float("nan")):
        with pytest.raises(_lib.SqgrError):
            _lib.leiden(ctx, *LC.graph("ring_cliques"), resolution)


def test_blobs_are_recovered_from_niche_neighbors():
    x, member = LC.points("knn_blobs8")
    graph = sq.gr.niche_neighbors(x, 15)
    res = sq.gr.niche_leiden(graph, 1.0)
    assert res.n_communities == 8
    assert np.array_equal(res.labels, LO.canonical(member))  # the same partition: adjusted Rand index 1
    assert res.quality == LO.quality(*_csr(sq.gr.quantise_weights(graph.connectivities)), res.labels, 1.0)


def _csr(q):
    return q.indptr, q.indices, q.data


def _steps(adata, flavour, n_neighbors, resolutions):
    """The chain through the public functions, one call per stage."""
    if flavour == "neighborhood":
        embedding = sq.gr.niche_scale(sq.gr.niche_nhood_profile(adata, "cell_type"))
    else:
        embedding = sq.gr.niche_utag_embedding(adata)
    graph = sq.gr.niche_neighbors(embedding, n_neighbors)
    return {res: list(sq.gr.niche_leiden(graph, res).labels.astype(str)) for res in resolutions}


@pytest.mark.parametrize("flavour", ["neighborhood", "utag"])
def test_drop_in_end_to_end(flavour):
    base = "nhood_niche" if flavour == "neighborhood" else "utag_niche"

    def run(adata, resolutions, **kw):
        if flavour == "neighborhood":
            return sq.gr.calculate_niche_neighborhood(adata, "cell_type", resolutions, **kw)
        return sq.gr.calculate_niche_utag(adata, resolutions, **kw)

    adata = LC.lattice_adata()
    before = set(adata.obs.columns)
    assert run(adata, [0.5, 1.0]) is None
    assert set(adata.obs.columns) - before == {f"{base}_res=0.5", f"{base}_res=1.0"}
    steps = _steps(LC.lattice_adata(), flavour, 15, [0.5, 1.0])
    for res in (0.5, 1.0):
        col = adata.obs[f"{base}_res={res}"]
        assert all(isinstance(v, str) for v in col) and list(col) == steps[res]
        assert 1 < col.nunique() < 200

    by_lib = run(LC.lattice_adata(), 1.0, library_key="library", inplace=False).obs[f"{base}_res=1.0"]
    whole = LC.lattice_adata()
    for lib in ("A", "B"):
        rows = (whole.obs["library"] == lib).to_numpy()
        part = whole[rows, :]
        run(part, 1.0)
        assert list(by_lib[rows]) == [f"lib={lib}_{v}" for v in part.obs[f"{base}_res=1.0"]]
