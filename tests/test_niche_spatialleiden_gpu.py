"""GPU: ``csrc/sqgr_leiden_multiplex.hip``, ``sq.gr.niche_spatialleiden`` and ``sq.gr.calculate_niche_spatialleiden``.

- ``sqgr_leiden_multiplex`` labels and all ten stats ``==`` the numpy restatement's (tests/niche_spatialleiden_oracle.py) bit for bit on
  every case x resolution pair x layer ratio of tests/niche_spatialleiden_cases.py — rows of the on-chip and of the global-memory path,
  the two rows whose summed lengths straddle the capacity, rows empty in one layer, an empty layer, the tiny inputs — and a second call
  returns the same bytes.
- ``sqgr_leiden_multiplex(G, empty)`` returns the bytes of ``sqgr_leiden(G)``.
- Fixed iteration counts; the device's refusals name the layer and the property.
- Launch geometry: every case at its first resolution pair and ratio again through ``sqgr_leiden_multiplex_hook`` with 1 and 3 blocks:
  the restatement's labels and stats and the bytes of the default call.
- The drop-in end to end on a 30 x 30 hexagonal lattice after ``sq.gr.niche_neighbors``: columns written, equal to
  ``niche_spatialleiden`` per resolution, and with ``library_key`` equal to two runs on the sub-objects."""

from __future__ import annotations

import numpy as np
import pytest

import squidpy_amd as sq
from squidpy_amd import _lib
from squidpy_amd._lib import default_context

from tests import niche_leiden_cases as LC
from tests import niche_leiden_oracle as LO
from tests import niche_spatialleiden_cases as MC
from tests import niche_spatialleiden_oracle as MO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return default_context(None)


def test_info_matches_the_restatement():
    info = _lib.leiden_multiplex_info()
    assert {k: info[k] for k in ("weight_bits", "sweep_cap", "iteration_cap", "capacity", "table_slots")} == {
        k: v for k, v in _lib.leiden_info().items() if k != "n_stats"}
    assert (info["weight_bits"], info["sweep_cap"], info["iteration_cap"]) == (LO.WEIGHT_BITS, LO.SWEEP_CAP, LO.ITER_CAP)
    assert info["n_layers"] == MO.N_LAYERS and info["n_stats"] == len(MO.STATS) == len(_lib.MULTIPLEX_STATS) and _lib.MULTIPLEX_STATS == MO.STATS
    l0, l1 = MC.layers("capacity_split")
    summed = np.diff(l0[0]) + np.diff(l1[0])
    assert summed[0] == info["capacity"] and summed[1] == info["capacity"] + 1  # one row on each side of the boundary
    assert np.diff(MC.layers("star_lattice")[1][0]).max() > info["capacity"]


@pytest.mark.parametrize("name,resolutions,ratio", MC.COMBOS)
def test_device_equals_the_restatement(ctx, name, resolutions, ratio):
    layers = MC.layers(name)
    labels, stats = _lib.leiden_multiplex(ctx, *layers, resolutions, ratio, -1)
    expected_labels, expected_stats = MC.expected(name, resolutions, ratio)
    assert labels.dtype == np.int32 and np.array_equal(labels, expected_labels)
    assert stats == expected_stats
    again, stats_again = _lib.leiden_multiplex(ctx, *layers, resolutions, ratio, -1)
    assert labels.tobytes() == again.tobytes() and stats == stats_again


@pytest.mark.parametrize("grid_blocks", [1, 3])
@pytest.mark.parametrize("name", MC.CASES)
def test_result_does_not_depend_on_the_grid(ctx, name, grid_blocks):
    resolutions, ratio = MC.RESOLUTIONS[0], MC.RATIOS[0]
    assert (name, resolutions, ratio) in MC.COMBOS
    layers = MC.layers(name)
    labels, stats = _lib.leiden_multiplex(ctx, *layers, resolutions, ratio, -1, grid_blocks=grid_blocks)
    expected_labels, expected_stats = MC.expected(name, resolutions, ratio)
    assert labels.dtype == np.int32 and np.array_equal(labels, expected_labels)
    assert stats == expected_stats
    default, default_stats = _lib.leiden_multiplex(ctx, *layers, resolutions, ratio, -1)
    assert labels.tobytes() == default.tobytes() and stats == default_stats


@pytest.mark.parametrize("resolution", LC.RESOLUTIONS)
@pytest.mark.parametrize("name", ["ring_cliques", "knn_blobs6", "capacity_rows"])
def test_empty_second_layer_returns_the_single_layer_bytes(ctx, name, resolution):
    graph = LC.graph(name)
    single, single_stats = _lib.leiden(ctx, *graph, resolution, -1)
    labels, stats = _lib.leiden_multiplex(ctx, graph, MC.empty_layer(single.shape[0]), (resolution, 1.0), 3.0, -1)
    assert labels.tobytes() == single.tobytes()
    assert {k: stats[k] for k in MO.SHARED_STATS} == {k: single_stats[k] for k in MO.SHARED_STATS}
    assert (stats["sum_in_0"], stats["two_m_0"], stats["sum_in_1"], stats["two_m_1"]) == (single_stats["sum_in"], single_stats["two_m"], 0, 0)


@pytest.mark.parametrize("n_iterations", [1, 2])
def test_fixed_iteration_counts(ctx, n_iterations):
    layers = MC.layers("lattice900")
    labels, stats = _lib.leiden_multiplex(ctx, *layers, (1.0, 1.0), 1.0, n_iterations)
    expected_labels, expected_stats = MO.leiden(*layers, (1.0, 1.0), 1.0, n_iterations)
    assert np.array_equal(labels, expected_labels) and stats == expected_stats and stats["iterations"] == n_iterations


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("damage,word", [("asymmetric", "symmetric"), ("self_loop", "self loop"), ("unsorted", "sorted"), ("weight", "weight"),
                                         ("index", "index")])
def test_device_refuses_and_names_layer_and_property(ctx, damage, word, layer):
    good = LC.graph("ring_cliques")
    indptr, indices, weights = (x.copy() for x in good)
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
    pair = ((indptr, indices, weights), good) if layer == 0 else (good, (indptr, indices, weights))
    with pytest.raises(_lib.SqgrError) as err:
        _lib.leiden_multiplex(ctx, *pair)
    assert err.value.status == -1 and word in str(err.value) and f"layer {layer}" in str(err.value)


def test_device_refuses_bad_coefficients(ctx):
    good = LC.graph("ring_cliques")
    for resolutions, ratio, word in [((0.0, 1.0), 1.0, "layer 0"), ((1.0, float("nan")), 1.0, "layer 1"), ((1.0, 1.0), 0.0, "layer_ratio"),
                                     ((1.0, 1.0), float("inf"), "layer_ratio")]:
        with pytest.raises(_lib.SqgrError) as err:
            _lib.leiden_multiplex(ctx, good, good, resolutions, ratio)
        assert err.value.status == -1 and word in str(err.value)
    with pytest.raises(_lib.SqgrError):
        _lib.leiden_multiplex(ctx, good, good, n_iterations=0)


def test_drop_in_end_to_end():
    resolutions = [1.0, (1.0, 0.5)]

    def prepared():
        adata = LC.lattice_adata()
        sq.gr.niche_neighbors(adata, n_neighbors=15)
        return adata

    adata = prepared()
    before = set(adata.obs.columns)
    assert sq.gr.calculate_niche_spatialleiden(adata, resolutions) is None
    assert set(adata.obs.columns) - before == {"spatialleiden_res=1.0", "spatialleiden_res=(1.0, 0.5)"}
    for res in resolutions:
        col = adata.obs[f"spatialleiden_res={res}"]
        direct = sq.gr.niche_spatialleiden(adata, res, copy=True)
        assert all(isinstance(v, str) for v in col) and list(col) == list(direct.labels.astype(str))
        assert 1 < col.nunique() < 200 and col.nunique() == direct.n_communities
        pair = sq.gr.niche_spatialleiden((adata.obsp["connectivities"], adata.obsp["spatial_connectivities"]), res)
        assert pair.labels.tobytes() == direct.labels.tobytes() and pair.quality == direct.quality

    by_lib = sq.gr.calculate_niche_spatialleiden(prepared(), resolutions, library_key="library", inplace=False).obs
    whole = prepared()
    for lib in ("A", "B"):
        rows = (whole.obs["library"] == lib).to_numpy()
        part = whole[rows, :]
        sq.gr.calculate_niche_spatialleiden(part, resolutions)
        for res in resolutions:
            key = f"spatialleiden_res={res}"
            assert list(by_lib[key][rows]) == [f"lib={lib}_{v}" for v in part.obs[key]]
