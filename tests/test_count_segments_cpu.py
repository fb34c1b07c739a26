"""The host-side model of the segment list (tests/segments_model.py: key (r >> 4, c - r), threshold 8) on the lattices the count
kernel's segment path is meant for: its entries and residual edges hold every half edge exactly once, and the figures the design
quotes for these graphs."""

from __future__ import annotations

import numpy as np

from squidpy_amd._synthetic import hex_grid_graph
from tests.segments_model import all_entries, expand, half_edges, segment_model, sorted_edges, square_grid_graph


def _popcount(m: np.ndarray) -> np.ndarray:
    return np.array([bin(int(x)).count("1") for x in m], dtype=np.int64)


def _check_partition(adj):
    seg, res = segment_model(adj)
    he = half_edges(adj)
    both = np.concatenate([expand(seg), res.reshape(-1, 2)])
    np.testing.assert_array_equal(sorted_edges(both), sorted_edges(he))          # every half edge exactly once
    assert np.all(_popcount(seg[:, 2]) >= 8) and np.all(seg[:, 0] % 16 == 0) and np.all(seg[:, 1] > 0)
    key = seg[:, 0] * (1 << 32) + seg[:, 1]
    assert np.all(np.diff(key) > 0)                                              # ordered by (r0, d), no entry twice
    return seg, res, he


def test_hex_40x37_takes_both_paths():
    adj = hex_grid_graph(40, 37)
    seg, res, he = _check_partition(adj)
    assert len(he) == 4287
    assert len(all_entries(adj)) == 311
    assert len(seg) == 270
    assert len(he) - len(res) == 4124 and len(res) == 163
    assert len(np.unique(he[:, 1] - he[:, 0])) == 4                              # a hex lattice in scan order: four offsets


def test_hex_7x5():
    adj = hex_grid_graph(7, 5)
    seg, res, he = _check_partition(adj)
    assert len(he) == 82
    assert len(all_entries(adj)) == 9
    assert len(seg) == 5


def test_square_300x300_every_entry_but_one_dense():
    adj = square_grid_graph(300, 300)
    seg, res, he = _check_partition(adj)
    assert len(he) == 179_400
    assert len(all_entries(adj)) == 11_232
    assert len(seg) == 11_231
    assert len(np.unique(he[:, 1] - he[:, 0])) == 2
    assert len(he) - len(res) >= 0.99 * len(he)


def test_random_order_has_no_segments():
    from tests.segments_model import renumber

    adj = hex_grid_graph(40, 37)
    order = np.random.default_rng(0).permutation(adj.shape[0])
    seg, res, he = _check_partition(renumber(adj, order))
    assert len(seg) == 0 and len(res) == len(he)
