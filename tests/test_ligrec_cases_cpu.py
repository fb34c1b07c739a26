"""CPU proof of the builders in tests/ligrec_cases.py, on the oracle alone and at the shapes tests/test_ligrec_regimes_gpu.py
uses: every planted threshold really sits on (or one ulp below) a permuted sum of the permutation that owns it, every
permutation of a range owns both kinds, and a one-ulp nudge of a planted threshold changes the oracle's count at every planted
cell — so a device sum that is wrong in its last bit, in any lane, changes a count too.  No device compute here."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import restate as O
from tests import ligrec_cases as C


def _labels(cl, generator):
    if generator == "numpy":
        return O.ligrec_perm_labels_numpy(cl, 11, C.N_NUMPY)
    return C.philox_labels(cl, 1234, C.DEVICE_BEGIN, C.DEVICE_BEGIN + C.N_DEVICE)


def _check_planted(data, labels, inv, inter, cp, perms=None):
    obs, tie, below = C.planted_obs(data, labels, inv, inter, cp, perms)
    owner = C.cell_owners(obs.shape, len(labels) if perms is None else perms)
    owners = np.unique(owner)
    assert (tie ^ below).all()
    # every permutation of the range owns at least one cell of either kind
    assert set(owner[tie]) == set(owners) and set(owner[below]) == set(owners)
    assert len(owners) == (len(labels) if perms is None else len(perms))
    # the owning permutation's sum: equal at the ties (contributes 0), one ulp above at the others (contributes 1)
    own = np.empty(obs.shape)
    for p in owners:
        own[owner == p] = C.shuffled_sums(data, labels[p], inv, inter, cp)[owner == p]
    assert np.isfinite(own).all()
    np.testing.assert_array_equal(own[tie], obs[tie])
    np.testing.assert_array_equal(np.nextafter(obs[below], np.inf), own[below])
    assert not (own[tie] > obs[tie]).any() and (own[below] > obs[below]).all()
    # a last-bit error flips a count at every planted cell, in both directions
    valid = np.ones(obs.shape, dtype=bool)
    base = C.score_with_obs(data, labels, inv, obs, inter, cp, valid)
    up = np.where(below, np.nextafter(obs, np.inf), obs)
    down = np.where(tie, np.nextafter(obs, -np.inf), obs)
    c_up = C.score_with_obs(data, labels, inv, up, inter, cp, valid)
    c_down = C.score_with_obs(data, labels, inv, down, inter, cp, valid)
    assert (c_up[below] < base[below]).all() and (c_up[tie] == base[tie]).all()
    assert (c_down[tie] > base[tie]).all() and (c_down[below] == base[below]).all()
    return obs, tie, below, own


@pytest.mark.parametrize("generator", ["numpy", "philox"])
@pytest.mark.parametrize("k", sorted(C.PLANTED_SHAPES))
def test_planted_cells_are_last_bit_sensitive(k, generator):
    data, cl, inter, cp, inv = C.planted_case(k)
    assert len(cl) >= 4 * k and (np.bincount(cl, minlength=k) > 0).all()
    _, _, _, own = _check_planted(data, _labels(cl, generator), inv, inter, cp)
    assert (own > 0).all()


@pytest.mark.parametrize("n_cp", [255, 256, 257])
def test_score_block_edge_columns_hold_both_kinds(n_cp):
    data, cl, inter, cp, inv = C.edge_case(n_cp)
    assert len(cp) == n_cp and len({tuple(p) for p in cp}) == n_cp
    _, tie, below, own = _check_planted(data, _labels(cl, "numpy")[: C.N_EDGE], inv, inter, cp)
    assert (own > 0).all()
    for col in (254, 255, 256):
        if col < n_cp:
            assert tie[:, col].any() and below[:, col].any(), col


@pytest.mark.parametrize("k", [4, 200])
def test_column_lengths_problem(k):
    data, cl, inter, cp, inv = C.lengths_case(k)
    m = sp.csc_matrix(data)
    np.testing.assert_array_equal(np.diff(m.indptr), C.COLUMN_LENGTHS)
    assert m.has_sorted_indices and data.shape == (300, len(C.COLUMN_LENGTHS)) and (data >= 0).all()
    assert (np.bincount(cl, minlength=k) > 0).all()
    g = len(C.COLUMN_LENGTHS)
    assert [0, g - 1] in inter.tolist() and [g - 1, 0] in inter.tolist()  # the empty gene next to the fullest one
    for gene in C.CELL0_GENES:  # a padded last trip (length not a multiple of 16) in a column that has a value at cell 0
        assert C.COLUMN_LENGTHS[gene] % 16 != 0 and data[0, gene] > 0
    # planted thresholds here may sit on a sum of 0.0 (the empty gene): ties and one-ulp-below cells all the same
    _check_planted(data, _labels(cl, "numpy"), inv, inter, cp)


def test_batched_device_generator_labels_are_the_oracles():
    _, cl, _, _, _ = C.planted_case(257)
    np.testing.assert_array_equal(C.philox_labels(cl, 99, 14, 19), O.ligrec_perm_labels_philox(cl, 99, 14, 19))
    _, cl, _, _, _, _ = C.chunk_case(False)
    np.testing.assert_array_equal(C.philox_labels(cl, 7, C.NPL_CAP - 2, C.NPL_CAP + 2), O.ligrec_perm_labels_philox(cl, 7, C.NPL_CAP - 2, C.NPL_CAP + 2))


def test_score_with_obs_is_the_oracle_loop():
    data, cl, inter, cp, inv = C.edge_case(255)
    pre = O.ligrec_prepare(data, cl, inter, cp, threshold=0.1)
    np.testing.assert_array_equal(inv, pre["inv_counts"])
    labels = _labels(cl, "numpy")[:20]
    want = O.ligrec_score_permutations(data, labels, inv, pre["mean_obs"], inter, cp, pre["valid"])
    np.testing.assert_array_equal(C.score_with_obs(data, labels, inv, pre["obs"], inter, cp, pre["valid"]), want)
    assert want.sum() > 0


def test_chunk_border_plants():
    """narrow chunk case: thresholds on the sums of the last permutation of the first launch chunk, the first of the second
    and the last of the range"""
    data, cl, inter, cp, inv, k = C.chunk_case(False)
    n_perms = C.NPL_CAP + 64 + 37
    labels = O.ligrec_perm_labels_numpy(cl, 3, n_perms)
    perms = [C.NPL_CAP - 1, C.NPL_CAP, n_perms - 1]
    _, _, _, own = _check_planted(data, labels, inv, inter, cp, perms)
    assert (own > 0).all()
