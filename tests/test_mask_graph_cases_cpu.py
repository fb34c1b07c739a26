"""CPU: the cases of tests/mask_graph_cases.py reach every branch of the segment-within-polygon predicate (shown on the host code
alone, from gr/_mask.py's own expressions), and the device path of ``mask_graph`` is bound and never falls back to the host."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import squidpy_amd as sq
from squidpy_amd import _lib
from squidpy_amd.gr._mask import _classify, _flat_rings, _polygons, segments_within
from tests import mask_graph_cases as MC

CAP = 256  # any capacity serves here: the comb is built from it


@pytest.fixture(scope="module")
def solved():
    return {name: (a, b, mask, MC.oracle(a, b, mask)) for name, a, b, mask in MC.cases(CAP)}


def test_case_list_is_what_the_gpu_test_expects(solved):
    names = set(solved)
    assert {"reference", "one_hole", "overlapping_holes", "multipolygon_span", "end_on_vertex", "end_on_edge", "collinear", "zero_length",
            "horizontal_edges", "through_hole", "concave_reenter", "wobbly_300", "comb"} <= names
    assert {f"ring_{n}" for n in (63, 64, 65, 257)} <= names and {f"segments_{n}" for n in (1, 63, 64, 65, 1031)} <= names
    for n in (63, 64, 65, 257):
        assert len(_flat_rings(_polygons(solved[f"ring_{n}"][2]))[0]) == n + 1
    for n in (1, 63, 64, 65, 1031):
        assert len(solved[f"segments_{n}"][0]) == n
    assert len(solved["wobbly_300"][0]) == 2000 and len(_polygons(solved["wobbly_300"][2])[0][0]) == 301


def test_every_branch_is_reached(solved):
    cat = {k: np.concatenate([o[k] for _, _, _, o in solved.values()]) for k in next(iter(solved.values()))[3]}
    touched, cut, within = cat["touched"], cat["cut"], cat["within"]
    assert (~touched & within).any(), "untouched, inside"
    assert (~touched & ~within).any(), "untouched, outside"
    assert (touched & ~cut).any() and not within[touched & ~cut].any(), "touched with an outside end"
    assert (cut & within).any(), "cut, all pieces inside"
    assert (cut & ~within).any(), "cut, an outside piece"
    assert (cut & (cat["n_col"] > 0) & within).any() and (cut & (cat["n_col"] > 0) & ~within).any(), "collinear"
    assert (cut & (cat["n_unique"] < cat["n_param"])).any(), "duplicate parameters removed"
    assert (cut & ((cat["ca"] == 1) | (cat["cb"] == 1))).any(), "class 1 at an end"
    assert (cut & (cat["n_param"] == 2)).any(), "cut without a new parameter (a zero-length segment on or inside the polygon)"


def test_named_cases_hold_what_their_names_say(solved):
    a, b, mask, o = solved["overlapping_holes"]
    polys = _polygons(mask)
    assert _classify(np.array([[5.0, 5.0]]), polys)[0] == 0  # inside both holes: per-ring parity (the total parity would say inside)
    assert not o["within"][0] and not o["within"][1]
    o = solved["multipolygon_span"][3]
    assert o["cut"][0] and not o["within"][0] and o["within"][1] and o["within"][2]
    o = solved["zero_length"][3]
    np.testing.assert_array_equal(o["within"], [True, True, False, False, False, False, False, False])
    np.testing.assert_array_equal(o["ca"], [2, 2, 1, 1, 1, 0, 0, 0])
    o = solved["collinear"][3]
    np.testing.assert_array_equal(o["within"], [False, False, False, False, False, True, False, False, True, True, True])
    assert (o["n_col"][:9] > 0).all() and o["n_col"][10] > 0
    o = solved["through_hole"][3]
    np.testing.assert_array_equal(o["within"], [False, False, True, False])
    o = solved["concave_reenter"][3]
    np.testing.assert_array_equal(o["within"], [False, True, False, True, True, True])
    o = solved["end_on_vertex"][3]
    np.testing.assert_array_equal(o["within"], [True, True, True, False, True, False])
    o = solved["horizontal_edges"][3]
    assert o["within"].any() and (~o["within"]).any() and (o["n_col"] > 0).any()
    o = solved["comb"][3]
    assert int((o["n_param"] > CAP).sum()) == MC.COMB_CROSSING and o["cut"][: MC.COMB_CROSSING].all() and not o["within"][: MC.COMB_CROSSING].any()
    assert o["touched"][3] and not o["cut"][3] and o["within"][4] and not o["touched"][4]
    for name, (_, _, _, o) in solved.items():
        if name != "comb":
            assert o["n_param"].max() <= 64, name  # far below any capacity: only the comb may overflow


def test_host_stats_are_the_oracle_counts(solved):
    for name in ("one_hole", "wobbly_300", "comb"):
        a, b, mask, o = solved[name]
        got, stats = segments_within(a, b, mask, chunk=97, return_stats=True)
        np.testing.assert_array_equal(got, o["within"])
        assert stats == {"touched": int(o["touched"].sum()), "cut": int(o["cut"].sum()), "overflow": 0, "launches": 0}, name


def test_entry_points_are_bound():
    assert "sqgr_segments_within" in _lib.SIGNATURES and "sqgr_mask_info" in _lib.SIGNATURES
    info = _lib.mask_info()  # needs no device
    assert info["param_cap"] >= 64 and 0 < info["pairs_per_launch"] <= 1 << 34


def _table():
    pts, poly = MC.reference_fixture()
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    adata = sq.AnnDataLite(X=np.zeros((len(pts), 2)), obs=pd.DataFrame(index=[str(i) for i in range(len(pts))]), obsm={"spatial": pts})
    adata.obsp["spatial_connectivities"] = sp.csr_matrix((d > 0).astype(np.float64))
    adata.obsp["spatial_distances"] = sp.csr_matrix(d)
    return adata, poly


def test_device_path_raises_without_a_device():
    """A device that is not there — ``device=0`` on a machine without a GPU — is an error, not a silent host result."""
    absent = _lib.device_count()  # 0 without a GPU; with GPUs the first index past them
    adata, poly = _table()
    with pytest.raises(_lib.SqgrError):
        sq.gr.mask_graph(adata, None, poly, copy=True, device=absent)
    with pytest.raises(_lib.SqgrError):
        segments_within(np.zeros((1, 2)), np.ones((1, 2)), poly, device=absent)
    assert sq.gr.mask_graph(adata, None, poly, copy=True)[0].nnz > 0  # the default stays the host path
    with pytest.raises(ValueError, match="device"):
        segments_within(np.zeros((1, 2)), np.ones((1, 2)), poly, device="gpu")
