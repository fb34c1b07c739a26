"""CPU: the host side of ``sq.gr.calculate_niche_cellcharter`` and the inputs of the GPU tests.

- every case of tests/niche_cases.py is admissible: sklearn's smallest margin between the best and the second-best weighted
  log-density over all rows is at least ``MIN_MARGIN``, and the numpy restatement of the device's fit (tests/niche_oracle.py — another
  summation order than sklearn's) returns sklearn's labels, ``n_iter_`` and ``converged_``;
- the initial rows of the front end are sklearn's ``check_random_state(seed).choice``;
- the signature, the post-processing and the library loop against the reference's literal source
  (tests/golden/niche_reference.npz, made by tests/golden/make_niche_golden.py);
- every validation error is raised before the device is touched."""

from __future__ import annotations

import inspect
import json
import os

import numpy as np
import pandas as pd
import pytest

import squidpy_amd as sq
from squidpy_amd import AnnDataLite
from squidpy_amd.gr import _niche

from tests import niche_cases as NC
from tests import niche_oracle as NO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "niche_reference.npz"))
COLUMN = "cellcharter_niche"


@pytest.mark.parametrize("rs", NC.SEEDS)
@pytest.mark.parametrize("name", NC.NAMES)
def test_case_is_admissible_and_restatement_equals_sklearn(name, rs):
    c = NC.CASES[name]
    x = NC.data(name)
    assert x.shape == (c.n, c.d) and x.dtype == np.float64 and np.isfinite(x).all()
    ref = NC.reference(name, rs)
    print(f"{name} rs={rs}: n_iter={ref.n_iter} converged={ref.converged} margin={ref.margin:.3g}")
    assert ref.margin >= NC.MIN_MARGIN, "give the case another seed in tests/niche_cases.py"
    got = NO.fit(x, c.k, _niche.gmm_init_rows(c.n, c.k, rs), NC.REG_COVAR, NC.TOL, c.max_iter)
    assert np.array_equal(got.labels, ref.labels)  # no row left out
    assert got.n_iter == ref.n_iter and got.converged == ref.converged and len(got.lower_bounds) == len(ref.lower_bounds)
    for field in ("weights", "means", "covariances", "lower_bounds"):
        dev, bound = NC.close(getattr(got, field), getattr(ref, field))
        print(f"  {field}: max |delta| = {dev:.3g} (bound {bound:.3g})")
        assert dev <= bound, field
    if name in NC.GEOMETRY_CASES:  # n_iter and converged are not decided by rounding: no step's change lies within 1e-6 of tol
        lb = np.r_[-np.inf, ref.lower_bounds]
        gap = float(np.min(np.abs(np.abs(np.diff(lb)) - NC.TOL)))
        print(f"  min | |lb_i - lb_(i-1)| - tol | = {gap:.3g}")
        assert gap >= 1e-6, "give the case another seed in tests/niche_cases.py"


def test_cases_have_what_they_say():
    x = NC.data("dups")
    assert (x[:40] == x[0]).all() and not (x[40] == x[0]).all()
    assert NC.data("offset1e3").mean() > 900
    for rs in NC.SEEDS:
        ref = NC.reference("maxiter5", rs)
        assert not ref.converged and ref.n_iter == 5
        assert NC.reference("overlap5", rs).n_iter >= 10
        cov = NC.reference("n_eq_k", rs).covariances
        assert np.allclose(cov, np.eye(2) * NC.REG_COVAR, rtol=0, atol=1e-12)
    assert all(NC.reference(n, rs).converged for n in NC.NAMES if n not in ("maxiter5",) + NC.GEOMETRY_CASES for rs in NC.SEEDS)
    sizes = np.bincount(NC.reference("default10", 42).labels, minlength=10)
    assert sizes.max() > 2 * sizes.min() > 0


@pytest.mark.parametrize("seed", [42, 1, 0, 2**31 + 5])
def test_init_rows_are_sklearns(seed):
    from sklearn.utils import check_random_state

    for n, k in ((3, 3), (50, 1), (5250, 10), (8000, 64)):
        want = check_random_state(seed).choice(n, size=k, replace=False)
        got = _niche.gmm_init_rows(n, k, seed)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    state = np.random.RandomState(7)
    assert _niche._check_random_state(state) is state and _niche._check_random_state(None) is np.random.mtrand._rand
    with pytest.raises(ValueError, match="cannot be used to seed"):
        _niche._check_random_state("seven")


def test_signature_matches_reference():
    ref = json.loads(str(GOLD["signature"]))
    params = list(inspect.signature(sq.gr.calculate_niche_cellcharter).parameters.values())
    pos = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == [a["name"] for a in ref["positional"]]
    for p, a in zip(pos, ref["positional"]):
        assert p.default == (inspect.Parameter.empty if a["default"] is None else eval(a["default"])), p.name
    kwonly = {p.name: p for p in params if p.kind == p.KEYWORD_ONLY}
    assert {a["name"] for a in ref["keyword_only"]} | {"device"} == set(kwonly) and kwonly["device"].default is None
    fit = inspect.signature(sq.gmm_fit)
    assert list(fit.parameters) == ["X", "n_components", "random_state", "reg_covar", "tol", "max_iter", "device"]
    assert (fit.parameters["reg_covar"].default, fit.parameters["tol"].default, fit.parameters["max_iter"].default) == (1e-6, 1e-3, 100)
    assert sq.GMMFit._fields == ("weights", "means", "covariances", "lower_bounds", "n_iter", "converged", "labels")


@pytest.mark.parametrize("name", [str(c) for c in GOLD["post_cases"]])
def test_postprocess_equals_literal(name):
    g = lambda k: GOLD[f"post/{name}/{k}"]  # noqa: E731
    obs = pd.DataFrame({COLUMN: pd.Categorical(g("labels"))}, index=g("names"))
    mask = pd.Series(g("mask"), index=g("mask_index")) if len(g("mask")) else None
    min_size = int(g("min_size")) if int(g("min_size")) >= 0 else None
    prefix = str(g("prefix")) or None
    _niche.postprocess_niche_results(obs, [COLUMN], mask, min_size, prefix)
    assert obs[COLUMN].map(type).eq(str).all()
    assert np.array_equal(obs[COLUMN].to_numpy().astype(str), g("expected"))


def test_postprocess_without_options_keeps_the_categorical():
    obs = pd.DataFrame({COLUMN: pd.Categorical([2, 0, 2])})
    _niche.postprocess_niche_results(obs, [COLUMN])
    assert isinstance(obs[COLUMN].dtype, pd.CategoricalDtype) and list(obs[COLUMN]) == [2, 0, 2]


def _given_labels(monkeypatch, labels):
    """The fit replaced by given labels: column 0 of the embedding holds the row's position."""

    def fake(X, n_components, random_state, **kw):
        rows = np.asarray(X)[:, 0].astype(np.int64)
        z = np.zeros(0)
        return _niche.GMMFit(z, z, z, z, 1, True, labels[rows].astype(np.int32))

    monkeypatch.setattr(_niche, "gmm_fit", fake)


def _lib_adata() -> AnnDataLite:
    n = len(GOLD["lib/labels"])
    obs = pd.DataFrame({"library": pd.Categorical(GOLD["lib/library"])}, index=GOLD["lib/names"])
    return AnnDataLite(X=None, obs=obs, obsm={"rep": np.c_[np.arange(n, dtype=np.float64), np.zeros((n, 2))]})


@pytest.mark.parametrize("tag", ["plain", "mask_min"])
def test_library_loop_equals_literal(monkeypatch, tag):
    _given_labels(monkeypatch, GOLD["lib/labels"])
    ad = _lib_adata()
    kw = {} if tag == "plain" else {"mask": pd.Series(GOLD["lib/mask"], index=GOLD["lib/names"]), "min_niche_size": int(GOLD["lib/min_size"])}
    assert sq.gr.calculate_niche_cellcharter(ad, n_components=2, use_rep="rep", library_key="library", **kw) is None
    assert np.array_equal(ad.obs[COLUMN].to_numpy().astype(str), GOLD[f"lib/{tag}/expected"])
    # an existing column is left alone by a library_key call: the reference fills only columns the first library added
    before = ad.obs[COLUMN].copy()
    _given_labels(monkeypatch, (GOLD["lib/labels"] + 1) % 4)
    sq.gr.calculate_niche_cellcharter(ad, n_components=2, use_rep="rep", library_key="library", **kw)
    assert ad.obs[COLUMN].equals(before)


def test_inplace_and_slicing_with_given_labels(monkeypatch):
    labels = GOLD["lib/labels"]
    seen = {}

    def fake(X, n_components, random_state, **kw):
        seen["shape"], seen["rs"], seen["k"] = np.asarray(X).shape, random_state, n_components
        z = np.zeros(0)
        return _niche.GMMFit(z, z, z, z, 1, True, labels.astype(np.int32))

    monkeypatch.setattr(_niche, "gmm_fit", fake)
    ad = _lib_adata()
    out = sq.gr.calculate_niche_cellcharter(ad, n_components=2, use_rep="rep", random_state=5, inplace=False)
    assert COLUMN not in ad.obs and out is not ad and seen == {"shape": (len(labels), 2), "rs": 5, "k": 2}
    want = pd.Categorical(labels)
    assert isinstance(out.obs[COLUMN].dtype, pd.CategoricalDtype) and out.obs[COLUMN].cat.categories.dtype == want.categories.dtype
    assert np.array_equal(out.obs[COLUMN].to_numpy(), labels) and list(out.obs[COLUMN].cat.categories) == list(want.categories)


def test_checks_raise_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_niche, "default_context", boom)
    n = 30
    rng = np.random.default_rng(0)
    obs = pd.DataFrame({"library": pd.Categorical(["a", "b"] * (n // 2))})
    ad = AnnDataLite(X=None, obs=obs, obsm={"rep": rng.normal(size=(n, 4)), "wide": rng.normal(size=(n, 70)), "nan": rng.normal(size=(n, 4))})
    ad.obsm["nan"][3, 1] = np.nan
    with pytest.raises(KeyError, match=r"Key `'nope'` not found in `adata.obsm`. Available keys: \['rep', 'wide', 'nan'\]."):
        sq.gr.calculate_niche_cellcharter(ad, use_rep="nope", n_components=3)
    with pytest.raises(ValueError, match=r"Embedding has 4 components, but n_components=10. Please provide an embedding with at least 10 components."):
        sq.gr.calculate_niche_cellcharter(ad, use_rep="rep")
    with pytest.raises(KeyError, match=r"Key `'batch'` not found in `adata.obs`. Available keys: \['library'\]."):
        sq.gr.calculate_niche_cellcharter(ad, use_rep="rep", n_components=3, library_key="batch")
    with pytest.raises(NotImplementedError, match="use_rep"):
        sq.gr.calculate_niche_cellcharter(ad, n_components=3)
    with pytest.raises(NotImplementedError, match="at most 64 features, 64 components"):
        sq.gr.calculate_niche_cellcharter(ad, use_rep="wide", n_components=65)
    with pytest.raises(NotImplementedError, match="at most 64 features"):
        sq.gmm_fit(ad.obsm["wide"], 3, 0)
    for kw in ({}, {"library_key": "library"}):
        with pytest.raises(ValueError, match="contains NaN or infinity"):
            sq.gr.calculate_niche_cellcharter(ad, use_rep="nan", n_components=3, **kw)
    with pytest.raises(ValueError, match="contains NaN or infinity"):
        sq.gmm_fit(np.array([[0.0], [np.inf], [1.0]]), 1, 0)
    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 4, n_samples = 3"):
        sq.gmm_fit(np.zeros((3, 4)), 4, 0)
    assert COLUMN not in ad.obs
    with pytest.raises(AssertionError, match="the device was touched"):
        sq.gr.calculate_niche_cellcharter(ad, use_rep="rep", n_components=3)
