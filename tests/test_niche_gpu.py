"""GPU: ``squidpy_amd.gmm_fit`` and ``sq.gr.calculate_niche_cellcharter`` against sklearn's ``GaussianMixture`` on the same machine.

Every case of tests/niche_cases.py with both seeds: labels, ``n_iter``, ``converged`` and the number of lower bounds ``==`` sklearn's;
weights, means, covariances and lower bounds within ``1e-9 * max(1, max |reference|)`` (tests/niche_cases.py ``close``: rounding order is
<= 3e-12 here, <= 2.0e-10 in the two launch-geometry cases ``cap_rows`` / ``cap_cov_k64``; the smallest real error >= 1e-6).  tests/test_niche_cpu.py shows that no row of any case sits closer than 1e-6 to a
label boundary, so no row is left out.  Then: repeatability byte for byte, allocator calls that do not grow with the number of
steps, and the front end on ``AnnDataLite`` end to end."""

from __future__ import annotations

import functools
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import squidpy_amd as sq
from squidpy_amd import AnnDataLite, _lib
from squidpy_amd.gr import _niche

from tests import niche_cases as NC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "niche_reference.npz"))
COLUMN = "cellcharter_niche"
FIELDS = ("weights", "means", "covariances", "lower_bounds")


def fit(name: str, rs: int, max_iter: int | None = None) -> sq.GMMFit:
    c = NC.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return sq.gmm_fit(NC.data(name), c.k, rs, max_iter=c.max_iter if max_iter is None else max_iter)


@functools.lru_cache(maxsize=None)
def device_fit(name: str, rs: int) -> sq.GMMFit:
    return fit(name, rs)


def same_bytes(a: sq.GMMFit, b: sq.GMMFit) -> bool:
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("rs", NC.SEEDS)
@pytest.mark.parametrize("name", NC.NAMES)
def test_fit_equals_sklearn(name, rs):
    c = NC.CASES[name]
    ref, got = NC.reference(name, rs), device_fit(name, rs)
    mismatches = int((got.labels != ref.labels).sum())
    print(f"{name} rs={rs}: n_iter {got.n_iter} / {ref.n_iter}, converged {got.converged} / {ref.converged}, label mismatches {mismatches} of {c.n}")
    figures = {f: NC.close(getattr(got, f), getattr(ref, f)) for f in FIELDS if len(getattr(got, f)) == len(getattr(ref, f))}
    for f, (dev, bound) in figures.items():
        print(f"  {f}: max |delta| = {dev:.3g} (bound {bound:.3g})")
    assert got.labels.dtype == np.int32 and got.labels.shape == (c.n,)
    assert got.weights.shape == (c.k,) and got.means.shape == (c.k, c.d) and got.covariances.shape == (c.k, c.d, c.d)
    assert got.n_iter == ref.n_iter and got.converged == ref.converged and len(got.lower_bounds) == len(ref.lower_bounds)
    assert mismatches == 0
    for f in FIELDS:
        dev, bound = figures[f]
        assert dev <= bound, f


@pytest.mark.parametrize("name,other", [("d17k6", "default10"), ("dups", "d2k2"), ("d32k32", "k1d1")])
def test_repeats_byte_for_byte(name, other):
    """Two identical calls, and the same call again after a fit of another shape on the same context: no stale buffer."""
    first = device_fit(name, 42)
    assert same_bytes(first, fit(name, 42))
    fit(other, 1)
    assert same_bytes(first, fit(name, 42))


def test_allocator_calls_do_not_grow_with_steps():
    ctx = _lib.default_context()
    fit("default10", 42, max_iter=5)  # whatever the first call of a shape parks or frees is behind us
    deltas = []
    for max_iter in (5, 100):
        before = ctx.alloc_counters()
        got = fit("default10", 42, max_iter=max_iter)
        after = ctx.alloc_counters()
        deltas.append({k: after[k] - before[k] for k in ("mallocs", "malloc_bytes", "frees", "pool_hits", "pool_parks")})
        print(max_iter, got.n_iter, deltas[-1])
        assert got.n_iter == (5 if max_iter == 5 else NC.reference("default10", 42).n_iter)
    assert deltas[0] == deltas[1]
    assert deltas[0]["mallocs"] + deltas[0]["pool_hits"] <= 8


def test_not_converged_warns_and_returns_sklearns_labels():
    c = NC.CASES["maxiter5"]
    with pytest.warns(UserWarning, match="Best performing initialization did not converge. Try different init parameters"):
        got = sq.gmm_fit(NC.data("maxiter5"), c.k, 42, max_iter=c.max_iter)
    assert not got.converged and got.n_iter == 5 and np.array_equal(got.labels, NC.reference("maxiter5", 42).labels)


def test_ill_defined_covariance_raises_sklearns_error():
    """A column of zeros and no regularisation: that column's variance is exactly 0 in every component, the second pivot of the
    factorisation is not positive — sklearn's ValueError (it raises it on this input too), from the device's pivot flag."""
    x = np.c_[NC.data("d1k3"), np.zeros(len(NC.data("d1k3")))]
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        sq.gmm_fit(x, 3, 42, reg_covar=0.0)
    assert same_bytes(device_fit("d1k3", 42), fit("d1k3", 42))  # the context is as good as before


def _adata(rep: np.ndarray, **obs) -> AnnDataLite:
    return AnnDataLite(X=None, obs=pd.DataFrame(obs, index=[str(i) for i in range(len(rep))]), obsm={"X_rep": rep})


def _same_categorical(col: pd.Series, labels: np.ndarray) -> None:
    want = pd.Categorical(labels)
    assert isinstance(col.dtype, pd.CategoricalDtype)
    assert np.array_equal(col.to_numpy(), np.asarray(want)) and col.cat.categories.equals(want.categories)


def test_front_end_default_call():
    ref = NC.reference("default10", 42)
    ad = _adata(NC.data("default10"))
    assert sq.gr.calculate_niche_cellcharter(ad, use_rep="X_rep") is None
    _same_categorical(ad.obs[COLUMN], ref.labels)


def test_front_end_uses_the_first_columns_only_and_copies():
    x = NC.data("default10")
    wide = np.c_[x, np.random.default_rng(3).normal(size=(len(x), 3)) * 50]
    ad = _adata(wide)
    out = sq.gr.calculate_niche_cellcharter(ad, use_rep="X_rep", inplace=False)
    assert COLUMN not in ad.obs and out is not ad and np.array_equal(ad.obsm["X_rep"], wide)
    _same_categorical(out.obs[COLUMN], NC.reference("default10", 42).labels)


def test_front_end_float32_is_fitted_in_float64():
    x32 = NC.data("overlap5").astype(np.float32)
    ref = NC.sklearn_fit(x32.astype(np.float64), 5, 1)
    assert ref.margin >= NC.MIN_MARGIN
    ad = _adata(x32)
    sq.gr.calculate_niche_cellcharter(ad, use_rep="X_rep", n_components=5, random_state=1)
    _same_categorical(ad.obs[COLUMN], ref.labels)


def test_front_end_libraries():
    """Two libraries of different sizes in interleaved order: each is its own sklearn fit, prefixed ``lib={id}_``."""
    x = NC.data("overlap5")
    lib = np.where(np.random.default_rng(4).random(len(x)) < 0.35, "B", "A")
    ad = _adata(x, sample=pd.Categorical(lib))
    sq.gr.calculate_niche_cellcharter(ad, use_rep="X_rep", n_components=5, library_key="sample")
    col = ad.obs[COLUMN]
    assert (lib == "A").sum() != (lib == "B").sum() and col.map(type).eq(str).all()
    for lib_id in ("A", "B"):
        rows = lib == lib_id
        ref = NC.sklearn_fit(x[rows], 5, 42)
        assert ref.margin >= NC.MIN_MARGIN
        assert np.array_equal(col.to_numpy()[rows].astype(str), np.array([f"lib={lib_id}_{v}" for v in ref.labels]))


def test_front_end_mask_and_min_niche_size():
    ad = _adata(NC.data("default10"))
    mask = pd.Series(GOLD["e2e/mask"], index=ad.obs.index)
    sq.gr.calculate_niche_cellcharter(ad, use_rep="X_rep", mask=mask, min_niche_size=int(GOLD["e2e/min_size"]))
    assert np.array_equal(ad.obs[COLUMN].to_numpy().astype(str), GOLD["e2e/expected"])
    assert (GOLD["e2e/expected"] == _niche.NOT_A_NICHE).sum() > (~GOLD["e2e/mask"]).sum()  # the size rule relabelled rows of its own
