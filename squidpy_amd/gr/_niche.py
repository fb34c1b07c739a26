"""``sq.gr.calculate_niche_cellcharter`` (gr/_niche.py:402-462) and the Gaussian mixture behind it, fitted on the GPU.

The reference ends in ``sklearn.mixture.GaussianMixture(n_components, random_state, init_params="random_from_data")`` followed by
``.fit(embedding).predict(embedding)`` (gr/_niche.py:1474-1480).  ``gmm_fit`` is that fit: the host draws the initial rows from
numpy's ``RandomState`` exactly as sklearn's ``check_random_state(random_state).choice`` does, everything else runs in
``csrc/sqgr_gmm.hip`` (``sqgr_gmm_fit``).  Neither this module nor the library imports sklearn."""

from __future__ import annotations

import numbers
import warnings
from typing import Any, NamedTuple

import numpy as np
import pandas as pd

from .._lib import SqgrError, default_context
from .._lib import gmm_fit as _gmm_fit
from .._utils import extract_adata_if_sdata, logg

__all__ = ["calculate_niche_cellcharter", "gmm_fit", "gmm_init_rows", "GMMFit", "GMM_MAX_FEATURES", "GMM_MAX_COMPONENTS"]

GMM_MAX_FEATURES = 64    # GMM_MAX of csrc/sqgr_gmm.hip
GMM_MAX_COMPONENTS = 64
NOT_A_NICHE = "not_a_niche"
NICHE_COLUMN = "cellcharter_niche"

# sklearn/mixture/_gaussian_mixture.py (_compute_precision_cholesky) and _base.py (fit_predict): the sentences of the reference's clusterer
ILL_DEFINED_MSG = (
    "Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by singleton "
    "or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data."
)
NOT_CONVERGED_MSG = (
    "Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check for degenerate data."
)


class GMMFit(NamedTuple):
    """What ``gmm_fit`` returns: sklearn's ``weights_``, ``means_``, ``covariances_``, ``lower_bounds_``, ``n_iter_``, ``converged_`` and
    ``predict(X)``."""

    weights: np.ndarray
    means: np.ndarray
    covariances: np.ndarray
    lower_bounds: np.ndarray
    n_iter: int
    converged: bool
    labels: np.ndarray


def _check_random_state(seed: Any) -> np.random.RandomState:
    """sklearn.utils.check_random_state."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def gmm_init_rows(n: int, n_components: int, random_state: Any) -> np.ndarray:
    """The rows sklearn's ``init_params="random_from_data"`` starts the components from (mixture/_base.py, _initialize_parameters)."""
    return _check_random_state(random_state).choice(int(n), size=int(n_components), replace=False).astype(np.int64)


def _validated_matrix(X: Any, n_components: int, check_rows: bool = True) -> np.ndarray:
    """``X`` as a C-contiguous float64 matrix the kernels accept; every refusal is raised here, on the host.  ``check_rows=False``
    leaves ``n_samples >= n_components`` to the fits of the parts the matrix is about to be cut into."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected a 2-D array, found shape `{X.shape}`.")
    n, d = X.shape
    k = int(n_components)
    if k < 1:
        raise ValueError(f"Expected `n_components` to be positive, found `{n_components}`.")
    if d < 1:
        raise ValueError(f"Found array with {d} feature(s) (shape={X.shape}) while a minimum of 1 is required.")
    if d > GMM_MAX_FEATURES or k > GMM_MAX_COMPONENTS or n >= 2**31:
        raise NotImplementedError(
            f"The Gaussian mixture kernels support at most {GMM_MAX_FEATURES} features, {GMM_MAX_COMPONENTS} components and 2**31 - 1 rows; "
            f"found {d} features, {k} components and {n} rows."
        )
    if check_rows and n < k:
        raise ValueError(f"Expected n_samples >= n_components but got n_components = {k}, n_samples = {n}")
    X = np.ascontiguousarray(X, dtype=np.float64)  # float32 is widened: the fit is float64 throughout
    if not np.isfinite(X).all():
        raise ValueError("Input X contains NaN or infinity.")
    return X


def gmm_fit(
    X: Any,
    n_components: int,
    random_state: Any,
    *,
    reg_covar: float = 1e-6,
    tol: float = 1e-3,
    max_iter: int = 100,
    device: int | None = None,
) -> GMMFit:
    """``GaussianMixture(n_components, random_state=random_state, init_params="random_from_data", reg_covar=reg_covar, tol=tol,
    max_iter=max_iter).fit(X)`` and ``.predict(X)`` on the GPU, in float64 (a float32 ``X`` is widened first; sklearn would keep it
    float32).  At most 64 features and 64 components.  Two calls with the same arguments return the same bytes.
    Warns with sklearn's sentence (as a ``UserWarning``) when ``max_iter`` steps did not converge; raises sklearn's ``ValueError`` when
    a covariance is not positive definite."""
    X = _validated_matrix(X, n_components)
    if max_iter < 1:
        raise ValueError(f"Expected `max_iter` to be positive, found `{max_iter}`.")
    if reg_covar < 0 or tol < 0:
        raise ValueError(f"Expected `reg_covar` and `tol` to be non-negative, found `{reg_covar}` and `{tol}`.")
    init_rows = gmm_init_rows(X.shape[0], n_components, random_state)
    ctx = default_context(device)
    try:
        out = _gmm_fit(ctx, X, int(n_components), init_rows, reg_covar, tol, max_iter)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        if exc.status == -1 and "ill-defined" in str(exc):
            raise ValueError(ILL_DEFINED_MSG) from None
        raise
    fit = GMMFit(*out)
    if not fit.converged:
        warnings.warn(NOT_CONVERGED_MSG, UserWarning, stacklevel=2)
    return fit


def _assert_key_in_adata(adata: Any, key: str, attr: str) -> None:
    """_validators.py:99-112."""
    container = getattr(adata, attr)
    if key not in container:
        available = list(container.keys()) if hasattr(container, "keys") else list(container)
        raise KeyError(f"Key `{key!r}` not found in `adata.{attr}`. Available keys: {available}.")


def postprocess_niche_results(
    obs: pd.DataFrame, result_columns: list[str], mask: pd.Series | None = None, min_niche_size: int | None = None, prefix: str | None = None
) -> None:
    """``_postprocess_niche_results`` (gr/_niche.py:1494-1542) on the ``obs`` frame, quirks included: the labels become ``str``; the
    mask is cut to the frame's index but not reordered; ``min_niche_size`` also counts (and can relabel) ``"not_a_niche"``; the
    prefix goes in front of ``"not_a_niche"`` as well."""
    if mask is None and min_niche_size is None and prefix is None:
        return
    for col in result_columns:
        labels = obs[col].astype(str)
        if mask is not None:
            aligned = mask[mask.index.isin(obs.index)]
            labels[~aligned] = NOT_A_NICHE
        if min_niche_size is not None:
            counts = labels.value_counts()
            too_small = counts[counts < min_niche_size].index
            labels[labels.isin(too_small)] = NOT_A_NICHE
        if prefix is not None:
            labels = prefix + labels
        obs[col] = labels


def _cluster(obs: pd.DataFrame, embedding: np.ndarray, n_components: int, random_state: Any, device: int | None) -> list[str]:
    """``_GMMClusterer.cluster`` (gr/_niche.py:1469-1486)."""
    fit = gmm_fit(embedding, n_components, random_state, device=device)
    if NICHE_COLUMN in obs.columns:
        logg.info("Overwriting existing column '%s'", NICHE_COLUMN)
    obs[NICHE_COLUMN] = pd.Categorical(fit.labels.astype(np.int64))
    return [NICHE_COLUMN]


def calculate_niche_cellcharter(
    data: Any,
    distance: int = 3,
    aggregation: str = "mean",
    random_state: int = 42,
    spatial_connectivities_key: str = "spatial_connectivities",
    n_components: int = 10,
    use_rep: str | None = None,
    min_niche_size: int | None = None,
    mask: pd.Series | None = None,
    library_key: str | None = None,
    inplace: bool = True,
    table_key: str | None = None,
    *,
    device: int | None = None,
) -> Any:
    """Compute niche assignments with the cellcharter flavour (drop-in for ``squidpy.gr.calculate_niche_cellcharter``,
    gr/_niche.py:402-462): a Gaussian mixture of ``n_components`` components on ``adata.obsm[use_rep][:, :n_components]``, fitted by EM
    on the GPU in float64 (``csrc/sqgr_gmm.hip``) the way sklearn 1.7's ``GaussianMixture(n_components, random_state=random_state,
    init_params="random_from_data")`` fits it; ``obs["cellcharter_niche"]`` gets ``pd.Categorical(labels)``.

    As in the reference, the same ``n_components`` is the number of columns taken and the number of mixture components, and
    ``distance``, ``aggregation`` and ``spatial_connectivities_key`` are not used when ``use_rep`` is given.  ``mask``,
    ``min_niche_size`` and ``library_key`` follow ``_postprocess_niche_results`` and ``_calculate_niche_custom``: labels become ``str``,
    masked or too-small niches become ``"not_a_niche"``; with ``library_key`` every library is fitted on its own, in
    ``obs[library_key].unique()`` order, and its labels are prefixed ``lib={id}_``; an ``obs["cellcharter_niche"]`` that exists
    before a ``library_key`` call is left as it is (the reference only fills columns the first library added).

    Two deliberate limits:

    - ``use_rep=None`` raises ``NotImplementedError``.  That path aggregates ``adata.X`` over hop shells and runs scanpy's PCA in
      front of the mixture; the reference itself warns that it is a proxy, and the PCA cannot be pinned here.
    - A float32 representation is converted to float64 and fitted in float64; sklearn would keep float32.  The result is pinned to
      sklearn on ``X.astype(np.float64)``.

    At most 64 components (``NotImplementedError`` beyond).  A fit that does not converge within 100 steps warns with sklearn's
    sentence (``UserWarning``); a covariance that is not positive definite raises sklearn's ``ValueError``.  Under a process group
    every rank computes the whole result.

    Returns ``None`` if ``inplace=True``, else a copy of ``adata`` with the column added."""
    orig_adata = extract_adata_if_sdata(data, table_key=table_key)
    # every refusal first: nothing has touched the device or the caller's object when one is raised
    if use_rep is None:
        raise NotImplementedError(
            "calculate_niche_cellcharter needs `use_rep` here: the reference's `use_rep=None` path (hop-shell aggregation of `adata.X` and "
            "scanpy's PCA in front of the mixture) is not implemented."
        )
    _assert_key_in_adata(orig_adata, use_rep, "obsm")
    embedding = np.asarray(orig_adata.obsm[use_rep])
    if embedding.shape[1] < n_components:
        raise ValueError(
            f"Embedding has {embedding.shape[1]} components, but n_components={n_components}. "
            f"Please provide an embedding with at least {n_components} components."
        )
    if library_key is not None:
        _assert_key_in_adata(orig_adata, library_key, "obs")
    embedding = _validated_matrix(embedding[:, :n_components], n_components, check_rows=library_key is None)

    adata = orig_adata if inplace else orig_adata.copy()
    if library_key is not None:
        logg.info("Stratifying by library_key '%s'", library_key)
        for itr, lib_id in enumerate(adata.obs[library_key].unique()):
            rows = (adata.obs[library_key] == lib_id).to_numpy()
            lib_indices = adata.obs[rows].index
            if len(lib_indices) == 0:
                logg.warning("Library '%s' contains no cells, skipping", lib_id)
                continue
            lib_obs = adata.obs[rows].copy()
            result_columns = _cluster(lib_obs, embedding[rows], n_components, random_state, device)
            postprocess_niche_results(lib_obs, result_columns, mask, min_niche_size, f"lib={lib_id}_")
            if itr == 0:  # the reference's rule: only columns the first library added are filled
                added_columns = list(set(lib_obs.columns) - set(adata.obs.columns))
            for col in added_columns:
                if col not in adata.obs:
                    adata.obs[col] = NOT_A_NICHE
                adata.obs.loc[lib_indices, col] = list(lib_obs[col].astype("str"))
    else:
        result_columns = _cluster(adata.obs, embedding, n_components, random_state, device)
        postprocess_niche_results(adata.obs, result_columns, mask, min_niche_size, None)
    return None if inplace else adata
