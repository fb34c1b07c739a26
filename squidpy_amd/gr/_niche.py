"""``sq.gr.calculate_niche_cellcharter`` (gr/_niche.py:402-462) and the Gaussian mixture behind it, fitted on the GPU.

The reference ends in ``sklearn.mixture.GaussianMixture(n_components, random_state, init_params="random_from_data")`` followed by
``.fit(embedding).predict(embedding)`` (gr/_niche.py:1474-1480).  ``gmm_fit`` is that fit: the host draws the initial rows from
numpy's ``RandomState`` exactly as sklearn's ``check_random_state(random_state).choice`` does, everything else runs in
``csrc/sqgr_gmm.hip`` (``sqgr_gmm_fit``).  Neither this module nor the library imports sklearn.

``niche_nhood_profile``, ``niche_utag_features`` and ``niche_cellcharter_features`` are stage 1 of the reference's three niche flavours:
the feature matrix each of them computes from the spatial graph and hands to scanpy (``csrc/sqgr_niche.hip``).  ``niche_pca`` is
scanpy's default ``sc.tl.pca`` on such a matrix — sklearn's ``PCA(svd_solver="arpack")`` — with the means, the scatter matrix and the
projection on the GPU (``csrc/sqgr_pca.hip``) and the D x D eigenproblem on the host; ``niche_utag_embedding`` and
``niche_cellcharter_embedding`` run it on feature blocks that never leave the device."""

from __future__ import annotations

import numbers
import warnings
from typing import Any, NamedTuple

import numpy as np
import pandas as pd

from .._lib import DeviceMatrix, DevicePCA, HopShells, SqgrError, cached_graph, default_context, niche_aggregate, niche_label_hops
from .._lib import gmm_fit as _gmm_fit
from .._utils import extract_adata_if_sdata, logg

__all__ = ["calculate_niche_cellcharter", "gmm_fit", "gmm_init_rows", "GMMFit", "GMM_MAX_FEATURES", "GMM_MAX_COMPONENTS",
           "niche_nhood_profile", "niche_utag_features", "niche_cellcharter_features", "hop_shells", "niche_pca", "PCAResult",
           "niche_utag_embedding", "niche_cellcharter_embedding", "pca_n_comps", "pca_components", "PCA_MAX_FEATURES",
           "PCA_MAX_COMPONENTS"]

GMM_MAX_FEATURES = 64    # GMM_MAX of csrc/sqgr_gmm.hip
GMM_MAX_COMPONENTS = 64
PCA_MAX_FEATURES = 4096  # PCA_MAX_D of csrc/sqgr_pca.hip
PCA_MAX_COMPONENTS = 64  # PCA_MAX_C
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
    **options: Any,
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

    - ``use_rep=None`` raises ``NotImplementedError`` unless ``proxy_pca=True`` is passed — by keyword only, default ``False``; it is
      the one option ``**options`` accepts (the named parameters are pinned to the reference's signature plus ``device``, so the
      switch is not one of them; any other keyword is a ``TypeError``).  That path (gr/_niche.py:1332-1359) logs
      the reference's warning that PCA is only a proxy, aggregates ``adata.X`` over ``distance`` hop shells
      (``niche_cellcharter_features``), runs the default PCA on the result (``niche_pca``: 50 components, or ``min(n, D) - 1``) and fits
      the mixture on ALL columns of that embedding — ``n_components`` is then the number of mixture components only.  Everything up
      to the embedding stays on the device.  The PCA is float64 where scanpy rounds ``X_pca`` to float32 by default: the path is
      pinned to the reference's features, sklearn's ``PCA(svd_solver="arpack")`` and ``GaussianMixture`` in float64.  With
      ``library_key`` every library runs on its own rows of ``X`` and its own sub-graph ``adj[rows][:, rows]`` (the reference's
      ``adata[lib_indices].copy()``).  ``proxy_pca=True`` together with a ``use_rep`` is a ``ValueError``.
    - A float32 representation is converted to float64 and fitted in float64; sklearn would keep float32.  The result is pinned to
      sklearn on ``X.astype(np.float64)``.

    At most 64 components (``NotImplementedError`` beyond).  A fit that does not converge within 100 steps warns with sklearn's
    sentence (``UserWarning``); a covariance that is not positive definite raises sklearn's ``ValueError``.  Under a process group
    every rank computes the whole result.

    Returns ``None`` if ``inplace=True``, else a copy of ``adata`` with the column added."""
    orig_adata = extract_adata_if_sdata(data, table_key=table_key)
    proxy_pca = bool(options.pop("proxy_pca", False))
    if options:
        raise TypeError(f"calculate_niche_cellcharter() got an unexpected keyword argument {next(iter(options))!r}")
    # every refusal first: nothing has touched the device or the caller's object when one is raised
    if proxy_pca and use_rep is not None:
        raise ValueError("`proxy_pca=True` runs the `use_rep=None` path; found `use_rep={!r}`.".format(use_rep))
    if use_rep is None and not proxy_pca:
        raise NotImplementedError(
            "calculate_niche_cellcharter needs `use_rep` here: the reference's `use_rep=None` path (hop-shell aggregation of `adata.X` and "
            "scanpy's PCA in front of the mixture) is not implemented."
        )
    if use_rep is None:
        if library_key is not None:
            _assert_key_in_adata(orig_adata, library_key, "obs")
        distance = _check_distance(distance)
        _check_aggregation(aggregation)
        adj = _unit_graph(orig_adata, spatial_connectivities_key)
        X = _feature_matrix(orig_adata)
        if library_key is None:
            _check_pca_shape(orig_adata.n_obs, (distance + 1) * X.shape[1], None)

        def embed(rows: np.ndarray | None) -> np.ndarray:
            logg.warning(PROXY_PCA_MSG)
            if rows is None:
                return _cellcharter_pca(adj, X, distance, aggregation, None, device).X_pca
            sub = adj[rows][:, rows]
            sub.sort_indices()
            return _cellcharter_pca(sub, X[rows], distance, aggregation, None, device).X_pca
    else:
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

        def embed(rows: np.ndarray | None) -> np.ndarray:
            return embedding if rows is None else embedding[rows]

    def cluster(adata: Any, obs: pd.DataFrame, rows: np.ndarray | None) -> list[str]:
        return _cluster(obs, embed(rows), n_components, random_state, device)

    return calculate_niche_custom(orig_adata, cluster, min_niche_size, mask, library_key, inplace)


def calculate_niche_custom(orig_adata: Any, cluster: Any, min_niche_size: int | None, mask: pd.Series | None, library_key: str | None,
                           inplace: bool, prefix: str | None = None) -> Any:
    """The frame of ``_calculate_niche_custom`` (gr/_niche.py:200-271) every flavour shares.  ``cluster(adata, obs, rows)`` computes the
    niche columns of the observations ``rows`` (a boolean mask over ``adata``, ``None`` for all), writes them into ``obs`` and returns
    their names.  With ``library_key`` every library is clustered on its own, in ``obs[library_key].unique()`` order, and its labels
    are prefixed ``lib={id}_``; only columns the first library added are filled (the reference's rule).  ``prefix`` (the spatialleiden
    flavour's) goes in front of the labels where there is no ``library_key``, as in gr/_niche.py:571 and :610."""
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
            result_columns = cluster(adata, lib_obs, rows)
            postprocess_niche_results(lib_obs, result_columns, mask, min_niche_size, f"lib={lib_id}_")
            if itr == 0:  # the reference's rule: only columns the first library added are filled
                added_columns = list(set(lib_obs.columns) - set(adata.obs.columns))
            for col in added_columns:
                if col not in adata.obs:
                    adata.obs[col] = NOT_A_NICHE
                adata.obs.loc[lib_indices, col] = list(lib_obs[col].astype("str"))
    else:
        result_columns = cluster(adata, adata.obs, None)
        postprocess_niche_results(adata.obs, result_columns, mask, min_niche_size, prefix)
    return None if inplace else adata


# ---- stage 1 of the three niche flavours: the feature matrix each of them hands to scanpy ----------------------------------------------
NOT_CATEGORICAL_MSG = "Since adata.obs[groups] does not already have categorical dtype, converting it into categorical type."
MAX_DISTANCE = 64  # MAX_DISTANCE of csrc/sqgr_niche.hip


def _canonical_graph(adata: Any, key: str) -> Any:
    """``adata.obsp[key]`` as a square scipy CSR matrix in canonical form (rows ascending, no repeated entry): the kernels sum a row in
    ascending column order.  The caller's matrix is never changed."""
    from scipy import sparse

    _assert_key_in_adata(adata, key, "obsp")
    adj = adata.obsp[key]
    adj = adj if sparse.isspmatrix_csr(adj) else sparse.csr_matrix(adj)
    if adj.shape[0] != adj.shape[1] or adj.shape[0] != adata.n_obs:
        raise ValueError(f"Expected `adata.obsp[{key!r}]` of shape `{(adata.n_obs, adata.n_obs)}`, found `{adj.shape}`.")
    if not adj.has_canonical_format:
        adj = adj.copy()
        adj.sum_duplicates()
    if adj.dtype not in (np.float32, np.float64):
        adj = adj.astype(np.float64)
    return adj


def _check_distance(distance: Any) -> int:
    if isinstance(distance, bool) or not isinstance(distance, numbers.Integral):
        raise TypeError(f"Expected `distance` to be of type `int`, found `{type(distance).__name__}`.")
    if distance < 1:
        raise ValueError(f"'distance' must be at least 1, got {distance}")
    if distance > MAX_DISTANCE:
        raise NotImplementedError(f"The niche kernels support a `distance` of at most {MAX_DISTANCE}, found {distance}.")
    return int(distance)


def _feature_matrix(adata: Any) -> Any:
    """``adata.X`` as the kernels take it: scipy CSR / CSC or a 2-D array, finite."""
    from scipy import sparse

    X = adata.X
    if X is None:
        raise ValueError("`adata.X` is `None`.")
    if not sparse.issparse(X):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"Expected `adata.X` to be 2-D, found shape `{X.shape}`.")
    if X.shape[0] != adata.n_obs:
        raise ValueError(f"Expected `adata.X` to have {adata.n_obs} rows, found {X.shape[0]}.")
    values = X.data if sparse.issparse(X) else X
    if values.dtype.kind not in "fiub":
        raise TypeError(f"Expected a numeric `adata.X`, found dtype `{values.dtype}`.")
    if values.dtype.kind == "f" and not np.isfinite(values).all():
        raise ValueError("`adata.X` contains NaN or infinity.")
    return X


def hop_weights(n_hop_weights: Any, distance: int) -> list[float] | None:
    """The hop weights of ``_NhoodProfileEmbedder.get_embedding`` (gr/_niche.py:1185-1192): ``None`` -> ones, a short list is extended
    with its last value (a new list: the caller's is not touched), a long one is kept whole — its surplus entries still count in
    ``sum(weights)``, as in the reference."""
    if distance == 1:
        return None  # (the reference does not look at the weights)
    if n_hop_weights is None:
        return [1.0] * distance
    if not isinstance(n_hop_weights, list):
        raise TypeError(f"Expected `n_hop_weights` to be of type `list`, found `{type(n_hop_weights).__name__}`.")
    if len(n_hop_weights) == 0:
        raise ValueError("Expected `n_hop_weights` to hold at least one weight.")
    weights = [float(w) for w in n_hop_weights]
    if not np.isfinite(weights).all():
        raise ValueError(f"Expected finite `n_hop_weights`, found `{n_hop_weights}`.")
    if len(weights) < distance:
        weights = weights + [weights[-1]] * (distance - len(weights))
    return weights


def combine_hop_profiles(hops: np.ndarray, weights: list[float] | None, abs_nhood: bool) -> np.ndarray:
    """gr/_niche.py:1194-1214 on the hop profiles ``hops[h - 1]``: ``w0 * P1``, ``+= w_h * P_(h+1)`` hop by hop, then ``/ sum(weights)``
    unless ``abs_nhood`` — numpy's elementwise operations in the reference's order.  One hop is returned as it is."""
    if hops.shape[0] == 1:
        return np.ascontiguousarray(hops[0])
    profile = weights[0] * hops[0]
    for h in range(1, hops.shape[0]):
        profile += weights[h] * hops[h]
    if not abs_nhood:
        profile = profile / sum(weights)
    return np.ascontiguousarray(profile)


def niche_nhood_profile(
    adata: Any,
    groups: str,
    spatial_connectivities_key: str = "spatial_connectivities",
    distance: int = 1,
    abs_nhood: bool = False,
    n_hop_weights: list[float] | None = None,
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> np.ndarray:
    """The neighbourhood profile of the reference's ``neighborhood`` flavour: ``_NhoodProfileEmbedder.get_embedding`` with
    ``scale=False`` (gr/_niche.py:1171-1221), an ``(n_obs, n_categories)`` C-contiguous float64 array with rows in ``adata.obs`` order
    and columns in ``adata.obs[groups].cat.categories`` order (empty categories included).

    Hop ``h`` (1 .. ``distance``) is ``A^h @ onehot(groups)`` with the graph's weights, computed on the GPU as ``A @ (A^(h-1) @ onehot)``
    (the reference forms the sparse power ``A^h``).  With ``abs_nhood=False`` every hop's rows are divided by their sum (0/0 -> 0).
    The hops are combined as ``w0 * P1 + w1 * P2 + ...`` and divided by ``sum(weights)`` unless ``abs_nhood``; ``n_hop_weights``
    shorter than ``distance`` is extended with its last value (the list itself is not changed); any finite weights are accepted.
    A column that is not categorical is converted for the call with the reference's warning; nothing is written into ``adata``.

    Float64 throughout (float32 graph weights are widened exactly); every row sum runs in ascending column order with separately
    rounded products and sums, so two calls return the same bytes.  The result is pinned to the reference run on a float64 graph: equal
    on graphs of unit weights, within rounding of the reference's other summation order otherwise.

    The reference's next step is ``sc.pp.scale(..., zero_center=True)`` (when ``scale=True``), then ``sc.pp.neighbors(use_rep="X")`` and
    ``sc.tl.leiden``.  Under a process group every rank computes the whole result."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    # every refusal first: nothing has touched the device when one is raised
    if not isinstance(groups, str):
        raise TypeError(f"Expected `groups` to be of type `str`, found `{type(groups).__name__}`.")
    _assert_key_in_adata(adata, groups, "obs")
    distance = _check_distance(distance)
    weights = hop_weights(n_hop_weights, distance)
    adj = _canonical_graph(adata, spatial_connectivities_key)
    column = adata.obs[groups]
    if column.dtype.name != "category":
        warnings.warn(NOT_CATEGORICAL_MSG, stacklevel=2)
        column = column.astype("category")  # a copy: `adata.obs` keeps its column
    n_categories = len(column.cat.categories)
    n = adata.n_obs
    if n == 0 or n_categories == 0:
        return np.zeros((n, n_categories), dtype=np.float64)
    codes = np.ascontiguousarray(column.cat.codes.to_numpy(), dtype=np.int32)  # -1: no category (NaN)

    ctx = default_context(device)
    g = cached_graph(ctx, adj, with_data=True)
    hops = niche_label_hops(ctx, g, codes, n_categories, distance, weighted=True, normalise=not abs_nhood)
    return combine_hop_profiles(hops, weights, bool(abs_nhood))


def niche_utag_features(
    adata: Any,
    spatial_connectivities_key: str = "spatial_connectivities",
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> np.ndarray:
    """The feature matrix of the reference's ``utag`` flavour, ``normalize(A, norm="l1", axis=1) @ adata.X`` (gr/_niche.py:1259-1260),
    as an ``(n_obs, n_vars)`` C-contiguous float64 array: the rows of the graph are divided by their L1 norm (a row of norm 0 stays
    as it is) and multiplied by ``adata.X`` on the GPU.  ``adata.X`` may be dense, CSR or CSC, float32 or float64; it is densified on
    the device one block of columns at a time.

    Float64 throughout (float32 is widened exactly; the reference's result dtype follows its inputs); every row sum runs in ascending
    column order with separately rounded products and sums.  The result is pinned to the reference run on ``.astype(float64)`` inputs.
    Nothing is written into ``adata``.

    The reference's next step is ``sc.tl.pca`` on this matrix, then ``sc.pp.neighbors`` and ``sc.tl.leiden``.  Under a process group
    every rank computes the whole result."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    adj = _canonical_graph(adata, spatial_connectivities_key)
    X = _feature_matrix(adata)
    out = np.zeros((adata.n_obs, X.shape[1]), dtype=np.float64)
    if out.size == 0:
        return out
    ctx = default_context(device)
    g = cached_graph(ctx, adj, with_data=True)
    m = DeviceMatrix(ctx, X)
    try:
        niche_aggregate(ctx, m, out, graph=g)
    finally:
        m.close()
    return out


def _unit_graph(adata: Any, key: str) -> Any:
    adj = _canonical_graph(adata, key)
    if adj.nnz and not (adj.data == 1).all():
        raise NotImplementedError(
            "The CellCharter hop shells need a graph whose stored values are all 1 (what every builder returns with `transform=None`): "
            "the reference compares float path sums of a weighted graph against visit counts, which has no meaning worth pinning."
        )
    return adj


def hop_shells(adj: Any, distance: int, *, device: int | None = None, count_limit: int = 0) -> "list[tuple[Any, Any]]":
    """``[(hop_k, vis_k) for k = 1 .. distance]`` of the reference's ``_hop`` recurrence (see ``niche_cellcharter_features``) as scipy
    CSR matrices, built on the GPU; ``adj`` a canonical CSR matrix of ones.  ``count_limit`` lowers the path count limit of 2**24."""
    ctx = default_context(device)
    shells = HopShells(ctx, cached_graph(ctx, adj, with_data=False), distance, count_limit)
    try:
        return [shells.read(k) for k in range(1, distance + 1)]
    finally:
        shells.close()


def niche_cellcharter_features(
    adata: Any,
    distance: int = 3,
    aggregation: str = "mean",
    spatial_connectivities_key: str = "spatial_connectivities",
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> np.ndarray:
    """The aggregated matrix of the reference's ``cellcharter`` flavour with ``use_rep=None`` — ``arr`` of gr/_niche.py:1336-1355, in
    front of the PCA — as an ``(n_obs, (distance + 1) * n_vars)`` C-contiguous float64 array.  Block 0 is ``adata.X``; block ``k`` is
    ``D_k^-1 hop_k X`` for ``"mean"`` and ``D_k^-1 hop_k X^2 - (D_k^-1 hop_k X)^2`` for ``"variance"``, ``D_k`` the row sums of
    ``hop_k`` (1/0 -> 0).

    The shells follow the reference's ``_setdiag`` / ``_hop`` literally, which is NOT a breadth-first search.  With ``vis_1 = A`` with
    its diagonal set to 1 and ``hop_1 = A`` without its diagonal::

        P_k   = hop_{k-1} @ A        # path counts; self loops of A take part
        hop_k = P_k > vis_{k-1}      # elementwise, an absent entry is 0
        vis_k = vis_{k-1} + hop_k

    so a node visited before re-enters shell ``k`` whenever more paths reach it than it has been visited: on a hexagonal lattice every
    1-hop neighbour is in shell 2 again.  The shells are built on the GPU as sorted CSR with 32-bit integer path counts.

    Every stored value of the graph must be 1 (``NotImplementedError`` otherwise), and a path count that reaches 2**24 — where the
    reference's float32 sums stop being exact — raises ``NotImplementedError``.  An invalid ``aggregation`` raises the reference's
    ``ValueError``.  Float64 throughout (float32 ``X`` is widened exactly; the reference's result dtype is an accident of its inputs);
    row sums in ascending column order, products and sums rounded separately, variance as ``m2 - m1 * m1``.  The result is pinned to
    the reference run on ``.astype(float64)`` inputs.  Nothing is written into ``adata``.

    The reference's next step is ``sc.tl.pca`` on this matrix, then the Gaussian mixture (``gmm_fit`` takes up to 64 columns of it).
    Under a process group every rank computes the whole result."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    distance = _check_distance(distance)
    if aggregation not in ("mean", "variance"):
        raise ValueError(f"Invalid aggregation method '{aggregation}'. Please choose either 'mean' or 'variance'.")
    adj = _unit_graph(adata, spatial_connectivities_key)
    X = _feature_matrix(adata)
    n, nv = adata.n_obs, X.shape[1]
    out = np.zeros((n, (distance + 1) * nv), dtype=np.float64)
    if out.size == 0:
        return out
    ctx = default_context(device)
    g = cached_graph(ctx, adj, with_data=False)
    m = DeviceMatrix(ctx, X)
    shells = None
    try:
        try:
            shells = HopShells(ctx, g, distance)
        except SqgrError as exc:
            if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
                raise NotImplementedError(str(exc)) from None
            raise
        for k in range(distance + 1):
            niche_aggregate(ctx, m, out[:, k * nv : (k + 1) * nv], shells=shells, k=k, variance=aggregation == "variance")
    finally:
        if shells is not None:
            shells.close()
        m.close()
    return out


# ---- stage 2 of the utag and cellcharter flavours: scanpy's default PCA -----------------------------------------------------------------
# gr/_niche.py:1334, the sentence `_CellcharterEmbedder.get_embedding` logs when `use_rep` is None
PROXY_PCA_MSG = (
    "CellCharter recommends to use a dimensionality reduced embedding of the data, e.g. a scVI embedding. Since 'use_rep' is not provided, "
    "PCA will be used as proxy - performance may be suboptimal."
)


class PCAResult(NamedTuple):
    """What ``niche_pca`` returns: scanpy's ``obsm["X_pca"]`` (float64 here), ``varm["PCs"].T``, ``uns["pca"]["variance"]`` and
    ``["variance_ratio"]`` — sklearn's ``fit_transform(X)``, ``components_``, ``explained_variance_``, ``explained_variance_ratio_`` — and
    ``mean_``."""

    X_pca: np.ndarray
    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    mean: np.ndarray


def _check_aggregation(aggregation: Any) -> None:
    if aggregation not in ("mean", "variance"):
        raise ValueError(f"Invalid aggregation method '{aggregation}'. Please choose either 'mean' or 'variance'.")


def pca_n_comps(n: int, d: int, n_comps: int | None = None) -> int:
    """The number of components: ``n_comps``, or scanpy's documented default — 50, or ``min(n, d) - 1`` when ``min(n, d) <= 50``."""
    if n_comps is None:
        return 50 if min(n, d) > 50 else min(n, d) - 1
    if isinstance(n_comps, bool) or not isinstance(n_comps, numbers.Integral):
        raise TypeError(f"Expected `n_comps` to be of type `int`, found `{type(n_comps).__name__}`.")
    if n_comps < 1:
        raise ValueError(f"Expected `n_comps` to be positive, found `{n_comps}`.")
    return int(n_comps)


def _check_pca_shape(n: int, d: int, n_comps: int | None) -> int:
    """Every refusal of the PCA kernels' limits, on the host; returns the number of components."""
    if not (2 <= d <= PCA_MAX_FEATURES) or not (2 <= n < 2**31):
        raise NotImplementedError(
            f"The PCA kernels support 2 to {PCA_MAX_FEATURES} features and 2 to 2**31 - 1 rows; found {d} features and {n} rows."
        )
    c = pca_n_comps(n, d, n_comps)
    if c > PCA_MAX_COMPONENTS or c >= min(n, d):
        raise NotImplementedError(
            f"The PCA kernels support at most {PCA_MAX_COMPONENTS} components, fewer than min(n_obs, n_features) = {min(n, d)} "
            f"(the arpack solver's own condition); found {c}."
        )
    return c


def pca_components(scatter: np.ndarray, n: int, c: int) -> tuple[np.ndarray, np.ndarray]:
    """``(components (c, D), explained_variance (c,))`` from the centred scatter matrix of ``n`` rows: the ``c`` largest eigenpairs of
    ``scatter / (n - 1)`` (LAPACK, on the host), descending, negative eigenvalues clamped to 0, every component oriented by sklearn's
    ``svd_flip(u_based_decision=False)``: its entry of largest magnitude — the first one on ties — is positive."""
    from scipy.linalg import eigh

    d = scatter.shape[0]
    lam, vec = eigh(scatter / (n - 1), subset_by_index=[d - c, d - 1])
    lam, vec = lam[::-1], vec[:, ::-1]
    components = np.ascontiguousarray(vec.T)
    pivot = np.argmax(np.abs(components), axis=1)  # the first maximum
    signs = np.sign(components[np.arange(c), pivot])
    signs[signs == 0] = 1.0
    components *= signs[:, None]
    return components, np.maximum(lam, 0.0)


def _pca_on_device(pca: DevicePCA, c: int) -> PCAResult:
    mean, scatter = pca.moments()
    components, variance = pca_components(scatter, pca.n, c)
    total = np.trace(scatter) / (pca.n - 1)
    return PCAResult(pca.project(components), components, variance, variance / total, mean)


def niche_pca(X: Any, n_comps: int | None = None, *, device: int | None = None) -> PCAResult:
    """scanpy's default ``sc.tl.pca`` on a dense matrix — ``sklearn.decomposition.PCA(n_comps, svd_solver="arpack",
    random_state=0).fit_transform(X)`` — split between device and host: the column means, the centred scatter matrix
    ``sum_i (x_i - mean)(x_i - mean)^T`` and the projection run on the GPU in float64 (``csrc/sqgr_pca.hip``); the ``c`` largest
    eigenpairs of the D x D matrix ``scatter / (n - 1)`` come from ``scipy.linalg.eigh`` on the host, are sorted descending, clamped at
    0 and oriented by sklearn's sign rule (in each component the entry of largest magnitude, the first on ties, is positive).

    ``n_comps=None`` follows scanpy's documented rule: 50, or ``min(n, D) - 1`` when ``min(n, D) <= 50``.  Supported are
    ``2 <= D <= 4096``, ``2 <= n < 2**31`` and ``1 <= n_comps <= 64`` with ``n_comps < min(n, D)`` (``NotImplementedError`` beyond);
    NaN or infinity is a ``ValueError``.

    The result is float64 (a float32 ``X`` is widened exactly first).  scanpy rounds ``X_pca`` to float32 by default, and sklearn's
    mixture would then fit in float32; as with ``gmm_fit`` this library stays in float64 and is pinned to sklearn on float64 input.
    An eigenvector is determined up to ``eps * lambda_1 / gap`` (``gap`` its eigenvalue's distance to the nearest other one): that is
    how closely the scores follow sklearn's.  Every order of summation depends on ``(n, D)`` alone: two calls return
    the same bytes.  Under a process group every rank computes the whole result."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected a 2-D array, found shape `{X.shape}`.")
    n, d = X.shape
    c = _check_pca_shape(n, d, n_comps)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    if X.strides[1] != X.itemsize or X.strides[0] % X.itemsize or X.strides[0] < d * X.itemsize:
        X = np.ascontiguousarray(X)
    if not np.isfinite(X).all():
        raise ValueError("Input X contains NaN or infinity.")
    ctx = default_context(device)
    pca = _device_pca(ctx, n, d)
    try:
        pca.upload(X)
        return _pca_on_device(pca, c)
    finally:
        pca.close()


def _device_pca(ctx: Any, n: int, d: int) -> DevicePCA:
    try:
        return DevicePCA(ctx, n, d)
    except SqgrError as exc:
        if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
            raise NotImplementedError(str(exc)) from None
        raise


def _cellcharter_pca(adj: Any, X: Any, distance: int, aggregation: str, n_comps: int | None, device: int | None) -> PCAResult:
    """``niche_pca`` of the CellCharter feature matrix of the unit graph ``adj`` (canonical CSR) and ``X``, block by block on the device."""
    n, nv = X.shape
    c = _check_pca_shape(n, (distance + 1) * nv, n_comps)
    ctx = default_context(device)
    g = cached_graph(ctx, adj, with_data=False)
    m = DeviceMatrix(ctx, X)
    shells = pca = None
    try:
        try:
            shells = HopShells(ctx, g, distance)
        except SqgrError as exc:
            if exc.status == -4:  # SQGR_ERR_UNSUPPORTED
                raise NotImplementedError(str(exc)) from None
            raise
        pca = _device_pca(ctx, n, (distance + 1) * nv)
        for k in range(distance + 1):
            pca.fill_aggregate(k * nv, m, shells=shells, k=k, variance=aggregation == "variance")
        return _pca_on_device(pca, c)
    finally:
        if pca is not None:
            pca.close()
        if shells is not None:
            shells.close()
        m.close()


def niche_cellcharter_embedding(
    adata: Any,
    distance: int = 3,
    aggregation: str = "mean",
    spatial_connectivities_key: str = "spatial_connectivities",
    n_comps: int | None = None,
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> np.ndarray:
    """The embedding of the reference's ``cellcharter`` flavour with ``use_rep=None`` (gr/_niche.py:1336-1359):
    ``niche_pca(niche_cellcharter_features(adata, distance, aggregation, ...), n_comps).X_pca``, bit for bit, with the
    ``(n_obs, (distance + 1) * n_vars)`` feature matrix built and reduced on the device — only the ``(n_obs, n_comps)`` float64
    embedding crosses to the host.  Arguments, refusals and arithmetic are those of ``niche_cellcharter_features`` and ``niche_pca``."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    distance = _check_distance(distance)
    _check_aggregation(aggregation)
    adj = _unit_graph(adata, spatial_connectivities_key)
    X = _feature_matrix(adata)
    return _cellcharter_pca(adj, X, distance, aggregation, n_comps, device).X_pca


def niche_utag_embedding(
    adata: Any,
    spatial_connectivities_key: str = "spatial_connectivities",
    n_comps: int | None = None,
    *,
    table_key: str | None = None,
    device: int | None = None,
) -> np.ndarray:
    """The embedding of the reference's ``utag`` flavour (gr/_niche.py:1259-1263): ``niche_pca(niche_utag_features(adata, ...),
    n_comps).X_pca``, bit for bit, with the feature matrix built and reduced on the device — only the ``(n_obs, n_comps)`` float64
    embedding crosses to the host.  The reference's next steps are ``sc.pp.neighbors`` and ``sc.tl.leiden``."""
    adata = extract_adata_if_sdata(adata, table_key=table_key)
    adj = _canonical_graph(adata, spatial_connectivities_key)
    X = _feature_matrix(adata)
    n, nv = X.shape
    c = _check_pca_shape(n, nv, n_comps)
    ctx = default_context(device)
    g = cached_graph(ctx, adj, with_data=True)
    m = DeviceMatrix(ctx, X)
    pca = None
    try:
        pca = _device_pca(ctx, n, nv)
        pca.fill_aggregate(0, m, graph=g)
        return _pca_on_device(pca, c).X_pca
    finally:
        if pca is not None:
            pca.close()
        m.close()
