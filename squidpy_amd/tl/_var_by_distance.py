"""``sq.tl.var_by_distance``: distances of every observation to the nearest member of each anchor group, per slide, as a design
matrix (tl/_var_by_distance.py).  The reference builds one sklearn ``KDTree`` per (anchor, slide) and queries it in a Python loop;
here ONE library call (``sqgr_anchor_dist``) serves all anchors and all slides, and the frame is then put together on the host
with pandas — O(n) bookkeeping, as in the reference.  There is no CPU path for the search.

One deliberate divergence: the reference finds the NaN rows in ``obsm[spatial_key]`` but reads the coordinates from
``obsm["spatial"]`` whatever ``spatial_key`` says; here ``spatial_key`` names both.  The default is identical."""

from __future__ import annotations

from functools import reduce
from typing import Any, Callable

import numpy as np
import pandas as pd

from .. import _lib
from .._utils import _save_data
from ..gr._ripley import KDTREE_VALID_METRICS

__all__ = ["var_by_distance", "anchor_distances"]

CUSTOM = "custom_anchor"
# search(coords (n, d), slide_codes (n,), ref_coords (m, d), ref_sets (m,), set_of (n_columns, n_slides), metric) -> (n_columns, n)
Search = Callable[[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, str], np.ndarray]


def _device_search(device: int | None) -> Search:
    def search(coords, slide_codes, ref_coords, ref_sets, set_of, metric):
        return _lib.anchor_distances(_lib.default_context(device), coords, slide_codes, ref_coords, ref_sets, set_of, metric)

    return search


def _check_metric(metric: str) -> None:
    if metric not in KDTREE_VALID_METRICS or metric not in _lib.METRICS:
        raise ValueError(f"metric '{metric}' is not valid for KDTree; use one of {[m for m in KDTREE_VALID_METRICS if m in _lib.METRICS]}")


def anchor_distances(
    coords: Any, labels: Any, anchors: Any, slides: Any = None, metric: str = "euclidean", *, device: int | None = None
) -> np.ndarray:
    """Raw distances without pandas: for every row of ``coords`` ((n, 2) or (n, 3)) and every label in ``anchors`` the ``metric``
    distance to the nearest row of the same slide (``slides``: one value per row, or ``None`` for a single slide) that carries the
    label -> float64 ``(n, len(anchors))``.  NaN marks a row with a non-finite coordinate (such rows are no anchor members
    either) and a slide in which the label does not occur."""
    _check_metric(metric)
    xy = _lib._search_coords(np.asarray(coords, dtype=np.float64))
    n = xy.shape[0]
    labels = np.asarray(labels)
    anchors = list(np.atleast_1d(np.asarray(anchors)).tolist()) if not isinstance(anchors, (list, tuple)) else list(anchors)
    if labels.shape != (n,):
        raise ValueError(f"Expected one label per row of the coordinates, found {labels.shape} for {n} rows.")
    if slides is None:
        slide_codes, n_slides = np.zeros(n, dtype=np.int32), 1
    else:
        slides = np.asarray(slides)
        if slides.shape != (n,):
            raise ValueError(f"Expected one slide per row of the coordinates, found {slides.shape} for {n} rows.")
        slide_codes, uniques = pd.factorize(slides)
        slide_codes, n_slides = slide_codes.astype(np.int32), max(len(uniques), 1)
    out = np.full((n, len(anchors)), np.nan)
    ok = np.isfinite(xy).all(axis=1) & (slide_codes >= 0)
    if not anchors or not ok.any():
        return out
    set_of = np.arange(len(anchors) * n_slides, dtype=np.int32).reshape(len(anchors), n_slides)
    member_rows, member_sets = [], []
    for a, name in enumerate(anchors):
        rows = np.nonzero(ok & (labels == name))[0]
        member_rows.append(rows)
        member_sets.append(set_of[a, slide_codes[rows]])
    rows = np.concatenate(member_rows)
    d = _device_search(device)(xy[ok], slide_codes[ok], xy[rows], np.concatenate(member_sets).astype(np.int32), set_of, metric)
    out[ok] = d.T
    return out


def _anchor_names(groups: Any) -> list:
    if isinstance(groups, str):
        return [groups]
    if isinstance(groups, list):
        return groups
    if isinstance(groups, np.ndarray):
        if groups.ndim != 1:
            raise ValueError(f"Expected a 1D array for 'groups', but got shape {groups.shape}.")
        return groups.astype(str).tolist()
    raise TypeError(f"Expected `groups` to be of type `str or list or ndarray`, got `{type(groups).__name__}`.")


def _slides(obs: pd.DataFrame, library_key: Any, library_id: Any) -> list:
    """The slides in the order the reference visits them; ``[None]`` without ``library_key``."""
    if library_key is None:
        return [None]
    if not isinstance(library_key, str):
        raise TypeError(f"Expected `library_key` to be of type `str`, got `{type(library_key).__name__}`.")
    present = obs[library_key].unique()
    if library_id is None:
        return present.tolist()
    wanted = [library_id] if isinstance(library_id, str) else list(library_id)
    for x in wanted:
        if x not in present:
            raise ValueError(f"library id {x} not in {library_key}")
    return wanted


class _Plan:
    """What one call searches: the anchor columns, the slides, and per (column, slide) the rows whose coordinates form the set."""

    def __init__(self, adata: Any, groups: Any, cluster_key: Any, library_key: Any, library_id: Any, metric: str, spatial_key: str):
        _check_metric(metric)
        obs = adata.obs
        self.anchors = _anchor_names(groups)
        self.slides = _slides(obs, library_key, library_id)
        self.custom = all(isinstance(x, list) for x in self.anchors)
        if self.custom and len(self.anchors) != len(self.slides):
            raise ValueError(
                f"There must be one anchor point per slide. A numpy array with {len(self.anchors)} anchor points was provided, "
                f"but {len(self.slides)} slides were found."
            )
        self.coords = _lib._search_coords(np.asarray(adata.obsm[spatial_key], dtype=np.float64))
        n = self.coords.shape[0]
        self.valid = np.isfinite(self.coords).all(axis=1)
        # rows of every slide (all of them, NaN coordinates included: they get their NaN back) and the code the search sees
        self.slide_rows = [np.ones(n, dtype=bool) if s is None else (obs[library_key] == s).to_numpy() for s in self.slides]
        self.slide_codes = np.full(n, -1, dtype=np.int32)
        for code, rows in enumerate(self.slide_rows):
            self.slide_codes[rows] = code
        self.columns = [CUSTOM] if self.custom else [str(a) for a in self.anchors]
        # (column, slide code) in the reference's order of visits; a labelled anchor that a slide lacks is left out
        self.visits: list[tuple[int, int]] = []
        self.ref_coords: list[np.ndarray] = []
        self.set_of = np.full((len(self.columns), len(self.slides)), -1, dtype=np.int32)
        if self.custom:
            for code, point in enumerate(self.anchors):
                ref = np.array(point, dtype=np.float64).reshape(1, -1)
                if ref.shape[1] != self.coords.shape[1] or not np.isfinite(ref).all():
                    raise ValueError(f"anchor point {point} does not match the coordinates of width {self.coords.shape[1]} (or is not finite)")
                self._add(0, code, ref)
        else:
            labels = obs[cluster_key]
            for col, name in enumerate(self.anchors):
                is_member = (labels == name).to_numpy()
                for code, rows in enumerate(self.slide_rows):
                    if self.slides[code] is not None and not (is_member & rows).any():
                        continue  # the slide's design matrix has no column for this anchor: NaN after the reindex
                    ref = self.coords[is_member & rows & self.valid]
                    if len(ref) == 0:
                        raise ValueError(f"anchor '{name}' has no observation with coordinates" + (f" in slide '{self.slides[code]}'" if self.slides[code] is not None else f" in `{cluster_key}`"))
                    self._add(col, code, ref)
                if (self.set_of[col] < 0).all():  # (the reference fails in pandas, with nothing to concatenate)
                    raise ValueError(f"anchor '{name}' occurs in none of the slides {self.slides} of `{cluster_key}`")

    def _add(self, col: int, code: int, ref: np.ndarray) -> None:
        self.set_of[col, code] = len(self.ref_coords)
        self.ref_coords.append(ref)
        self.visits.append((col, code))

    def distances(self, search: Search, metric: str) -> np.ndarray:
        """(n_columns, n) with NaN for the rows without coordinates: ONE search for all columns and slides."""
        out = np.full((len(self.columns), self.coords.shape[0]), np.nan)
        if self.visits and self.valid.any():
            ref_sets = np.concatenate([np.full(len(r), s, dtype=np.int32) for s, r in enumerate(self.ref_coords)])
            out[:, self.valid] = search(self.coords[self.valid], self.slide_codes[self.valid], np.concatenate(self.ref_coords), ref_sets, self.set_of, metric)
        return out


def _normalised(frame: pd.DataFrame, name: str) -> pd.DataFrame:
    """Per (slide, anchor): keep the distances as ``{name}_raw``; in ``name`` zeros become NaN, the first minimum 0, and the column
    is divided by its maximum."""
    frame[f"{name}_raw"] = frame[name]
    frame[name] = frame[name].mask(frame[name] == 0)
    frame.loc[frame[name].idxmin(), name] = 0
    frame[name] = frame[name] / frame[name].max()
    return frame


def _design_matrix(
    adata: Any, groups: Any, cluster_key: Any, library_key: Any, library_id: Any, covariates: Any, metric: str, spatial_key: str, search: Search
) -> pd.DataFrame:
    """The frame of :func:`var_by_distance`; ``search`` computes the distances (the device in the product, sklearn in the CPU tests)."""
    plan = _Plan(adata, groups, cluster_key, library_key, library_id, metric, spatial_key)
    dist = plan.distances(search, metric)
    obs = adata.obs
    by_slide = library_key is not None
    position = 2 if (by_slide and cluster_key is not None) else 1
    frames = []
    for col, code in plan.visits:
        rows = plan.slide_rows[code]
        if by_slide:
            sub = obs.loc[rows]
            frame = sub[[cluster_key]].copy() if cluster_key is not None else sub[[library_key]].copy()
            if cluster_key is not None:
                frame[library_key] = sub[library_key].copy()
        else:
            frame = obs[[cluster_key]].copy() if cluster_key is not None else pd.DataFrame(index=obs.index)
        frame.insert(loc=position, column=plan.columns[col], value=dist[col, rows])
        frame["obs"] = obs.index[rows]
        frames.append(_normalised(frame, plan.columns[col]))

    columns = plan.columns
    if not by_slide and len(columns) > 1:  # one frame per anchor over the same rows: joined on the label and the observation
        df = reduce(lambda a, b: pd.merge(a, b, on=[cluster_key, "obs"]), frames)
        df.set_index("obs", inplace=True)
        df.index.name = None
    elif by_slide and len(columns) == 1:  # one frame per slide, stacked and put back into the order of the observations
        df = pd.concat(frames).reindex(obs.index).drop("obs", axis=1)
    elif by_slide:
        per_anchor = [pd.concat([f for f in frames if name in f.columns]).reindex(obs.index).drop("obs", axis=1) for name in columns]
        df = reduce(lambda a, b: pd.merge(a, b[b.columns.difference(a.columns)], left_index=True, right_index=True, how="outer"), per_anchor)
    else:
        df = frames[0].drop("obs", axis=1)

    if covariates is not None:
        covariates = [covariates] if isinstance(covariates, str) else covariates
        df[covariates] = obs[covariates].copy()
    if isinstance(groups, list):
        df = df.reindex(obs.index)
    return df


def var_by_distance(
    adata: Any,
    groups: Any,
    cluster_key: str | None = None,
    library_key: str | None = None,
    library_id: str | list[str] | None = None,
    design_matrix_key: str = "design_matrix",
    covariates: str | list[str] | None = None,
    metric: str = "euclidean",
    spatial_key: str = "spatial",
    copy: bool = False,
    *,
    device: int | None = None,
) -> pd.DataFrame | None:
    """Design matrix of distances to the selected anchor point(s) for each observation — ``squidpy.tl.var_by_distance`` with the
    same positional arguments and defaults.  ``groups``: one label or several of ``obs[cluster_key]`` (str, list, 1-D ndarray), or
    a list of coordinate lists, one per slide (column ``custom_anchor``).  Per (slide, anchor) the raw distances go to
    ``{anchor}_raw``; ``{anchor}`` holds them scaled to [0, 1] with zeros as NaN.  Rows with a non-finite coordinate are neither
    queries nor anchor members and get NaN.  ``metric``: one of sklearn's KDTree metrics.  ``device``: the GPU to run on.

    Returns the frame if ``copy``; otherwise stores it in ``adata.obsm[design_matrix_key]``."""
    df = _design_matrix(adata, groups, cluster_key, library_key, library_id, covariates, metric, spatial_key, _device_search(device))
    if copy:
        return df
    _save_data(adata, attr="obsm", key=design_matrix_key, data=df)
    return None
