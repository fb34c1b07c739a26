"""``squidpy.tl`` on the MI355X: the one function of that module with a data-parallel search, :func:`var_by_distance`."""

from ._var_by_distance import anchor_distances, var_by_distance

__all__ = ["var_by_distance", "anchor_distances"]
