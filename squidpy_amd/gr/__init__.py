"""``squidpy_amd.gr`` — the MI355X-native ``sq.gr`` spatial-statistics hot path."""

from . import neighbors
from ._build import (
    SpatialNeighborsResult,
    spatial_neighbors,
    spatial_neighbors_delaunay,
    spatial_neighbors_from_builder,
    spatial_neighbors_grid,
    spatial_neighbors_knn,
    spatial_neighbors_radius,
)
from ._ligrec import PermutationTest, ligrec
from ._mask import MultiPolygon, Polygon, mask_graph, segments_within
from ._nhood import NhoodEnrichmentResult, centrality_scores, interaction_matrix, nhood_enrichment
from ._niche import (
    PCAResult,
    calculate_niche_cellcharter,
    niche_cellcharter_embedding,
    niche_cellcharter_features,
    niche_nhood_profile,
    niche_pca,
    niche_utag_embedding,
    niche_utag_features,
)
from ._niche_graph import NicheNeighborsResult, niche_knn, niche_neighbors, niche_scale
from ._niche_leiden import LeidenResult, calculate_niche_neighborhood, calculate_niche_utag, niche_leiden, quantise_weights
from ._niche_spatialleiden import MultiplexLeidenResult, calculate_niche_spatialleiden, niche_spatialleiden, quantise_layers
from ._ppatterns import co_occurrence, spatial_autocorr
from ._ripley import ripley
from ._sepal import sepal

__all__ = ["nhood_enrichment", "interaction_matrix", "centrality_scores", "calculate_niche_cellcharter", "niche_nhood_profile", "niche_utag_features", "niche_cellcharter_features", "niche_pca", "niche_utag_embedding", "niche_cellcharter_embedding", "PCAResult", "niche_knn", "niche_neighbors", "niche_scale", "NicheNeighborsResult", "niche_leiden", "quantise_weights", "LeidenResult", "calculate_niche_neighborhood", "calculate_niche_utag", "niche_spatialleiden", "quantise_layers", "MultiplexLeidenResult",
           "calculate_niche_spatialleiden", "NhoodEnrichmentResult", "co_occurrence", "spatial_autocorr", "ripley", "sepal", "ligrec", "PermutationTest", "spatial_neighbors",
           "spatial_neighbors_knn", "spatial_neighbors_delaunay", "spatial_neighbors_radius", "spatial_neighbors_grid", "spatial_neighbors_from_builder",
           "neighbors", "SpatialNeighborsResult", "mask_graph", "Polygon", "MultiPolygon", "segments_within"]
