"""graph_weather/models/gencast/graph/model_utils.py of the reference: the coordinate helpers and the two spatial-feature functions
under the configuration GraphBuilder fixes (the xarray helpers are not provided)."""
from graph_weather_amd.gencast_graphs import (  # noqa: F401
    cartesian_to_spherical,
    get_bipartite_graph_spatial_features,
    get_graph_spatial_features,
    lat_lon_deg_to_spherical,
    spherical_to_cartesian,
    spherical_to_lat_lon,
)
