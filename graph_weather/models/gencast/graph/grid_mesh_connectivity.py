"""graph_weather/models/gencast/graph/grid_mesh_connectivity.py of the reference (the closest face by the package's own rule:
graph_weather_amd/gencast_graphs.py)."""
from graph_weather_amd.gencast_graphs import in_mesh_triangle_indices, radius_query_indices  # noqa: F401
