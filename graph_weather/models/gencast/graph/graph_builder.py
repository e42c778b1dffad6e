"""graph_weather/models/gencast/graph/graph_builder.py of the reference."""
from graph_weather_amd.gencast_graphs import Data, GraphBuilder, HeteroData  # noqa: F401
