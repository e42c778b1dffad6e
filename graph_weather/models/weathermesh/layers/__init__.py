"""graph_weather/models/weathermesh/layers.py of the reference."""
from graph_weather_amd.weathermesh_model import ConvDownBlock, ConvUpBlock  # noqa: F401
