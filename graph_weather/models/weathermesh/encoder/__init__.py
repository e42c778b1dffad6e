"""graph_weather/models/weathermesh/encoder.py of the reference."""
from graph_weather_amd.weathermesh_model import WeatherMeshEncoder, WeatherMeshEncoderConfig  # noqa: F401
