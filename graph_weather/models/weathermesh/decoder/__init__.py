"""graph_weather/models/weathermesh/decoder.py of the reference."""
from graph_weather_amd.weathermesh_model import WeatherMeshDecoder, WeatherMeshDecoderConfig  # noqa: F401
