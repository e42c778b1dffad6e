"""graph_weather/models/weathermesh/weathermesh2.py of the reference."""
from graph_weather_amd.weathermesh_model import WeatherMesh, WeatherMeshConfig, WeatherMeshOutput  # noqa: F401
