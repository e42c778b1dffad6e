"""graph_weather/models/weathermesh/processor.py of the reference."""
from graph_weather_amd.weathermesh import WeatherMeshProcessor, WeatherMeshProcessorConfig  # noqa: F401
