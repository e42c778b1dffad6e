"""graph_weather/models/weathermesh/__init__.py of the reference: the processor only (encoder, decoder and model are not built)."""
from .processor import WeatherMeshProcessor, WeatherMeshProcessorConfig  # noqa: F401
