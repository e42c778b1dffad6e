"""graph_weather/models/layers/film.py of the reference."""
from graph_weather_amd.modulation import FiLMApplier, FiLMGenerator  # noqa: F401
