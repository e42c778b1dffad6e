"""graph_weather/models/cafa/model.py of the reference."""
from graph_weather_amd.cafa import CaFAForecaster  # noqa: F401
