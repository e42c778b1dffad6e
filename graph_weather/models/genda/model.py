"""graph_weather/models/genda/model.py of the reference."""
from graph_weather_amd.genda import GenDA, GenDAConfig  # noqa: F401
