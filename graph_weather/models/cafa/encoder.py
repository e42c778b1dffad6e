"""graph_weather/models/cafa/encoder.py of the reference."""
from graph_weather_amd.cafa import CaFAEncoder  # noqa: F401
