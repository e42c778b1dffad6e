"""graph_weather/models/aurora/encoder.py of the reference."""
from graph_weather_amd.aurora import Swin3DEncoder  # noqa: F401
