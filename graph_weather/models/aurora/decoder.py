"""graph_weather/models/aurora/decoder.py of the reference."""
from graph_weather_amd.aurora import Decoder3D  # noqa: F401
