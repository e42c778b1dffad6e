"""graph_weather/models/layers/thermalizer.py of the reference."""
from graph_weather_amd.thermalizer import AdaptiveUNet, ThermalizerLayer  # noqa: F401
