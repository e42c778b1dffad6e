"""graph_weather/models/gencast/layers/encoder.py of the reference."""
from graph_weather_amd.gencast import Encoder  # noqa: F401
