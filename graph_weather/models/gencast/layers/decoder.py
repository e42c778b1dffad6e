"""graph_weather/models/gencast/layers/decoder.py of the reference."""
from graph_weather_amd.gencast import Decoder  # noqa: F401
