"""graph_weather/models/cafa/decoder.py of the reference."""
from graph_weather_amd.cafa import CaFADecoder  # noqa: F401
