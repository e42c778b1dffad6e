"""graph_weather/models/cafa/processor.py of the reference."""
from graph_weather_amd.cafa import CaFAProcessor  # noqa: F401
