"""graph_weather/models/fgn/layers/processor.py of the reference."""
from graph_weather_amd.fgn import Processor  # noqa: F401
