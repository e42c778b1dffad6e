"""graph_weather/models/gencast/layers/processor.py of the reference."""
from graph_weather_amd.gencast import Processor  # noqa: F401
