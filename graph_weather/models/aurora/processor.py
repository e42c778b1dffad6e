"""graph_weather/models/aurora/processor.py of the reference."""
from graph_weather_amd.aurora import PerceiverProcessor, ProcessorConfig  # noqa: F401
