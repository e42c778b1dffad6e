"""graph_weather/models/gencast/sampler.py of the reference."""
from graph_weather_amd.gencast_sampler import Sampler  # noqa: F401
