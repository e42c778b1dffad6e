"""graph_weather/models/gencast/denoiser.py of the reference."""
from graph_weather_amd.gencast_model import Denoiser, DenoiserConfig  # noqa: F401
