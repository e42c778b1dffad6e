"""graph_weather/models/fgn/model.py of the reference."""
from graph_weather_amd.fgn import FunctionalGenerativeNetwork, FunctionalGenerativeNetworkConfig  # noqa: F401
