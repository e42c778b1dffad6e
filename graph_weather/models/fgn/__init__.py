"""graph_weather/models/fgn/__init__.py of the reference."""
from .model import FunctionalGenerativeNetwork, FunctionalGenerativeNetworkConfig  # noqa: F401
