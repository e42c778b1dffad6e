"""graph_weather/models/genda/__init__.py of the reference."""
from .model import GenDA  # noqa: F401
