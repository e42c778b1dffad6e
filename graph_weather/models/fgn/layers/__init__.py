"""graph_weather/models/fgn/layers/__init__.py of the reference."""
from .processor import Processor  # noqa: F401
