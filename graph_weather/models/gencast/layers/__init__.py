"""graph_weather/models/gencast/layers/__init__.py of the reference."""
from .decoder import Decoder  # noqa: F401
from .encoder import Encoder  # noqa: F401
from .modules import MLP, InteractionNetwork  # noqa: F401
