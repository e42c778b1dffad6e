"""graph_weather/models/aurora/__init__.py of the reference."""
from graph_weather_amd.aurora import MODEL_CONFIGS, __version__, create_loss, create_model  # noqa: F401

from .decoder import Decoder3D  # noqa: F401
from .encoder import Swin3DEncoder  # noqa: F401
from .model import AuroraModel, EarthSystemLoss  # noqa: F401
from .processor import PerceiverProcessor  # noqa: F401

__all__ = [
    "AuroraModel",
    "EarthSystemLoss",
    "Swin3DEncoder",
    "Decoder3D",
    "PerceiverProcessor",
]
