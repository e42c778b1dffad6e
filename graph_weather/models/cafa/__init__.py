"""graph_weather/models/cafa/__init__.py of the reference."""
from .decoder import CaFADecoder  # noqa: F401
from .encoder import CaFAEncoder  # noqa: F401
from .factorize import AxialAttention, FactorizedAttention, FactorizedTransformerBlock  # noqa: F401
from .model import CaFAForecaster  # noqa: F401
from .processor import CaFAProcessor  # noqa: F401
