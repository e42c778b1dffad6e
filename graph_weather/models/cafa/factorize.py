"""graph_weather/models/cafa/factorize.py of the reference."""
from graph_weather_amd.cafa import AxialAttention, FactorizedAttention, FactorizedTransformerBlock, FeedFoward  # noqa: F401
