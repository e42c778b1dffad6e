"""graph_weather/models/layers/stochastic_decomposition.py of the reference."""
from graph_weather_amd.modulation import StochasticDecompositionLayer  # noqa: F401
