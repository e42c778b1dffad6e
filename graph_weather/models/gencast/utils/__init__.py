"""graph_weather/models/gencast/utils of the reference (statistics.py is not provided)."""
from .noise import generate_isotropic_noise  # noqa: F401
