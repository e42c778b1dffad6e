"""graph_weather/models/gencast/utils/batching.py of the reference."""
from graph_weather_amd.gencast_model import batch, hetero_batch  # noqa: F401
