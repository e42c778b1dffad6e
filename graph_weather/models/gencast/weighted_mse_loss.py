"""graph_weather/models/gencast/weighted_mse_loss.py of the reference."""
from graph_weather_amd.gencast_sampler import WeightedMSELoss  # noqa: F401
