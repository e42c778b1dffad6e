"""graph_weather/models/losses.py of the reference: both of its losses."""
from graph_weather_amd.losses import AMSENormalizedLoss, NormalizedMSELoss  # noqa: F401
