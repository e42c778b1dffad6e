"""graph_weather/models/layers/constraint_layer.py of the reference."""
from graph_weather_amd.constraint import PhysicalConstraintLayer  # noqa: F401
