"""graph_weather/models/aurora/model.py of the reference."""
from graph_weather_amd.aurora import (  # noqa: F401
    AuroraModel,
    EarthSystemLoss,
    PointCloudProcessor,
    PointDecoder,
    PointEncoder,
    SelfAttentionLayer,
)
