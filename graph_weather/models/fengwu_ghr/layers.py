"""graph_weather/models/fengwu_ghr/layers.py of the reference."""
from graph_weather_amd.fengwu_ghr import (  # noqa: F401
    Attention,
    FeedForward,
    ImageMetaModel,
    MetaModel,
    Transformer,
    WrapperImageModel,
    WrapperMetaModel,
    pair,
    posemb_sincos_2d,
)
