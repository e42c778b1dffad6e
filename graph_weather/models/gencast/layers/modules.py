"""graph_weather/models/gencast/layers/modules.py of the reference."""
from graph_weather_amd.gencast import (  # noqa: F401
    MLP,
    ConditionalLayerNorm,
    CondTransformerBlock,
    FourierEmbedding,
    InteractionNetwork,
)
