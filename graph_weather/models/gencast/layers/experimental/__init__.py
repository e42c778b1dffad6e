"""graph_weather/models/gencast/layers/experimental/__init__.py of the reference."""
from .sparse_transformer import SparseAttention, SparseTransformer  # noqa: F401
