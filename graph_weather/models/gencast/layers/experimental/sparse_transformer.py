"""graph_weather/models/gencast/layers/experimental/sparse_transformer.py of the reference."""
from graph_weather_amd.gencast_sparse import SparseAttention, SparseTransformer  # noqa: F401
