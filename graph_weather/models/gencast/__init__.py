"""graph_weather/models/gencast of the reference: the layers, the graphs, the Denoiser and its utilities (Sampler, WeightedMSELoss,
utils/statistics.py and train.py are not provided; generate_isotropic_noise raises NotImplementedError)."""
from .denoiser import Denoiser  # noqa: F401
from .graph.graph_builder import GraphBuilder  # noqa: F401
from .utils.noise import generate_isotropic_noise  # noqa: F401
