"""graph_weather/models/gencast of the reference: the layers, the graphs, the Denoiser, the Sampler, the loss and the utilities
(utils/statistics.py and train.py are not provided; generate_isotropic_noise draws on a HIP device given with device=)."""
from .denoiser import Denoiser  # noqa: F401
from .graph.graph_builder import GraphBuilder  # noqa: F401
from .sampler import Sampler  # noqa: F401
from .utils.noise import generate_isotropic_noise  # noqa: F401
from .weighted_mse_loss import WeightedMSELoss  # noqa: F401
