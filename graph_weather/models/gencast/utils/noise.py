"""graph_weather/models/gencast/utils/noise.py of the reference (generate_isotropic_noise draws on a HIP device given with device=)."""
from graph_weather_amd.gencast_model import Preconditioner, generate_isotropic_noise, sample_noise_level  # noqa: F401
