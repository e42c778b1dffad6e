"""graph_weather/models/gencast of the reference: the layers package only (Denoiser, GraphBuilder, Sampler, WeightedMSELoss and
generate_isotropic_noise are not provided)."""
