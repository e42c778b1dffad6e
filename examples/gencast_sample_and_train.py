"""GenCast with the reference's import paths on an MI355X: one training step as the paper trains the Denoiser (isotropic noise at a
sampled noise level, the noise-level-weighted loss) and one ensemble forecast with the Sampler.

    python examples/gencast_sample_and_train.py [--degrees 10] [--members 2] [--steps 5]

The reference's usage (graph_weather/models/gencast/README.md and train.py of openclimatefix/graph_weather) with two changes:
``generate_isotropic_noise`` gets ``device=`` (the noise is drawn and transformed on the device, no torch_harmonics), and
``prev_inputs`` may hold several ensemble members."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from graph_weather.models.gencast import Denoiser, Sampler, WeightedMSELoss, generate_isotropic_noise  # the reference's line
from graph_weather.models.gencast.utils.noise import sample_noise_level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", type=float, default=10.0)
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5, help="num_steps of the Sampler (the reference's default is 20)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    grid_lon = np.arange(0.0, 360.0, args.degrees)
    grid_lat = np.arange(-90.0, 90.0 + 1e-9, args.degrees)  # 2N x (N + 1): one of the two grids isotropic noise accepts
    features, batch = 4, 2

    denoiser = Denoiser(grid_lon=grid_lon, grid_lat=grid_lat, input_features_dim=features, output_features_dim=features,
                        hidden_dims=[64, 64], num_blocks=2, num_heads=4, splits=2, num_hops=2).to(device)
    criterion = WeightedMSELoss(grid_lat=torch.tensor(grid_lat, dtype=torch.float32), pressure_levels=torch.tensor([500.0, 850.0]),
                                num_atmospheric_features=1, single_features_weights=torch.tensor([1.0, 0.1])).to(device)
    optimizer = torch.optim.AdamW(denoiser.parameters(), lr=1e-3)

    # ---- one training step -------------------------------------------------------------------------------------------------
    prev_inputs = torch.randn(batch, len(grid_lon), len(grid_lat), 2 * features, device=device)
    target_residuals = torch.randn(batch, len(grid_lon), len(grid_lat), features, device=device)
    noise_levels = torch.tensor([[sample_noise_level()] for _ in range(batch)], dtype=torch.float32, device=device)
    noise = generate_isotropic_noise(len(grid_lon), len(grid_lat), features, device=device, batch=batch)
    corrupted_targets = target_residuals + noise_levels[:, :, None, None] * noise
    denoiser.train()
    optimizer.zero_grad()
    loss = criterion(denoiser(corrupted_targets, prev_inputs, noise_levels), noise_levels, target_residuals)
    loss.backward()
    optimizer.step()
    print("training step: loss %.4f at noise levels %s" % (loss.item(), [round(v, 3) for v in noise_levels.flatten().tolist()]))

    # ---- an ensemble forecast ----------------------------------------------------------------------------------------------
    denoiser.eval()
    sampler = Sampler(num_steps=args.steps)
    members = prev_inputs[:1].expand(args.members, -1, -1, -1).contiguous()  # every member starts from the same two timesteps
    forecast = sampler.sample(denoiser, members, generator=torch.Generator(device=device).manual_seed(0))
    spread = forecast.std(dim=0).mean().item() if args.members > 1 else 0.0
    print("forecast: %s, finite %s, mean ensemble spread %.4f" % (tuple(forecast.shape), bool(torch.isfinite(forecast).all()), spread))


if __name__ == "__main__":
    main()
