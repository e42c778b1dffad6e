"""Training an FGN ensemble on an MI355X with the fair CRPS: a small ``FunctionalGenerativeNetwork``, four members per sample,
``EnsembleCRPSLoss`` weighted by the area of the grid cells, and ``graph_weather_amd.AdamW``.

    python examples/fgn_train_crps.py [--degrees 10] [--members 4] [--steps 5] [--alpha 1.0]

The reference has no such loss; ``alpha`` below 1 gives the "almost fair" score, which keeps a penalty on members that collapse onto
each other."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import graph_weather_amd as gw
from graph_weather.models.fgn import FunctionalGenerativeNetwork  # the reference's line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", type=float, default=10.0)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1.0)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    grid_lon = np.arange(0.0, 360.0, args.degrees)
    grid_lat = np.arange(-90.0, 90.0 + 1e-9, args.degrees)
    features, batch = 4, 2

    model = FunctionalGenerativeNetwork(grid_lon=grid_lon, grid_lat=grid_lat, input_features_dim=features, output_features_dim=features,
                                        noise_dimension=16, hidden_dims=[64, 64], num_blocks=2, num_heads=4, splits=2,
                                        num_hops=2).to(device)
    criterion = gw.EnsembleCRPSLoss(grid_lat=torch.tensor(grid_lat, dtype=torch.float32), alpha=args.alpha).to(device)
    optimizer = gw.AdamW(model.parameters(), lr=1e-3)

    previous_state = torch.randn(batch, len(grid_lon), len(grid_lat), features, device=device)
    target = previous_state + 0.1 * torch.randn(batch, len(grid_lon), len(grid_lat), features, device=device)
    model.train()
    for step in range(args.steps):
        optimizer.zero_grad()
        members = model(previous_state, num_ensemble=args.members)  # [batch, members, lon, lat, features]
        loss = criterion(members, target)
        loss.backward()
        optimizer.step()
        print("step %d: fair CRPS %.5f, mean ensemble spread %.4f" % (step, loss.item(), members.detach().std(dim=1).mean().item()))

    model.eval()
    with torch.no_grad():
        members = model(previous_state, num_ensemble=args.members)
        score_map = gw.EnsembleCRPSLoss(grid_lat=torch.tensor(grid_lat, dtype=torch.float32), alpha=args.alpha, reduction="none").to(device)(
            members, target)
    print("per-feature score after training: %s" % [round(v, 4) for v in score_map.mean(dim=(0, 1, 2)).tolist()])


if __name__ == "__main__":
    main()
