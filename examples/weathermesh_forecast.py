"""A WeatherMesh forecast and one training step on an MI355X: the model is built with the reference's constructor, moved to the GPU
TOGETHER WITH ITS PROCESSORS (``WeatherMesh.processors`` is a plain Python list, as in the reference: ``.to()``, ``.parameters()``
and ``state_dict()`` do not reach them), run for two forecast steps, and trained for one step.

    python examples/weathermesh_forecast.py [--height 48] [--width 96] [--levels 5] [--hidden 8]

The output's height and width are 2^n times the latent's: larger than the input's when they are no multiple of 2^n."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from graph_weather.models.weathermesh.weathermesh2 import WeatherMesh  # the reference's line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=8)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    surface_channels, pressure_channels, batch = 4, 5, 2

    model = WeatherMesh(encoder=None, processors=None, decoder=None, timesteps=[1, 6], surface_channels=surface_channels,
                        pressure_channels=pressure_channels, pressure_levels=args.levels, latent_dim=32, encoder_num_conv_blocks=2,
                        encoder_num_transformer_layers=1, encoder_hidden_dim=args.hidden, decoder_num_conv_blocks=2,
                        decoder_num_transformer_layers=1, decoder_hidden_dim=args.hidden, processor_num_layers=2, kernel=(3, 5, 5),
                        num_heads=4)
    model.to(device)
    for processor in model.processors:  # not registered sub-modules: moved one by one
        processor.to(device)
    parameters = list(model.parameters()) + [p for processor in model.processors for p in processor.parameters()]
    print("parameters: %d in the model, %d in its %d processors" % (sum(p.numel() for p in model.parameters()),
                                                                   sum(p.numel() for q in model.processors for p in q.parameters()),
                                                                   len(model.processors)))

    surface = torch.randn(batch, surface_channels, args.height, args.width, device=device)
    pressure = torch.randn(batch, pressure_channels, args.levels, args.height, args.width, device=device)

    model.eval()
    with torch.no_grad():
        forecast = model(surface, pressure, forecast_steps=2)
    print("forecast: surface %s, pressure %s" % (tuple(forecast.surface.shape), tuple(forecast.pressure.shape)))

    model.train()
    optimizer = torch.optim.AdamW(parameters, lr=1e-3)
    target_surface, target_pressure = torch.randn_like(forecast.surface), torch.randn_like(forecast.pressure)
    for step in range(2):
        optimizer.zero_grad()
        out = model(surface, pressure, forecast_steps=1)
        loss = (out.surface - target_surface).square().mean() + (out.pressure - target_pressure).square().mean()
        if step == 0:
            loss.backward()
            optimizer.step()
        print("loss %s the training step: %.6f" % ("before" if step == 0 else "after", loss.item()))


if __name__ == "__main__":
    main()
