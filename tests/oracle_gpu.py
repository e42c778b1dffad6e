"""The replicated (reference) branch of oracle/reference_math.py run on the device: at 1 degree its fp64 autograd needs tens of
GB and hours on the host.  The oracle's own factory calls (torch.zeros, torch.tensor) take no device argument; they are sent to
the device by running it under ``torch.device(dev)``, and its graph arrays are moved there here."""
import torch

from oracle import reference_math as om


def graphs_on(g: dict, dev, dtype) -> dict:
    g = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    return om.graphs_to_dtype(g, dtype)


def params_on(sd: dict, dev, dtype, requires_grad: bool = False) -> dict:
    return {k: v.detach().to(dev, dtype).clone().requires_grad_(requires_grad) for k, v in sd.items()}


def forecast(sd: dict, g: dict, feats: torch.Tensor, dev, dtype=torch.float64) -> torch.Tensor:
    """GraphWeatherForecaster.forward of the oracle (replicated branch) under no_grad, on ``dev`` in ``dtype``."""
    with torch.no_grad(), torch.device(dev):
        return om.forecaster_forward(params_on(sd, dev, dtype), graphs_on(g, dev, dtype), feats.to(dev, dtype))


def loss(p: dict, g: dict, feats: torch.Tensor, target: torch.Tensor, lat_lons, dev) -> torch.Tensor:
    """NormalizedMSELoss(normalize=False) of the oracle forecast, with autograd, on ``dev`` in the dtype of ``p``."""
    dtype = next(iter(p.values())).dtype
    with torch.device(dev):
        y = om.forecaster_forward(p, graphs_on(g, dev, dtype), feats.to(dev, dtype))
        return om.normalized_mse_loss(y, target.to(dev, dtype), lat_lons, None, normalize=False)
