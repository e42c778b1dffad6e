"""``NormalizedMSELoss`` - reference ``graph_weather/models/losses.py:9-94`` (cos-latitude weighted MSE)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class NormalizedMSELoss(torch.nn.Module):
    """losses.py:12-44 (constructor) / :46-94 (forward).  The four shape prints and the two host-syncing NaN
    asserts of the reference forward are dropped; the value is identical."""

    def __init__(self, feature_variance: list, lat_lons: list, device="cpu", normalize: bool = False):
        super().__init__()
        self.feature_variance = torch.as_tensor(feature_variance, dtype=torch.float32).clone()
        assert not torch.isnan(self.feature_variance).any()
        unique_lats = sorted(set(lat for lat, _ in lat_lons))
        self.weights = torch.tensor([np.cos(lat * np.pi / 180.0) for lat in unique_lats], dtype=torch.float)
        self.normalize = normalize
        assert not torch.isnan(self.weights).any()

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self.feature_variance = self.feature_variance.to(pred.device)
        self.weights = self.weights.to(pred.device)
        inv_var = None
        if self.normalize:
            fv = self.feature_variance
            if fv.numel() == pred.shape[-1]:
                inv_var = (1.0 / fv.reshape(-1)).contiguous()
            else:  # anything that broadcasts against [B, G, C] (losses.py:69; the reference's own test passes [B, G, C])
                inv_var = (1.0 / torch.broadcast_to(fv, pred.shape)).contiguous()
        if torch.is_grad_enabled() and pred.requires_grad:
            from .autograd import NormalizedMSEFunction

            return NormalizedMSEFunction.apply(pred.contiguous(), target.contiguous(), self.weights.contiguous(), inv_var)
        return ops.normalized_mse_forward(pred.contiguous(), target.contiguous(), self.weights.contiguous(), inv_var)


class AMSENormalizedLoss(torch.nn.Module):
    """losses.py:98-195: the spectrally adjusted MSE of "Fixing the Double Penalty in Data-Driven Weather Forecasting Through
    a Modified Spherical Harmonic Loss Function" on [B, C, H, W] fields.  The reference's ``torch_harmonics.RealSHT`` is
    replaced by the HIP kernels of csrc/gw_sht.hip (fp32 MFMA, per-degree sums and loss terms combined in fp64); the tables
    are built on the host once per ``(nlat, nlon, device)`` (``ops.amse_tables``) - see ``sht_tables`` for what a shape costs.  Unlike the
    reference's ``.view`` the inputs need not be contiguous.  Only ``pred`` gets a gradient."""

    def __init__(self, feature_variance, epsilon: float = 1e-9):
        super().__init__()
        if not isinstance(feature_variance, torch.Tensor):
            feature_variance = torch.tensor(feature_variance, dtype=torch.float32)
        else:
            feature_variance = feature_variance.clone().detach().float()
        self.register_buffer("feature_variance", feature_variance)
        self.epsilon = epsilon

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if pred.shape != target.shape:
            raise ValueError("Prediction and target tensors must have the same shape.")
        if pred.ndim != 4:
            raise ValueError("Input tensors must be 4D: (batch, channels, lat, lon)")
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("graph_weather_amd: pred and target must be on a HIP device - there is no CPU path")
        if torch.is_grad_enabled() and target.requires_grad:
            raise NotImplementedError("graph_weather_amd: AMSENormalizedLoss has no gradient for target (only for pred)")
        variance = self.feature_variance.to(pred.device).reshape(-1).contiguous()
        p, t = pred.float().contiguous(), target.detach().float().contiguous()
        if torch.is_grad_enabled() and pred.requires_grad:
            from .autograd import AMSENormalizedFunction

            return AMSENormalizedFunction.apply(p, t, variance, float(self.epsilon))
        return ops.amse_forward(p, t, variance, float(self.epsilon))
