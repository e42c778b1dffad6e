"""``NormalizedMSELoss`` - reference ``graph_weather/models/losses.py:9-94`` (cos-latitude weighted MSE) -, ``AMSENormalizedLoss``
(losses.py:98-195) and ``EnsembleCRPSLoss``, the training loss of the FGN ensembles (the reference has none)."""
from __future__ import annotations

from typing import Optional

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


class EnsembleCRPSLoss(torch.nn.Module):
    """The continuous ranked probability score of an ensemble against the truth, the training loss of
    ``FunctionalGenerativeNetwork``: ``crit(pred, target)`` with pred [B, N, lon, lat, C] (FGN's output layout) and target
    [B, lon, lat, C].  At one (sample, grid point, feature), with members x_1 .. x_N and truth y,

        v = (1/N) sum_i |x_i - y| - c2 sum_i sum_j |x_i - x_j|,   c2 = alpha / (2 N (N-1)) + (1 - alpha) / (2 N^2)

    ``alpha=1`` is the fair score (unbiased in N; needs N >= 2), ``alpha=0`` the plain ensemble score, values between the "almost
    fair" score, which keeps a penalty on two members that collapse onto each other.  ``grid_lat`` [lat] in degrees gives the area
    weights |cos| normalised to mean 1 (as ``WeightedMSELoss`` forms them), ``features_weights`` [C] the weight of every feature;
    both are non-persistent buffers and either may be absent.  ``reduction="mean"`` returns the mean of the weighted score over
    B lon lat C, ``"none"`` the weighted field [B, lon, lat, C].  Both are differentiable in ``pred`` (sign(0) = 0: tied members
    contribute exactly zero); ``target`` gets no gradient.  fp32 device tensors only; the kernels are csrc/gw_crps.hip."""

    def __init__(self, grid_lat: Optional[torch.Tensor] = None, features_weights: Optional[torch.Tensor] = None, alpha: float = 1.0,
                 reduction: str = "mean"):
        super().__init__()
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1], got {alpha}.")
        if reduction not in ("mean", "none"):
            raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}.")
        area_weights = None
        if grid_lat is not None:  # |cos(latitude)|, normalised to mean 1
            grid_lat = torch.as_tensor(grid_lat, dtype=torch.float32)
            area_weights = torch.abs(torch.cos(grid_lat * np.pi / 180.0))
            area_weights = area_weights / torch.mean(area_weights)
        if features_weights is not None:
            features_weights = torch.as_tensor(features_weights, dtype=torch.float32).clone()
        self.alpha = float(alpha)
        self.reduction = reduction
        self.register_buffer("area_weights", area_weights, persistent=False)
        self.register_buffer("features_weights", features_weights, persistent=False)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if pred.dim() != 5:
            raise ValueError(f"The expected shape for predictions is [batch, ensemble, lon, lat, var], but got {tuple(pred.shape)}.")
        if tuple(target.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
            raise ValueError("The target must have the shape of the predictions without the ensemble axis. The actual shapes are "
                             f"{tuple(pred.shape)} and {tuple(target.shape)}.")
        if pred.shape[1] == 1 and self.alpha > 0:
            raise ValueError(f"The fair score (alpha = {self.alpha} > 0) needs at least two ensemble members, got 1; use alpha=0.")
        if self.area_weights is not None and self.area_weights.numel() != pred.shape[3]:
            raise ValueError(f"The size of grid_lat at initialization ({self.area_weights.numel()}) and the number of latitudes in "
                             f"predictions ({pred.shape[3]}) don't match.")
        if self.features_weights is not None and self.features_weights.numel() != pred.shape[4]:
            raise ValueError(f"The size of features weights at initialization ({self.features_weights.numel()}) and the number of "
                             f"features in predictions ({pred.shape[4]}) don't match.")
        if torch.is_grad_enabled() and target.requires_grad:
            raise NotImplementedError("graph_weather_amd: EnsembleCRPSLoss has no gradient for target (only for pred)")
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("graph_weather_amd: pred and target must be on a HIP device - there is no CPU path")
        aw = None if self.area_weights is None else self.area_weights.to(device=pred.device, dtype=torch.float32).reshape(-1).contiguous()
        fw = None if self.features_weights is None else self.features_weights.to(device=pred.device, dtype=torch.float32).reshape(-1).contiguous()
        p, t = pred.contiguous(), target.detach().contiguous()
        if torch.is_grad_enabled() and pred.requires_grad:
            from .autograd import EnsembleCRPSFunction

            return EnsembleCRPSFunction.apply(p, t, aw, fw, self.alpha, self.reduction)
        return ops.ensemble_crps_forward(p, t, aw, fw, self.alpha, self.reduction)
