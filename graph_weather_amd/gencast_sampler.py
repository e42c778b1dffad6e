"""GenCast's ``Sampler`` (graph_weather/models/gencast/sampler.py of the reference) and ``WeightedMSELoss``
(weighted_mse_loss.py).

``Sampler``: same constructor, defaults, attribute names and ``_sigmas_fn``.  ``sample`` is the reference's loop - DPMSolver++2S
with Karras' stochastic churn and noise inflation, a final Euler step - without its device reads: the schedule is computed once on
the host, every noise level goes to the device in one tensor, the coefficients of the state updates are host scalars handed to
one elementwise kernel (``gw_gencast_sampler_combine``), the noise is drawn on the device (``generate_isotropic_noise``) and the
Denoiser is entered behind its checks.  ``prev_inputs`` may hold an ensemble of B >= 1 samples (the reference's loop takes 1).

``WeightedMSELoss``: same constructor, buffers and error messages; one reduction kernel forward, one elementwise kernel backward.
fp32 device tensors only.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .gencast_model import Denoiser, generate_isotropic_noise

__all__ = ["Sampler", "WeightedMSELoss"]


class Sampler:
    """Sampler for the denoiser: the second-order DPMSolver++2S solver (Lu et al., 2022) with the stochastic churn and noise
    inflation of Karras et al. (2022), conditioned on the previous two timesteps."""

    def __init__(self, S_noise: float = 1.05, S_tmin: float = 0.75, S_tmax: float = 80.0, S_churn: float = 2.5, r: float = 0.5,
                 sigma_max: float = 80.0, sigma_min: float = 0.03, rho: float = 7, num_steps: int = 20):
        self.S_noise = S_noise
        self.S_tmin = S_tmin
        self.S_tmax = S_tmax
        self.S_churn = S_churn
        self.r = r
        self.num_steps = num_steps

        self.sigma_max = sigma_max
        self.sigma_min = sigma_min
        self.rho = rho

    def _sigmas_fn(self, u):
        return (
            self.sigma_max ** (1 / self.rho)
            + u * (self.sigma_min ** (1 / self.rho) - self.sigma_max ** (1 / self.rho))
        ) ** self.rho

    def _schedule(self):
        """The loop's scalars, computed once with torch float32 CPU tensors in the reference's order of operations and returned as
        Python floats: (sigmas, gammas, steps), one dict per step.

        The reference evaluates the same expressions on ``prev_inputs.device``; its churn test ``S_tmin <= sigmas[i] <= S_tmax``
        sits on a rounding boundary at the defaults (``sigmas[0]`` is 79.99998474 in float32 on the CPU; a device's ``pow`` need
        not round the same way).  This is the reference's CPU result: step 0 churns; with the default sigma range the gammas are 14 x
        0.125 then 5 x 0 for ``num_steps=20`` and 3 x (sqrt(2) - 1) then 0 for ``num_steps=5``."""
        time_steps = torch.arange(0, self.num_steps) / (self.num_steps - 1)
        sigmas = self._sigmas_fn(time_steps)
        gammas, steps = [], []
        for i in range(len(sigmas) - 1):
            gamma = (
                min(self.S_churn / self.num_steps, math.sqrt(2) - 1)
                if self.S_tmin <= sigmas[i] <= self.S_tmax
                else 0.0
            )
            gammas.append(float(gamma))
            sigma_hat = sigmas[i] * (gamma + 1)
            st = dict(sigma_hat=sigma_hat.item(), sigma_mid=sigma_hat.item(), churn=0.0)
            if gamma > 0:
                st["churn"] = ((sigma_hat**2 - sigmas[i] ** 2) ** 0.5).item()
            if i == len(sigmas) - 2:
                # x + (x - denoised) / sigma_hat * (sigma_next - sigma_hat)
                t = ((sigmas[i + 1] - sigma_hat) / sigma_hat).item()
                st.update(euler=(1.0 + t, -t))
            else:
                lambda_hat = -torch.log(sigma_hat)
                lambda_next = -torch.log(sigmas[i + 1])
                h = lambda_next - lambda_hat
                lambda_mid = lambda_hat + self.r * h
                sigma_mid = torch.exp(-lambda_mid)
                e_h = (torch.exp(-h) - 1).item()
                st.update(sigma_mid=sigma_mid.item(),
                          u=((sigma_mid / sigma_hat).item(), -(torch.exp(-self.r * h) - 1).item()),
                          x=((sigmas[i + 1] / sigma_hat).item(), -e_h * (1 - 1 / (2 * self.r)), -e_h * (1 / (2 * self.r))))
            steps.append(st)
        return [s.item() for s in sigmas], gammas, steps

    @torch.no_grad()
    def sample(self, denoiser: Denoiser, prev_inputs: torch.Tensor, generator: Optional[torch.Generator] = None,
               coeffs: Optional[Sequence[torch.Tensor]] = None):
        """Generate samples from random noise for the given inputs.

        Args:
            denoiser (Denoiser): the denoiser model.
            prev_inputs (torch.Tensor): previous two timesteps [B, lon, lat, 2 in]; every sample of the batch gets its own noise.
            generator: the device generator of the noise draws (the same seed gives a bitwise equal result).
            coeffs: ``num_steps`` complex64 tensors [B * out, lmax, lmax + 1] to use instead of the draws: the initial noise, then
                steps 0 .. num_steps - 2 in order (the last one belongs to the Euler step, which draws and may not use it).

        Returns:
            torch.Tensor: normalized residuals predicted [B, lon, lat, out].
        """
        if not prev_inputs.is_cuda:
            raise RuntimeError("graph_weather_amd: prev_inputs must live on a HIP device (no CPU path exists)")
        if coeffs is not None and len(coeffs) != self.num_steps:
            raise ValueError(f"coeffs must hold num_steps = {self.num_steps} tensors, got {len(coeffs)}")
        device, B = prev_inputs.device, int(prev_inputs.shape[0])
        sigmas, _, steps = self._schedule()
        # sigma_hat and sigma_mid of every step ([2 (num_steps - 1), B, 1]), in one copy: slices [B, 1] are the Denoiser's noise_levels
        levels = torch.tensor([[st["sigma_hat"], st["sigma_mid"]] for st in steps], dtype=torch.float32).reshape(-1, 1, 1)
        levels = levels.expand(-1, B, 1).contiguous().to(device)
        draws = iter(coeffs) if coeffs is not None else None

        def draw():
            return generate_isotropic_noise(num_lon=denoiser.num_lon, num_lat=denoiser.num_lat, num_samples=denoiser.output_features_dim,
                                            device=device, generator=generator, batch=B, coeffs=None if draws is None else next(draws))

        x = draw()
        denoiser._check_shapes(x, prev_inputs, levels[0])
        prev_inputs = prev_inputs.contiguous()
        ops.sampler_combine(x, sigmas[0], x)
        u = torch.empty_like(x)
        for i, st in enumerate(steps):
            noise = draw()
            if st["churn"] > 0:
                ops.sampler_combine(x, 1.0, x, st["churn"] * self.S_noise, noise)
            denoised = denoiser._forward_impl(x, prev_inputs, levels[2 * i])
            if "euler" in st:
                ops.sampler_combine(x, st["euler"][0], x, st["euler"][1], denoised)
            else:
                ops.sampler_combine(u, st["u"][0], x, st["u"][1], denoised)
                denoised_2 = denoiser._forward_impl(u, prev_inputs, levels[2 * i + 1])
                ops.sampler_combine(x, st["x"][0], x, st["x"][1], denoised, st["x"][2], denoised_2)
        return x


class WeightedMSELoss(torch.nn.Module):
    """The loss described in GenCast's paper: squared residuals weighted by the area of the grid cell, the feature and the noise
    level, lambda(sigma) = (sigma^2 + sigma_data^2) / (sigma sigma_data)^2."""

    def __init__(self, grid_lat: Optional[torch.Tensor] = None, pressure_levels: Optional[torch.Tensor] = None,
                 num_atmospheric_features: Optional[int] = None, single_features_weights: Optional[torch.Tensor] = None):
        super().__init__()
        given = [v is not None for v in (pressure_levels, num_atmospheric_features, single_features_weights)]
        if any(given) and not all(given):
            raise ValueError("Please to use features weights provide all three: pressure_levels,"
                             "num_atmospheric_features and single_features_weights.")
        area_weights = features_weights = None
        if grid_lat is not None:  # |cos(latitude)|, normalised to mean 1
            area_weights = torch.abs(torch.cos(grid_lat * np.pi / 180.0))
            area_weights = area_weights / torch.mean(area_weights)
        if all(given):  # the pressure levels' shares for every atmospheric feature, then the single-level weights
            pressure_weights = pressure_levels / torch.sum(pressure_levels)
            features_weights = torch.cat((pressure_weights.repeat(num_atmospheric_features), single_features_weights), dim=-1)
        self.sigma_data = 1  # assuming normalized data!
        self.register_buffer("area_weights", area_weights, persistent=False)
        self.register_buffer("features_weights", features_weights, persistent=False)

    def _lambda_sigma(self, noise_level):
        noise_weights = (noise_level**2 + self.sigma_data**2) / (noise_level * self.sigma_data) ** 2
        return noise_weights  # [batch, 1]

    def forward(self, pred: torch.Tensor, noise_level: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """pred, target [batch, lon, lat, var], noise_level [batch, 1] -> the scalar loss.  The NaN check reads one flag from the
        device; it is skipped while the current stream is capturing."""
        if pred.shape != target.shape:
            raise ValueError(f"Predictions and targets must have same shape. The actual shapes are {pred.shape} and {target.shape}.")
        if pred.dim() != 4:
            raise ValueError(f"The expected shape for predictions and targets is [batch, lon, lat, var], but got {pred.shape}.")
        if noise_level.shape != (pred.shape[0], 1):
            raise ValueError(f"The expected shape for noise levels is [batch, 1], but got {noise_level.shape}.")
        if self.area_weights is not None and len(self.area_weights) != pred.shape[2]:
            raise ValueError(f"The size of grid_lat at initialization ({len(self.area_weights)}) and the number of latitudes in "
                             f"predictions ({pred.shape[2]}) don't match.")
        if self.features_weights is not None and len(self.features_weights) != pred.shape[-1]:
            raise ValueError(f"The size of features weights at initialization ({len(self.features_weights)}) and the number of "
                             f"features in predictions ({pred.shape[-1]}) don't match.")
        if not (pred.is_cuda and target.is_cuda and noise_level.is_cuda):
            raise RuntimeError("graph_weather_amd: pred, noise_level and target must be on a HIP device - there is no CPU path")
        if torch.is_grad_enabled() and target.requires_grad:
            raise NotImplementedError("graph_weather_amd: WeightedMSELoss has no gradient for target (only for pred)")
        aw = None if self.area_weights is None else self.area_weights.to(device=pred.device, dtype=torch.float32).contiguous()
        fw = None if self.features_weights is None else self.features_weights.to(device=pred.device, dtype=torch.float32).contiguous()
        p, t, s = pred.contiguous(), target.detach().contiguous(), noise_level.detach().contiguous()
        if torch.is_grad_enabled() and pred.requires_grad:
            from .autograd import WeightedMSEFunction

            loss, flag = WeightedMSEFunction.apply(p, t, s, aw, fw, float(self.sigma_data))
        else:
            loss, flag = ops.weighted_mse_forward(p, t, s, aw, fw, float(self.sigma_data))
        if not torch.cuda.is_current_stream_capturing() and flag.item():
            raise ValueError("NaN values encountered in loss calculation.")
        return loss
