"""The reference's two per-channel modulation layers on ``[B, C, *spatial]`` activations, on the HIP kernels of
``csrc/gw_modulate.hip``: ``StochasticDecompositionLayer`` (``graph_weather/models/layers/stochastic_decomposition.py``,
ensemble noise) and ``FiLMGenerator`` / ``FiLMApplier`` (``layers/film.py``, lead-time conditioning).  Same constructor
signatures, same ``state_dict`` keys.  The streaming part of each layer is one fused launch each way; the small dense parts
(``style_net``, the generator's two Linears) run through ``gw_linear_forward`` and its autograd node (``wide._Linear``).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops


def _activation(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 on a HIP device, dense (a ``.contiguous()`` copy where it is not)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"graph_weather_amd: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"graph_weather_amd: {name} must live on a HIP device (no CPU path exists)")
    if t.dtype != torch.float32:
        raise TypeError(f"graph_weather_amd: {name} must be float32, got {t.dtype}")
    return t.contiguous()


def _linear(x: torch.Tensor, lin: nn.Linear, relu: bool) -> torch.Tensor:
    from .wide import _Linear, linear_forward

    if not lin.weight.is_cuda:
        raise RuntimeError("graph_weather_amd: the layer's parameters must live on a HIP device (no CPU path exists)")
    if torch.is_grad_enabled() and (x.requires_grad or lin.weight.requires_grad or (lin.bias is not None and lin.bias.requires_grad)):
        return _Linear.apply(x, lin.weight, lin.bias, relu)
    return linear_forward(x, lin.weight.detach(), None if lin.bias is None else lin.bias.detach(), relu)


class StochasticDecompositionLayer(nn.Module):
    """stochastic_decomposition.py:26-68: ``x + alpha * style_net(z) * eps`` with eps ~ N(0, 1) per element.

    The noise is not drawn into memory: the kernel makes it in registers from a 64-bit key and the flat element index
    (Philox4x32-10 + Box-Muller, include/gw_amd.h; |eps| <= 5.89) and the backward makes it again, so nothing of the size of
    ``x`` is saved.  The key comes from torch's generator of the device (``ops.sdl_key``): ``torch.manual_seed`` reproduces
    the output, successive calls differ and a captured graph draws fresh noise on every replay.  ``noise=`` (shaped like
    ``x``) replaces the generated noise - for parity tests and for common random numbers across ensemble members."""

    def __init__(self, input_dim: int, latent_dim: int):
        super().__init__()
        self.input_dim = input_dim
        self.latent_dim = latent_dim
        self.alpha = nn.Parameter(torch.zeros(1, input_dim, 1))
        self.style_net = nn.Linear(latent_dim, input_dim)

    def forward(self, x: torch.Tensor, z: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x.dim() < 3:
            raise ValueError(f"Expected [Batch, Channels, *Spatial] with at least one spatial dimension, got {tuple(x.shape)}")
        if x.size(1) != self.input_dim:
            raise ValueError(f"Expected {self.input_dim} channels, got {x.size(1)}")
        x, z = _activation(x, "x"), _activation(z, "z")
        if z.dim() != 2 or z.shape[0] != x.shape[0] or z.shape[1] != self.latent_dim:
            raise ValueError(f"Expected z of shape [{x.shape[0]}, {self.latent_dim}], got {tuple(z.shape)}")
        if noise is not None:
            noise = _activation(noise, "noise").detach()
            if noise.shape != x.shape:
                raise ValueError(f"Expected noise shaped like x {tuple(x.shape)}, got {tuple(noise.shape)}")
        style = _linear(z, self.style_net, False)  # [B, C]
        key = ops.sdl_key(x.device) if noise is None else None
        if torch.is_grad_enabled() and (x.requires_grad or style.requires_grad or self.alpha.requires_grad):
            from .autograd import StochasticDecompositionFunction

            return StochasticDecompositionFunction.apply(x, style, self.alpha, key, noise)
        return ops.sdl_forward(x, style, self.alpha.detach(), key, noise)


class FiLMGenerator(nn.Module):
    """film.py:5-48: (gamma, beta), each ``[batch_size, feature_dim]``, from a lead-time index.  The reference feeds a one-hot
    row per batch element through ``network``; so does this (the rows are built on the device, the two Linears are HIP
    GEMMs).  ``device`` defaults to the device of the parameters."""

    def __init__(self, num_lead_times: int, hidden_dim: int, feature_dim: int):
        super().__init__()
        self.num_lead_times = num_lead_times
        self.feature_dim = feature_dim
        self.network = nn.Sequential(
            nn.Linear(num_lead_times, hidden_dim),
            nn.ReLU(),
            nn.Linear(hidden_dim, 2 * feature_dim),
        )

    def forward(self, batch_size: int, lead_time: int, device=None):
        lead_time = int(lead_time)
        if not -self.num_lead_times <= lead_time < self.num_lead_times:
            raise IndexError(f"index {lead_time} is out of bounds for dimension 1 with size {self.num_lead_times}")
        device = self.network[0].weight.device if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("graph_weather_amd: FiLMGenerator must run on a HIP device (no CPU path exists)")
        one_hot = torch.zeros(batch_size, self.num_lead_times, device=device)
        one_hot[:, lead_time] = 1.0
        gamma_beta = _linear(_linear(one_hot, self.network[0], True), self.network[2], False)
        return gamma_beta[:, : self.feature_dim], gamma_beta[:, self.feature_dim:]


class FiLMApplier(nn.Module):
    """film.py:51-75: ``x * gamma + beta`` with gamma / beta ``[B, C]`` broadcast over every trailing dimension of ``x``."""

    def forward(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
        x, gamma, beta = _activation(x, "x"), _activation(gamma, "gamma"), _activation(beta, "beta")
        if x.dim() < 2 or gamma.shape != x.shape[:2] or beta.shape != x.shape[:2]:
            raise ValueError(f"Expected gamma and beta of shape {tuple(x.shape[:2])} for x {tuple(x.shape)}, got "
                             f"{tuple(gamma.shape)} and {tuple(beta.shape)}")
        if torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad or beta.requires_grad):
            from .autograd import FiLMFunction

            return FiLMFunction.apply(x, gamma, beta)
        return ops.film_forward(x, gamma, beta)
