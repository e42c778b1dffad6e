"""fp64 restatement of the reference thermalizer (graph_weather/models/layers/thermalizer.py) with torch CPU / device ops.

``score(sd, x)`` is AdaptiveUNet.forward on NCHW ``x``; ``thermalize(sd, rows, noise_rows, t, B, H, W)`` is
ThermalizerLayer.forward with the noise given as the rows the layer drew (``last_noise``).  ``sd`` holds the layer's (or the
score model's) parameters under their state_dict keys without the ``score_model.`` prefix.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

TIMESTEPS = 1000


def alphas_cumprod(timesteps: int = TIMESTEPS) -> torch.Tensor:
    x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / timesteps) + 0.008) / 1.008 * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)
    return torch.cumprod(1.0 - betas, 0)


def coefficients(t: int, timesteps: int = TIMESTEPS):
    ac = float(alphas_cumprod(timesteps)[min(max(int(t), 0), timesteps - 1)])
    return math.sqrt(ac), math.sqrt(1.0 - ac)


@torch.no_grad()
def fill_(module: torch.nn.Module, seed: int = 0) -> torch.nn.Module:
    """Per-key seeded weights of a sensible scale: conv kernels ~ N(0, 1 / fan_in), GroupNorm gains 1 + 0.1 N, biases 0.1 N."""
    for key, t in module.state_dict().items():
        if not t.is_floating_point():
            continue
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        n = rs.standard_normal(tuple(t.shape))
        if t.dim() == 4:
            fan_in = t.shape[1] * t.shape[2] * t.shape[3] if "upconv" not in key or not key.endswith("6.weight") else t.shape[0] * 9
            v = n / np.sqrt(fan_in)
        elif key.endswith("weight"):
            v = 1.0 + 0.1 * n
        else:
            v = 0.1 * n
        t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return module


def _block(sd: Dict[str, torch.Tensor], p: str, x, pad: int, expand: bool):
    for i, j in ((0, 1), (3, 4)):
        w = sd[f"{p}.{i}.weight"]
        x = F.conv2d(x, w, sd[f"{p}.{i}.bias"], padding=pad)
        c = w.shape[0]
        x = F.relu(F.group_norm(x, min(8, c), sd[f"{p}.{j}.weight"], sd[f"{p}.{j}.bias"], 1e-5))
    if expand:
        return F.conv_transpose2d(x, sd[f"{p}.6.weight"], sd[f"{p}.6.bias"], stride=2, padding=1, output_padding=1)
    return F.max_pool2d(x, 3, 2, 1)


def score(sd: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """AdaptiveUNet.forward (thermalizer.py) on NCHW x, in x's dtype."""
    H, W = x.shape[-2:]
    if min(H, W) <= 4:
        h = x
        for i, j in ((0, 1), (3, 4), (6, 7)):
            w = sd[f"simple_net.{i}.weight"]
            h = F.conv2d(h, w, sd[f"simple_net.{i}.bias"], padding=1)
            h = F.relu(F.group_norm(h, 8, sd[f"simple_net.{j}.weight"], sd[f"simple_net.{j}.bias"], 1e-5))
        return F.conv2d(h, sd["simple_net.9.weight"], sd["simple_net.9.bias"], padding=1)
    c1 = _block(sd, "conv1", x, 3, False)
    c2 = _block(sd, "conv2", c1, 1, False)
    c3 = _block(sd, "conv3", c2, 1, False)
    u = _block(sd, "upconv3", c3, 1, True)
    if u.shape[-2:] != c2.shape[-2:]:
        u = F.interpolate(u, size=c2.shape[-2:], mode="bilinear", align_corners=False)
    u = _block(sd, "upconv2", torch.cat([u, c2], 1), 1, True)
    if u.shape[-2:] != c1.shape[-2:]:
        u = F.interpolate(u, size=c1.shape[-2:], mode="bilinear", align_corners=False)
    u = _block(sd, "upconv1", torch.cat([u, c1], 1), 1, True)
    if u.shape[-2:] != (H, W):
        u = F.interpolate(u, size=(H, W), mode="bilinear", align_corners=False)
    return u


def thermalize(sd: Dict[str, torch.Tensor], rows: torch.Tensor, noise: torch.Tensor, t: int, B: int, H: int, W: int) -> torch.Tensor:
    """ThermalizerLayer.forward on rows [B * H * W, Fe] with the given noise rows, in rows' dtype."""
    Fe = rows.shape[1]
    sa, s1 = coefficients(t)
    x = rows.reshape(B, H, W, Fe).permute(0, 3, 1, 2)
    n = noise.to(rows.dtype).reshape(B, H, W, Fe).permute(0, 3, 1, 2)
    noisy = sa * x + s1 * n
    ys = torch.linspace(0, 1, H, dtype=rows.dtype, device=rows.device).view(1, 1, H, 1).expand(B, 1, H, W)
    xs = torch.linspace(0, 1, W, dtype=rows.dtype, device=rows.device).view(1, 1, 1, W).expand(B, 1, H, W)
    eps = score(sd, torch.cat([noisy, xs, ys], 1))
    pred = (noisy - s1 * eps) / sa
    return pred.permute(0, 2, 3, 1).reshape(B * H * W, Fe)


def strip(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
