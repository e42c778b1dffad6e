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


# ----------------------------------------------------------------------------------------------------------------------------
# The same operations one by one on NHWC pixel rows [B * H * W, C] (row (b * H + y) * W + x), in the dtype of their arguments,
# built from the F.* calls above so that autograd gives every gradient.  tests/test_thermalizer_host.py composes them into
# ``score`` / ``thermalize``; tests/test_gpu_thermal_kernels.py holds each kernel of csrc/gw_thermal.hip against one of them.
# ----------------------------------------------------------------------------------------------------------------------------


def to_image(rows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return rows.reshape(B, H, W, rows.shape[-1]).permute(0, 3, 1, 2)


def to_rows(img: torch.Tensor) -> torch.Tensor:
    B, C, H, W = img.shape
    return img.permute(0, 2, 3, 1).reshape(B * H * W, C)


def conv_rows(x, w, b, B: int, H: int, W: int):
    """Conv2d(w [co, ci, k, k], padding k // 2), any odd k."""
    return to_rows(F.conv2d(to_image(x, B, H, W), w, b, padding=int(w.shape[-1]) // 2))


def conv_transpose_rows(x, w, b, B: int, H: int, W: int):
    """ConvTranspose2d(w [ci, co, 3, 3], stride 2, padding 1, output_padding 1): rows of the 2H x 2W image."""
    return to_rows(F.conv_transpose2d(to_image(x, B, H, W), w, b, stride=2, padding=1, output_padding=1))


def group_norm_stats(x, gamma, beta, B: int, groups: int, eps: float = 1e-5):
    """(mean [B, G], rstd [B, G], scale [B, C], shift [B, C]) of GroupNorm over the rows of each sample: the statistics are
    those F.group_norm computes (torch.native_group_norm, the operator behind it: F.group_norm returns no statistics and refuses
    one value per channel; should a torch release drop that operator, mean / var(unbiased=False) over each group are the
    same numbers), and y = x * scale + shift."""
    C = x.shape[-1]
    hw = x.shape[0] // B
    img = x.reshape(B, hw, C).permute(0, 2, 1).contiguous()
    _, mean, rstd = torch.native_group_norm(img, gamma, beta, B, C, hw, groups, eps)
    scale = gamma.reshape(1, groups, -1) * rstd.reshape(B, groups, 1)
    shift = beta.reshape(1, groups, -1) - mean.reshape(B, groups, 1) * scale
    return mean, rstd, scale.reshape(B, C), shift.reshape(B, C)


def group_norm_rows(x, gamma, beta, B: int, groups: int, eps: float = 1e-5):
    """GroupNorm before its ReLU (the pre-activation whose sign is the backward mask)."""
    C = x.shape[-1]
    hw = x.shape[0] // B
    img = x.reshape(B, hw, C).permute(0, 2, 1).contiguous()
    # (what F.group_norm calls; F.group_norm itself refuses a single value per channel, which the kernel tests include)
    return torch.native_group_norm(img, gamma, beta, B, C, hw, groups, eps)[0].permute(0, 2, 1).reshape(B * hw, C)


def gn_relu_rows(x, gamma, beta, B: int, groups: int, eps: float = 1e-5):
    return F.relu(group_norm_rows(x, gamma, beta, B, groups, eps))


def affine_relu_rows(x, scale, shift, B: int):
    """relu(x * scale[b] + shift[b]) with per-(sample, channel) scale and shift [B, C]: the GroupNorm + ReLU operand load."""
    C = x.shape[-1]
    return F.relu(x.reshape(B, -1, C) * scale.reshape(B, 1, C) + shift.reshape(B, 1, C)).reshape(-1, C)


def max_pool_rows(x, B: int, H: int, W: int):
    """MaxPool2d(3, 2, 1): (rows of the pooled image, indices y * W + x of the winners in the same layout)."""
    y, idx = F.max_pool2d(to_image(x, B, H, W), 3, 2, 1, return_indices=True)
    return to_rows(y), to_rows(idx)


def resize_rows(x, B: int, H: int, W: int, Ho: int, Wo: int):
    return to_rows(F.interpolate(to_image(x, B, H, W), size=(Ho, Wo), mode="bilinear", align_corners=False))


def colsum_rows(x):
    return x.sum(0)


def rows_finalize(x, eps, eps_hat, sa: float, s1: float):
    """(noisy - s1 * eps_hat) / sa with noisy = sa * x + s1 * eps."""
    return ((sa * x + s1 * eps) - s1 * eps_hat) / sa


def rows_scale(p, sa: float):
    return sa * p


def rows_axpy(p, q, sa: float):
    return p + sa * q


def diffuse_rows(x, eps, sa: float, s1: float, B: int, H: int, W: int):
    """The score model's input as ``thermalize`` builds it: sa * x + s1 * eps, the x coordinate, the y coordinate."""
    noisy = sa * x + s1 * eps
    ys = torch.linspace(0, 1, H, dtype=x.dtype, device=x.device).view(1, H, 1, 1).expand(B, H, W, 1)
    xs = torch.linspace(0, 1, W, dtype=x.dtype, device=x.device).view(1, 1, W, 1).expand(B, H, W, 1)
    return torch.cat([noisy, xs.reshape(-1, 1), ys.reshape(-1, 1)], 1)


def _block_rows(sd, p: str, x, B: int, H: int, W: int, expand: bool):
    for i, j in ((0, 1), (3, 4)):
        w = sd[f"{p}.{i}.weight"]
        x = conv_rows(x, w, sd[f"{p}.{i}.bias"], B, H, W)
        x = gn_relu_rows(x, sd[f"{p}.{j}.weight"], sd[f"{p}.{j}.bias"], B, min(8, int(w.shape[0])))
    if expand:
        return conv_transpose_rows(x, sd[f"{p}.6.weight"], sd[f"{p}.6.bias"], B, H, W)
    return max_pool_rows(x, B, H, W)[0]


def score_rows(sd: Dict[str, torch.Tensor], x, B: int, H: int, W: int):
    """``score`` composed from the per-operation helpers, rows in -> rows out."""
    if min(H, W) <= 4:
        h = x
        for i, j in ((0, 1), (3, 4), (6, 7)):
            h = conv_rows(h, sd[f"simple_net.{i}.weight"], sd[f"simple_net.{i}.bias"], B, H, W)
            h = gn_relu_rows(h, sd[f"simple_net.{j}.weight"], sd[f"simple_net.{j}.bias"], B, 8)
        return conv_rows(h, sd["simple_net.9.weight"], sd["simple_net.9.bias"], B, H, W)
    pooled = lambda n: (n - 1) // 2 + 1
    H1, W1 = pooled(H), pooled(W)
    H2, W2 = pooled(H1), pooled(W1)
    H3, W3 = pooled(H2), pooled(W2)
    c1 = _block_rows(sd, "conv1", x, B, H, W, False)
    c2 = _block_rows(sd, "conv2", c1, B, H1, W1, False)
    c3 = _block_rows(sd, "conv3", c2, B, H2, W2, False)
    u = _block_rows(sd, "upconv3", c3, B, H3, W3, True)
    if (2 * H3, 2 * W3) != (H2, W2):
        u = resize_rows(u, B, 2 * H3, 2 * W3, H2, W2)
    u = _block_rows(sd, "upconv2", torch.cat([u, c2], 1), B, H2, W2, True)
    if (2 * H2, 2 * W2) != (H1, W1):
        u = resize_rows(u, B, 2 * H2, 2 * W2, H1, W1)
    u = _block_rows(sd, "upconv1", torch.cat([u, c1], 1), B, H1, W1, True)
    if (2 * H1, 2 * W1) != (H, W):
        u = resize_rows(u, B, 2 * H1, 2 * W1, H, W)
    return u


def thermalize_rows(sd: Dict[str, torch.Tensor], rows, noise, t: int, B: int, H: int, W: int):
    """``thermalize`` composed from the per-operation helpers."""
    sa, s1 = coefficients(t)
    noise = noise.to(rows.dtype)
    eps_hat = score_rows(sd, diffuse_rows(rows, noise, sa, s1, B, H, W), B, H, W)
    return rows_finalize(rows, noise, eps_hat, sa, s1)
