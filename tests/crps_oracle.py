"""The broadcasting restatement of ``EnsembleCRPSLoss`` in torch ops, in a chosen dtype: float64 is the reference, float32 on the CPU
the yardstick.  It forms the [B, N, N, lon, lat, C] differences the kernels avoid.  Touches no product code.

    v = (1/N) sum_i |x_i - y| - c2 sum_i sum_j |x_i - x_j|,   c2 = alpha / (2 N (N-1)) + (1 - alpha) / (2 N^2)   (0 at N = 1)

weighted by |cos(grid_lat)| normalised to mean 1 and by ``features_weights``; the gradients come from autograd (``torch.abs`` has
sign(0) = 0)."""
import math

import numpy as np
import torch


def c2(n, alpha):
    return alpha / (2.0 * n * (n - 1)) + (1.0 - alpha) / (2.0 * n * n) if n > 1 else 0.0


def weights(grid_lat, features_weights, dtype):
    """(area_weights [lat] or None, features_weights [C] or None) in ``dtype``, formed as the loss forms them (in float32)."""
    aw = fw = None
    if grid_lat is not None:
        aw = torch.abs(torch.cos(torch.as_tensor(grid_lat, dtype=torch.float32) * np.pi / 180.0))
        aw = (aw / torch.mean(aw)).to(dtype)
    if features_weights is not None:
        fw = torch.as_tensor(features_weights, dtype=torch.float32).to(dtype)
    return aw, fw


def field(pred, target, grid_lat=None, features_weights=None, alpha=1.0, dtype=torch.float64):
    """The weighted score [B, lon, lat, C] of pred [B, N, lon, lat, C] against target [B, lon, lat, C] (differentiable)."""
    x, y = pred.to(dtype), target.to(dtype)
    n = x.shape[1]
    v = (x - y[:, None]).abs().sum(1) / n - c2(n, alpha) * (x[:, :, None] - x[:, None]).abs().sum((1, 2))
    aw, fw = weights(grid_lat, features_weights, dtype)
    if aw is not None:
        v = v * aw[None, None, :, None]
    if fw is not None:
        v = v * fw
    return v


def loss(pred, target, grid_lat=None, features_weights=None, alpha=1.0, reduction="mean", dtype=torch.float64):
    v = field(pred, target, grid_lat, features_weights, alpha, dtype)
    return v.mean() if reduction == "mean" else v


def loss_and_grad(pred, target, grid_lat=None, features_weights=None, alpha=1.0, reduction="mean", dtype=torch.float64, dout=None):
    """(value, dpred) in ``dtype``; ``dout`` [B, lon, lat, C] is the upstream gradient of the field ("none"; default ones)."""
    x = pred.detach().to(dtype).requires_grad_(True)
    out = loss(x, target.detach(), grid_lat, features_weights, alpha, reduction, dtype)
    if reduction == "mean":
        out.backward()
    else:
        out.backward(torch.ones_like(out) if dout is None else dout.to(dtype))
    return out.detach(), x.grad


def triple_loop(pred, target, alpha):
    """The unweighted score by plain Python loops over floats: [B, lon, lat, C] as nested lists flattened to a float64 tensor."""
    B, N, LON, LAT, C = pred.shape
    out = torch.zeros(B, LON, LAT, C, dtype=torch.float64)
    for b in range(B):
        for lo in range(LON):
            for la in range(LAT):
                for c in range(C):
                    xs = [float(pred[b, i, lo, la, c]) for i in range(N)]
                    y = float(target[b, lo, la, c])
                    s1 = math.fsum(abs(xi - y) for xi in xs)
                    s2 = math.fsum(abs(xi - xj) for xi in xs for xj in xs)
                    out[b, lo, la, c] = s1 / N - c2(N, alpha) * s2
    return out
