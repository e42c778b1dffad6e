"""A restatement of the reference's Aurora files (graph_weather/models/aurora/: model, encoder, processor, decoder), written
from their arithmetic as plain torch compositions over a ``state_dict``: float64 for the oracle, float32 on the CPU for the
yardstick (what fp32 arithmetic in the reference's own order of operations costs).  Nothing here touches the HIP kernels, and
nothing imports the reference, einops or ``torch.nn.MultiheadAttention``.

It also carries the per-key seeded ``fill_`` of tests/cafa_oracle.py (matrices and convolution weights ~ N(0, 1 / fan_in),
LayerNorm gains 1 + 0.25 N, every bias 0.1 N) and the case table of scripts/gen_aurora_golden.py.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .cafa_oracle import fill_, params  # noqa: F401  (re-exported)

RADIUS = 5.0  # degrees: EarthSystemLoss.spatial_correlation_loss
MAX_VALUE = 500.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def lattice(seed: int, n_lon: int = 12, n_lat: int = 9, spacing: float = 3.0, jitter: float = 0.1) -> np.ndarray:
    """[n_lon * n_lat, 2] (longitude, latitude) in degrees: a jittered lattice on which no pair lies within 0.05 degrees of the
    5 degree radius, so that a distance formed by a matrix product (the reference's cdist) and one formed from direct
    differences put every pair on the same side of it.  That is a condition on the inputs, not a tolerance."""
    rs = np.random.RandomState(seed)
    lon, lat = np.meshgrid((np.arange(n_lon) - (n_lon - 1) / 2) * spacing, (np.arange(n_lat) - (n_lat - 1) / 2) * spacing, indexing="ij")
    pts = np.stack([lon.ravel(), lat.ravel()], axis=-1) + rs.uniform(-jitter, jitter, (n_lon * n_lat, 2))
    pts = pts.astype(np.float32)
    d = np.sqrt(((pts[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(-1))
    assert np.abs(d - RADIUS).min() > 0.05, "a pair of points lies too close to the radius"
    return pts


# name -> (kind, constructor keywords, input description, seed)
MODEL_CFG = dict(input_features=5, output_features=3, latent_dim=64, num_layers=2)
PERCEIVER_CFG = dict(input_dim=24, latent_dim=40, d_model=32, num_self_attention_layers=2, num_attention_heads=4)
CASES = {
    "aurora_model_b1": ("model", MODEL_CFG, dict(batch=1, n=108, mask=False), 21),
    "aurora_model_b2_mask": ("model", MODEL_CFG, dict(batch=2, n=108, mask=True), 22),
    "aurora_loss_n108": ("loss", dict(alpha=0.5, beta=0.3, gamma=0.2), dict(batch=1, n=108, channels=3), 23),
    "aurora_swin_3x4x5": ("swin", dict(in_channels=2, embed_dim=32), dict(shape=(2, 2, 3, 4, 5)), 24),
    "aurora_perceiver": ("perceiver", PERCEIVER_CFG, dict(batch=2, seq=60, mask=False), 25),
    "aurora_perceiver_mask": ("perceiver", PERCEIVER_CFG, dict(batch=2, seq=60, mask=True), 26),
    "aurora_decoder_3x4x5": ("decoder", dict(output_channels=2, embed_dim=32, target_shape=(3, 4, 5)), dict(batch=2), 27),
}


def case_inputs(name: str) -> Dict[str, torch.Tensor]:
    kind, cfg, spec, seed = CASES[name]
    rs = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))  # noqa: E731
    if kind == "model":
        b, n = spec["batch"], spec["n"]
        out = {"points": f32(np.stack([lattice(seed + 100 * i) for i in range(b)])),
               "features": f32(rs.standard_normal((b, n, cfg["input_features"])))}
        if spec["mask"]:
            out["mask"] = torch.from_numpy(rs.uniform(size=(b, n)) > 0.25)
        return out
    if kind == "loss":
        n, c = spec["n"], spec["channels"]
        pred = 250.0 + 200.0 * rs.standard_normal((1, n, c))  # some values below 0 and some above 500: every physical term is active
        return {"pred": f32(pred), "target": f32(pred + 5.0 * rs.standard_normal((1, n, c))), "points": f32(lattice(seed)[None])}
    if kind == "swin":
        return {"x": f32(rs.standard_normal(spec["shape"]))}
    if kind == "perceiver":
        b, s = spec["batch"], spec["seq"]
        out = {"x": f32(rs.standard_normal((b, s, cfg["input_dim"])))}
        if spec["mask"]:
            mask = np.ones((b, s), dtype=bool)
            mask[1, 40:] = False  # one sample with the keys 40.. padded
            out["attention_mask"] = torch.from_numpy(mask)
        return out
    if kind == "decoder":
        d, h, w = cfg["target_shape"]
        return {"x": f32(rs.standard_normal((spec["batch"], d * h * w, cfg["embed_dim"])))}
    raise KeyError(kind)


def build(pkg, name: str):
    """(module of ``pkg`` in eval() with the seeded parameters, or the loss module) of a case; ``pkg`` has the reference's names."""
    kind, cfg, _, seed = CASES[name]
    if kind == "model":
        return fill_(pkg.AuroraModel(**cfg), seed).eval()
    if kind == "loss":
        return pkg.EarthSystemLoss(**cfg)
    if kind == "swin":
        return fill_(pkg.Swin3DEncoder(**cfg), seed).eval()
    if kind == "perceiver":
        return fill_(pkg.PerceiverProcessor(pkg.ProcessorConfig(**cfg)), seed).eval()
    if kind == "decoder":
        return fill_(pkg.Decoder3D(**cfg), seed).eval()
    raise KeyError(kind)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def linear(p, key, x):
    return x @ p[key + ".weight"].T + p[key + ".bias"]


def layer_norm(p, key, x):
    return F.layer_norm(x, (x.shape[-1],), p[key + ".weight"], p[key + ".bias"], 1e-5)


def self_attention(p, key, x, heads: int, key_bias: Optional[torch.Tensor] = None):
    """torch's multi-head self-attention on x [batch, seq, embed]; key_bias [batch, seq] is added to the scores of every query."""
    b, s, e = x.shape
    d = e // heads
    qkv = x @ p[key + ".in_proj_weight"].T + p[key + ".in_proj_bias"]
    q, k, v = (t.reshape(b, s, heads, d).permute(0, 2, 1, 3) for t in qkv.split(e, dim=-1))
    sim = (q * d**-0.5) @ k.transpose(-1, -2)
    if key_bias is not None:
        sim = sim + key_bias[:, None, None, :].to(sim.dtype)
    out = (sim.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(b, s, e)
    return linear(p, key + ".out_proj", out)


def encoder_layer(p, key, x, heads: int, act, key_bias=None):
    """A post-norm nn.TransformerEncoderLayer in eval()."""
    x = layer_norm(p, key + ".norm1", x + self_attention(p, key + ".self_attn", x, heads, key_bias))
    return layer_norm(p, key + ".norm2", x + linear(p, key + ".linear2", act(linear(p, key + ".linear1", x))))


def point_branch(p, key, x):
    h = F.relu(layer_norm(p, key + ".1", linear(p, key + ".0", x)))
    return linear(p, key + ".3", h)


def aurora_model(p, points, features, mask, cfg):
    if mask is not None:
        m = mask.to(points.dtype).unsqueeze(-1)
        points, features = points * m, features * m
    normalized = torch.stack([points[..., 0] / 180.0, points[..., 1] / 90.0], dim=-1)
    x = point_branch(p, "encoder.coord_encoder", normalized) + point_branch(p, "encoder.feature_encoder", features)
    x = layer_norm(p, "encoder.norm", x)
    for i in range(cfg["num_layers"]):
        key = "processor.layers.%d" % i
        x = layer_norm(p, key + ".norm1", x + self_attention(p, key + ".attention", x, 8))
        x = layer_norm(p, key + ".norm2", x + linear(p, key + ".ffn.2", F.relu(linear(p, key + ".ffn.0", x))))
    out = linear(p, "decoder.decoder.2", F.relu(linear(p, "decoder.decoder.0", x)))
    return out if mask is None else out * m


def earth_loss(pred, target, points, alpha: float, beta: float, gamma: float):
    """The four values of EarthSystemLoss.forward (batch 1), distances from direct differences."""
    assert pred.shape[0] == 1
    mse = ((pred - target) ** 2).mean()
    pts = points[0]
    dist2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    near = (dist2 < RADIUS**2).to(pred.dtype)[None, :, :, None]
    e = pred - target
    spatial = (near * (e.unsqueeze(2) - e.unsqueeze(1)) ** 2).mean()
    physical = physical_loss(pred, points)
    return {"total_loss": alpha * mse + beta * spatial + gamma * physical, "mse_loss": mse, "spatial_correlation_loss": spatial,
            "physical_loss": physical}


def physical_loss(pred, points):
    lat = points[..., 1].abs()
    consistency = F.relu(pred[..., 0] - (1.0 - lat / 90.0) * pred.mean()).mean()
    return F.relu(-pred).mean() + F.relu(pred - MAX_VALUE).mean() + 0.1 * consistency


LOSS_KEYS = ("total_loss", "mse_loss", "spatial_correlation_loss", "physical_loss")


def conv3d(p, key, x):
    return F.conv3d(x, p[key + ".weight"], p[key + ".bias"], padding=1)


def conv_transpose3d(p, key, x):
    return F.conv_transpose3d(x, p[key + ".weight"], p[key + ".bias"], padding=1)


def swin_encoder(p, x):
    """[b, c, d, h, w] -> [b, d h w, embed_dim]: conv1, norm, the four encoder layers (ReLU) and the encoder's final norm."""
    x = conv3d(p, "conv1", x).permute(0, 2, 3, 4, 1)
    b, d, h, w, c = x.shape
    x = layer_norm(p, "norm", x).reshape(b, d * h * w, c)
    for i in range(4):
        x = encoder_layer(p, "swin_transformer.encoder.layers.%d" % i, x, 8, F.relu)
    return layer_norm(p, "swin_transformer.encoder.norm", x)


def perceiver(p, x, attention_mask, cfg):
    key_bias = None
    if attention_mask is not None:
        key_bias = torch.zeros(attention_mask.shape, dtype=x.dtype).masked_fill(~attention_mask, float("-inf"))
    x = linear(p, "input_projection", x)
    for i in range(cfg["num_self_attention_layers"]):
        x = encoder_layer(p, "encoder.layers.%d" % i, x, cfg["num_attention_heads"], F.gelu, key_bias)
    return linear(p, "output_projection", x).mean(dim=1)


def decoder3d(p, x, cfg):
    d, h, w = cfg["target_shape"]
    return conv_transpose3d(p, "deconv1", x.reshape(x.shape[0], cfg["embed_dim"], d, h, w))


def run(name: str, p, inputs: Dict[str, torch.Tensor], dtype=torch.float64):
    """The restatement of a case on ``inputs`` (converted to ``dtype``; masks stay boolean): a tensor, or [4] for the loss."""
    kind, cfg, _, _ = CASES[name]
    t = {k: (v if v.dtype == torch.bool else v.to(dtype)) for k, v in inputs.items()}
    if kind == "model":
        return aurora_model(p, t["points"], t["features"], t.get("mask"), cfg)
    if kind == "loss":
        out = earth_loss(t["pred"], t["target"], t["points"], **cfg)
        return torch.stack([out[k] for k in LOSS_KEYS])
    if kind == "swin":
        return swin_encoder(p, t["x"])
    if kind == "perceiver":
        return perceiver(p, t["x"], t.get("attention_mask"), cfg)
    if kind == "decoder":
        return decoder3d(p, t["x"], cfg)
    raise KeyError(kind)
