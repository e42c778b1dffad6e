"""A restatement of the reference's FengWu-GHR file (graph_weather/models/fengwu_ghr/layers.py), written from its arithmetic
as plain torch compositions over a ``state_dict``: float64 for the oracle, float32 on the CPU for the yardstick (what fp32
arithmetic in the reference's own order of operations costs).  Nothing here touches the HIP kernels.

It also carries the tie rule of the neighbour assignment (per target the 4 sources smallest by (exact squared distance, source
index) - the reference's kd-tree leaves the order among equidistant sources open), a per-key seeded ``fill_`` (LayerNorm gains
away from 1, LayerNorm and Linear biases nonzero) and the case tables of scripts/gen_fengwu_golden.py.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict

import numpy as np
import torch

K = 4


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


@torch.no_grad()
def fill_(module: torch.nn.Module, seed: int = 0) -> torch.nn.Module:
    """Per-key seeded parameters: matrices ~ N(0, 1 / fan_in), LayerNorm gains 1 + 0.25 N, every bias 0.1 N."""
    for key, t in module.state_dict().items():
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        n = rs.standard_normal(tuple(t.shape))
        if t.dim() == 2:
            v = n / np.sqrt(t.shape[1])
        elif key.endswith("weight"):
            v = 1.0 + 0.25 * n
        else:
            v = 0.1 * n
        t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return module


def params(module: torch.nn.Module, dtype=torch.float64, requires_grad: bool = False) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(requires_grad) for k, v in module.state_dict().items()}


# ---- the neighbour assignment ---------------------------------------------------------------------------------------------
def knn_assign(pos_x: torch.Tensor, pos_y: torch.Tensor) -> torch.Tensor:
    """[n_y, 4] indices into pos_x: an exhaustive sort of every target's sources by (squared distance, index).  Exact
    arithmetic: Python-int-sized integers fit int64 here; float positions are compared in float64."""
    integer = not (pos_x.is_floating_point() or pos_y.is_floating_point())
    px = pos_x.to(torch.int64 if integer else torch.float64).numpy()
    py = pos_y.to(torch.int64 if integer else torch.float64).numpy()
    out = np.empty((py.shape[0], K), dtype=np.int64)
    idx = np.arange(px.shape[0])
    for t in range(py.shape[0]):
        d = px - py[t]
        d2 = (d * d).sum(-1)
        out[t] = np.lexsort((idx, d2))[:K]  # last key is the primary one
    return torch.from_numpy(out)


def knn_weights(pos_x: torch.Tensor, pos_y: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
    """[n_y, 4] float32: 1 / max(d^2, 1e-16) in the dtype the positions promote to, as the reference forms them."""
    y_idx = torch.arange(pos_y.shape[0]).repeat_interleave(K)
    diff = pos_x[assign.reshape(-1)] - pos_y[y_idx]
    sq = (diff * diff).sum(dim=-1, keepdim=True)
    return (1.0 / torch.clamp(sq, min=1e-16)).reshape(-1, K).to(torch.float32)


def knn_interpolate(x: torch.Tensor, assign: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """x [n_x, f] -> [n_y, f]: sum_k w x[idx] / sum_k w, summed slot by slot as an index_add_ does."""
    w = weights.to(x.dtype)
    num = torch.zeros((assign.shape[0], x.shape[1]), dtype=x.dtype)
    den = torch.zeros((assign.shape[0], 1), dtype=x.dtype)
    for k in range(K):
        num = num + x[assign[:, k]] * w[:, k:k + 1]
        den = den + w[:, k:k + 1]
    return num / den


def image_positions(i_h: int, i_w: int) -> torch.Tensor:
    return torch.cartesian_prod((torch.arange(-i_h / 2, i_h / 2, 1) / i_h * 180).to(torch.long),
                                (torch.arange(0, i_w, 1) / i_w * 360).to(torch.long))


# ---- the layers -----------------------------------------------------------------------------------------------------------
def posemb_sincos_2d(h: int, w: int, dim: int, temperature: int = 10000) -> torch.Tensor:
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    omega = torch.arange(dim // 4) / (dim // 4 - 1)
    omega = 1.0 / (temperature ** omega)
    y = y.flatten()[:, None] * omega[None, :]
    x = x.flatten()[:, None] * omega[None, :]
    return torch.cat((x.sin(), x.cos(), y.sin(), y.cos()), dim=1).to(torch.float32)


def layer_norm(x, w, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention_core(q, k, v, scale):
    """[..., n, d] operands: softmax(scale q k^T) v with the maximum subtracted, as torch's softmax does."""
    dots = torch.matmul(q, k.transpose(-1, -2)) * scale
    dots = dots - dots.max(dim=-1, keepdim=True).values
    e = torch.exp(dots)
    return torch.matmul(e / e.sum(-1, keepdim=True), v)


def attention(sd, p, x, heads):
    b, n, _ = x.shape
    h = layer_norm(x, sd[p + "norm.weight"], sd[p + "norm.bias"])
    qkv = h @ sd[p + "to_qkv.weight"].T
    inner = qkv.shape[-1] // 3
    d = inner // heads
    q, k, v = (t.reshape(b, n, heads, d).permute(0, 2, 1, 3) for t in qkv.split(inner, dim=-1))
    out = attention_core(q, k, v, d ** -0.5).permute(0, 2, 1, 3).reshape(b, n, inner)
    return out @ sd[p + "to_out.weight"].T


def feed_forward(sd, p, x):
    h = layer_norm(x, sd[p + "net.0.weight"], sd[p + "net.0.bias"])
    h = gelu(h @ sd[p + "net.1.weight"].T + sd[p + "net.1.bias"])
    return h @ sd[p + "net.3.weight"].T + sd[p + "net.3.bias"]


def transformer(sd, p, x, depth, heads, res, window):
    for i in range(depth):
        x = attention(sd, "%slayers.%d.0." % (p, i), x, heads) + x
        x = feed_forward(sd, "%slayers.%d.1." % (p, i), x) + x
        if res:
            h, w, s_h, s_w = window
            bt, n, d = x.shape
            b = bt // (s_h * s_w)
            xw = x.reshape(b, s_h, s_w, h, w, d).permute(0, 3, 4, 1, 2, 5).reshape(b * h * w, s_h * s_w, d)
            xw = attention(sd, "%sres_layers.%d.1." % (p, i), xw, heads) + xw
            x = xw.reshape(b, h, w, s_h, s_w, d).permute(0, 3, 4, 1, 2, 5).reshape(bt, n, d)
    return layer_norm(x, sd[p + "norm.weight"], sd[p + "norm.bias"])


def image_meta_model(sd, cfg, x, p=""):
    """cfg: the constructor keywords (image_size, patch_size, depth, heads, channels, res, scale_factor)."""
    ih, iw = pair(cfg["image_size"])
    ph, pw = pair(cfg["patch_size"])
    h, w = ih // ph, iw // pw
    b, c = x.shape[0], x.shape[1]
    t = x.reshape(b, c, h, ph, w, pw).permute(0, 2, 4, 3, 5, 1).reshape(b, h * w, ph * pw * c)
    e = p + "to_patch_embedding."
    t = layer_norm(t, sd[e + "1.weight"], sd[e + "1.bias"])
    t = t @ sd[e + "2.weight"].T + sd[e + "2.bias"]
    t = layer_norm(t, sd[e + "3.weight"], sd[e + "3.bias"])
    t = t + posemb_sincos_2d(h, w, ph * pw * c).to(device=t.device, dtype=t.dtype)
    res = bool(cfg.get("res", False))
    window = (h, w) + tuple(pair(cfg["scale_factor"])) if res else None
    t = transformer(sd, p + "transformer.", t, cfg["depth"], cfg["heads"], res, window)
    return t.reshape(b, h, w, ph, pw, c).permute(0, 5, 1, 3, 2, 4).reshape(b, c, ih, iw)


def batcher(x, s_h, s_w):
    b, c, hh, ww = x.shape
    h, w = hh // s_h, ww // s_w
    return x.reshape(b, c, h, s_h, w, s_w).permute(0, 3, 5, 1, 2, 4).reshape(b * s_h * s_w, c, h, w)


def debatcher(x, s_h, s_w):
    bt, c, h, w = x.shape
    b = bt // (s_h * s_w)
    return x.reshape(b, s_h, s_w, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(b, c, h * s_h, w * s_w)


def wrapper_image_model(sd, cfg, scale, x):
    s_h, s_w = pair(scale)
    cfg = dict(cfg, res=True, scale_factor=scale)
    return debatcher(image_meta_model(sd, cfg, batcher(x, s_h, s_w), "image_meta_model."), s_h, s_w)


def _interpolated(x, pos_x, pos_y, i_h, i_w, image_fn):
    b, n, c = x.shape
    a1 = knn_assign(pos_x, pos_y)
    a2 = knn_assign(pos_y, pos_x)
    t = x.permute(1, 0, 2).reshape(n, b * c)
    t = knn_interpolate(t, a1, knn_weights(pos_x, pos_y, a1))
    t = t.reshape(i_h, i_w, b, c).permute(2, 3, 0, 1)
    t = image_fn(t)
    t = t.permute(2, 3, 0, 1).reshape(i_h * i_w, b * c)
    t = knn_interpolate(t, a2, knn_weights(pos_y, pos_x, a2))
    return t.reshape(n, b, c).permute(1, 0, 2)


def meta_model(sd, cfg, lat_lons, x):
    i_h, i_w = pair(cfg["image_size"])
    pos_x = torch.tensor(lat_lons).to(torch.long)
    return _interpolated(x, pos_x, image_positions(i_h, i_w), i_h, i_w, lambda t: image_meta_model(sd, cfg, t, "image_meta_model."))


def wrapper_meta_model(sd, cfg, scale, lat_lons, x):
    s_h, s_w = pair(scale)
    i_h, i_w = pair(cfg["image_size"])
    i_h, i_w = i_h * s_h, i_w * s_w
    pos_x = torch.tensor(lat_lons)
    return _interpolated(x, pos_x, image_positions(i_h, i_w), i_h, i_w, lambda t: wrapper_image_model(sd, cfg, scale, t))


# ---- the fixture cases of scripts/gen_fengwu_golden.py ---------------------------------------------------------------------------
def lat_lons_5deg():
    return [(float(lat), float(lon)) for lat in np.arange(-90.0, 90.0, 5.0) for lon in np.arange(0.0, 360.0, 5.0)]


SMALL = dict(image_size=4, patch_size=2, depth=1, heads=1, mlp_dim=7, channels=3, dim_head=8)
ERA5 = dict(image_size=(36, 72), patch_size=4, depth=2, heads=4, mlp_dim=5, channels=4, dim_head=64)  # train/era5.py's shape
BASE = dict(image_size=(8, 12), patch_size=4, depth=2, heads=2, mlp_dim=5, channels=3, dim_head=16)   # the wrappers' inner model
META = dict(image_size=20, patch_size=4, depth=1, heads=2, mlp_dim=5, channels=3, dim_head=16)

IMAGE_CASES = {  # name -> (cfg, batch, seed)
    "fengwu_image_small": (SMALL, 2, 41),
    "fengwu_image_era5": (ERA5, 2, 42),
}
WRAPPER_IMAGE_CASES = {  # name -> (cfg of the wrapped model, scale_factor, batch, seed)
    "fengwu_wrapper_image_s3": (BASE, 3, 2, 43),
    "fengwu_wrapper_image_s2x3": (BASE, (2, 3), 2, 44),
}
META_CASES = {"fengwu_meta_5deg": (META, 2, 45)}  # name -> (cfg, batch, seed)
WRAPPER_META_CASES = {"fengwu_wrapper_meta_5deg": (META, 2, 2, 46)}  # name -> (cfg, scale_factor, batch, seed)


def image_input(cfg, batch: int, seed: int, scale=1) -> torch.Tensor:
    ih, iw = pair(cfg["image_size"])
    s_h, s_w = pair(scale)
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((batch, cfg["channels"], ih * s_h, iw * s_w)).astype(np.float32))


def rows_input(cfg, batch: int, seed: int, n: int) -> torch.Tensor:
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((batch, n, cfg["channels"])).astype(np.float32))


ALL_CASES = sorted(list(IMAGE_CASES) + list(WRAPPER_IMAGE_CASES) + list(META_CASES) + list(WRAPPER_META_CASES))


def build(ns, name: str):
    """A fixture case on the classes of ``ns`` (ours, or the reference's): (filled model, float32 CPU input, restatement
    ``fn(sd, x)`` in the dtype of its arguments)."""
    if name in IMAGE_CASES:
        cfg, batch, seed = IMAGE_CASES[name]
        return fill_(ns.ImageMetaModel(**cfg), seed), image_input(cfg, batch, seed), lambda sd, x: image_meta_model(sd, cfg, x)
    if name in WRAPPER_IMAGE_CASES:
        cfg, scale, batch, seed = WRAPPER_IMAGE_CASES[name]
        model = fill_(ns.WrapperImageModel(ns.ImageMetaModel(**cfg), scale), seed)
        return model, image_input(cfg, batch, seed, scale), lambda sd, x: wrapper_image_model(sd, cfg, scale, x)
    lat_lons = lat_lons_5deg()
    if name in META_CASES:
        cfg, batch, seed = META_CASES[name]
        model = fill_(ns.MetaModel(lat_lons, **cfg), seed)
        return model, rows_input(cfg, batch, seed, len(lat_lons)), lambda sd, x: meta_model(sd, cfg, lat_lons, x)
    cfg, scale, batch, seed = WRAPPER_META_CASES[name]
    model = fill_(ns.WrapperMetaModel(lat_lons, ns.MetaModel(lat_lons, **cfg), scale), seed)
    return model, rows_input(cfg, batch, seed, len(lat_lons)), lambda sd, x: wrapper_meta_model(sd, cfg, scale, lat_lons, x)
