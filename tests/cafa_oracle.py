"""A restatement of the reference's CaFA files (graph_weather/models/cafa/: encoder, factorize, processor, decoder, model),
written from their arithmetic as plain torch compositions over a ``state_dict``: float64 for the oracle, float32 on the CPU
for the yardstick (what fp32 arithmetic in the reference's own order of operations costs).  Nothing here touches the HIP
kernels, and nothing imports einops.

It also carries a per-key seeded ``fill_`` (the rule of tests/fengwu_oracle.fill_, extended to 4-D weights: matrices and
convolution weights ~ N(0, 1 / fan_in), LayerNorm gains 1 + 0.25 N, every bias 0.1 N) and the case table of
scripts/gen_cafa_golden.py.
"""
from __future__ import annotations

import zlib
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F


@torch.no_grad()
def fill_(module: torch.nn.Module, seed: int = 0) -> torch.nn.Module:
    for key, t in module.state_dict().items():
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        n = rs.standard_normal(tuple(t.shape))
        if t.dim() >= 2:
            v = n / np.sqrt(int(np.prod(t.shape[1:])))  # Linear [out, in], Conv2d [out, in, f, f], ConvTranspose2d [in, out, f, f]
        elif key.endswith("weight"):
            v = 1.0 + 0.25 * n
        else:
            v = 0.1 * n
        t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return module


def params(module: torch.nn.Module, dtype=torch.float64, requires_grad: bool = False) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(requires_grad) for k, v in module.state_dict().items()}


# name -> (constructor keywords, (batch, height, width), seed)
CASES = {
    "cafa_ref_32x64": (dict(input_channels=3, output_channels=3, model_dim=128, downsampling_factor=2, processor_depth=2, num_heads=4,
                            dim_head=64, feedforward_multiplier=4), (2, 32, 64), 11),
    "cafa_ref_33x65": (dict(input_channels=3, output_channels=3, model_dim=128, downsampling_factor=2, processor_depth=2, num_heads=4,
                            dim_head=64, feedforward_multiplier=4), (2, 33, 65), 12),
    "cafa_f3_20x37": (dict(input_channels=5, output_channels=4, model_dim=48, downsampling_factor=3, processor_depth=1, num_heads=3,
                           dim_head=20, feedforward_multiplier=4), (2, 20, 37), 13),
    "cafa_f1_9x17": (dict(input_channels=4, output_channels=4, model_dim=32, downsampling_factor=1, processor_depth=1, num_heads=2,
                          dim_head=8, feedforward_multiplier=4), (2, 9, 17), 14),
}
META_KEYS = ("input_channels", "output_channels", "model_dim", "downsampling_factor", "processor_depth", "num_heads", "dim_head",
             "feedforward_multiplier")


def case_input(name: str) -> torch.Tensor:
    cfg, (b, h, w), seed = CASES[name]
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((b, cfg["input_channels"], h, w)).astype(np.float32))


def build(pkg, name: str):
    """(model of ``pkg`` with the seeded parameters, input) of a case."""
    cfg, _, seed = CASES[name]
    return fill_(pkg.CaFAForecaster(**cfg), seed), case_input(name)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def layer_norm(p, key, x):
    return F.layer_norm(x, (x.shape[-1],), p[key + ".weight"], p[key + ".bias"], 1e-5)


def axial_attention(p, key, x, axis: int, heads: int):
    """x [b, h, w, d]; attention along the height (axis 1) or the width (axis 2)."""
    if axis not in (1, 2):
        raise ValueError("Axis must be 1 (height) or 2 (width)")
    b, h, w, d = x.shape
    seq = x.permute(0, 2, 1, 3).reshape(b * w, h, d) if axis == 1 else x.reshape(b * h, w, d)
    qkv = seq @ p[key + ".to_qkv.weight"].T
    inner = qkv.shape[-1] // 3
    dim_head = inner // heads
    q, k, v = (t.reshape(t.shape[0], t.shape[1], heads, dim_head).permute(0, 2, 1, 3) for t in qkv.split(inner, dim=-1))
    sim = (q @ k.transpose(-1, -2)) * dim_head**-0.5
    out = sim.softmax(dim=-1) @ v
    out = out.permute(0, 2, 1, 3).reshape(seq.shape[0], seq.shape[1], inner)
    out = out @ p[key + ".to_out.weight"].T + p[key + ".to_out.bias"]
    return out.reshape(b, w, h, d).permute(0, 2, 1, 3) if axis == 1 else out.reshape(b, h, w, d)


def factorized_attention(p, key, x, heads: int):
    x = x + axial_attention(p, key + ".attn_height", layer_norm(p, key + ".norm1", x), 1, heads)
    return x + axial_attention(p, key + ".attn_width", layer_norm(p, key + ".norm2", x), 2, heads)


def feed_forward(p, key, x):
    h = F.gelu(x @ p[key + ".0.weight"].T + p[key + ".0.bias"])
    return h @ p[key + ".3.weight"].T + p[key + ".3.bias"]


def block(p, key, x, heads: int):
    x = x + factorized_attention(p, key + ".attn", layer_norm(p, key + ".norm1", x), heads)
    return x + feed_forward(p, key + ".ffn", layer_norm(p, key + ".norm2", x))


def processor(p, key, x, depth: int, heads: int):
    """x [b, c, h, w] -> [b, c, h, w]"""
    x = x.permute(0, 2, 3, 1)
    for i in range(depth):
        x = block(p, "%s.blocks.%d" % (key, i), x, heads)
    return x.permute(0, 3, 1, 2)


def patch_embed(p, key, x, f: int):
    return F.conv2d(x, p[key + ".weight"], p[key + ".bias"], stride=f)


def patch_expand(p, key, x, f: int):
    return F.conv_transpose2d(x, p[key + ".weight"], p[key + ".bias"], stride=f)


def forecaster(p, x, cfg):
    f = cfg["downsampling_factor"]
    h, w = x.shape[2:]
    pad_h, pad_w = (f - h % f) % f, (f - w % f) % f
    if pad_h > 0 or pad_w > 0:
        x = F.pad(x, (0, pad_w, 0, pad_h))
    x = patch_embed(p, "encoder.encoder", x, f)
    x = processor(p, "processor", x, cfg["processor_depth"], cfg["num_heads"])
    x = patch_expand(p, "decoder.decoder", x, f)
    return x[:, :, :h, :w]
