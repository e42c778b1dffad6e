"""Test helper (not a test file): torch-only restatements of WeatherMesh's convolution blocks, encoder, decoder and model in any
float dtype, from ``state_dict``-keyed tables of tensors; a nested stand-in for ``dacite`` (the configs of ``weathermesh2.py`` hold
dataclasses and lists of dataclasses); and the table of recorded cases (scripts/gen_weathermesh_model_golden.py).

Written from the behaviour of the reference's ``layers.py``, ``encoder.py``, ``decoder.py`` and ``weathermesh2.py``:

* a block is ``gelu(bn2(conv2(gelu(bn1(conv1(x))))) + bn_skip(skip(x)))`` with 3-tap convolutions of padding 1 (conv1 at stride 1,
  conv2 at the block's stride), a 1-tap skip at the block's stride, no biases, exact (erf) GELU; an up block first upsamples height
  and width 2 x bilinearly (``align_corners=False``) and runs at stride 1;
* BatchNorm: eps 1e-5, momentum 0.1; training mode normalises with the batch mean and biased variance and moves the running
  buffers towards the mean and the UNBIASED variance; eval mode normalises with the running buffers;
* the encoder appends the surface plane as the last depth index, ``to_latent`` is a 1 x 1 x 1 convolution with bias, the latent is
  channels-last; the decoder mirrors it.

The attention is that of tests/weathermesh_oracle.py (NATTEN's semantics restated from its documentation).
"""
import dataclasses
import re
import types
import typing
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from . import weathermesh_oracle as wo
from .cafa_oracle import fill_

EPS, MOMENTUM = 1e-5, 0.1


def fill_model_(module: torch.nn.Module, seed: int) -> torch.nn.Module:
    """The rule of tests/cafa_oracle.fill_ (which cannot fill the 0-dim ``num_batches_tracked``): per key, seeded by the key's
    CRC and ``seed``, N(0, 1 / fan_in) for matrices and kernels, 1 + 0.25 N for other ``weight``s, 0.1 N for the rest -
    every ``running_var`` drawn as 0.5 + 0.5 |N| (a variance has to be positive) and every ``num_batches_tracked`` zeroed."""
    with torch.no_grad():
        for key, t in module.state_dict().items():
            if t.dim() == 0:
                t.zero_()
                continue
            rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
            n = rs.standard_normal(tuple(t.shape))
            if t.dim() >= 2:
                v = n / np.sqrt(int(np.prod(t.shape[1:])))
            elif key.endswith("weight"):
                v = 1.0 + 0.25 * n
            elif key.endswith("running_var"):
                v = 0.5 + 0.5 * np.abs(n)
            else:
                v = 0.1 * n
            t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return module


def batch_norm(p: dict, pre: str, x: torch.Tensor, training: bool, updates: dict) -> torch.Tensor:
    dims = [0] + list(range(2, x.dim()))
    shape = [1, -1] + [1] * (x.dim() - 2)
    if training:
        n = x.numel() // x.shape[1]
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
        updates[pre + "running_mean"] = ((1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean).detach()
        updates[pre + "running_var"] = ((1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * var * n / max(n - 1, 1)).detach()
    else:
        mean, var = p[pre + "running_mean"], p[pre + "running_var"]
    xhat = (x - mean.view(shape)) / torch.sqrt(var.view(shape) + EPS)
    return xhat * p[pre + "weight"].view(shape) + p[pre + "bias"].view(shape)


def conv(x: torch.Tensor, w: torch.Tensor, stride, padding: int, bias=None) -> torch.Tensor:
    return (F.conv3d if x.dim() == 5 else F.conv2d)(x, w, bias, stride=stride, padding=padding)


def upsample(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 5:
        return F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


def res_block(p: dict, pre: str, x: torch.Tensor, stride, skip: str, bn_skip: str, training: bool, updates: dict) -> torch.Tensor:
    identity = batch_norm(p, pre + bn_skip + ".", conv(x, p[pre + skip + ".weight"], stride, 0), training, updates)
    out = F.gelu(batch_norm(p, pre + "bn1.", conv(x, p[pre + "conv1.weight"], 1, 1), training, updates))
    out = batch_norm(p, pre + "bn2.", conv(out, p[pre + "conv2.weight"], stride, 1), training, updates)
    return F.gelu(out + identity)


def down_block(p, pre, x, stride, training, updates):
    return res_block(p, pre, x, stride, "downsample", "bn_down", training, updates)


def up_block(p, pre, x, training, updates):
    return res_block(p, pre, upsample(x), 1, "upsample", "bn_up", training, updates)


def attention_layers(p: dict, pre: str, x: torch.Tensor, n_layers: int, kernel, num_heads: int) -> torch.Tensor:
    sub = {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
    return wo.processor_forward({"layers." + k: v for k, v in sub.items()}, x, n_layers, kernel, num_heads)


def encoder_forward(p: dict, pre: str, surface, pressure, n_blocks: int, n_layers: int, kernel, num_heads: int, training: bool,
                    updates: dict) -> torch.Tensor:
    for i in range(n_blocks):
        surface = down_block(p, "%ssurface_path.%d." % (pre, i), surface, 2, training, updates)
        pressure = down_block(p, "%spressure_path.%d." % (pre, i), pressure, (1, 2, 2), training, updates)
    features = torch.cat([pressure, surface.unsqueeze(2)], dim=2)
    latent = conv(features, p[pre + "to_latent.weight"], 1, 0, p[pre + "to_latent.bias"]).permute(0, 2, 3, 4, 1)
    return attention_layers(p, pre + "transformer_layers.", latent, n_layers, kernel, num_heads)


def decoder_forward(p: dict, pre: str, latent, n_blocks: int, n_layers: int, kernel, num_heads: int, training: bool, updates: dict):
    latent = attention_layers(p, pre + "transformer_layers.", latent, n_layers, kernel, num_heads)
    features = conv(latent.permute(0, 4, 1, 2, 3), p[pre + "split.weight"], 1, 0, p[pre + "split.bias"])
    pressure, surface = features[:, :, :-1], features[:, :, -1]
    for i in range(n_blocks):
        pressure = up_block(p, "%spressure_path.%d." % (pre, i), pressure, training, updates)
        surface = up_block(p, "%ssurface_path.%d." % (pre, i), surface, training, updates)
    return surface, pressure


def model_forward(p: dict, processors: list, surface, pressure, forecast_steps: int, kw: dict, training: bool, updates: dict):
    """WeatherMesh.forward: ``p`` the model's table, ``processors`` one table per processor (they are not part of the model's)."""
    latent = encoder_forward(p, "encoder.", surface, pressure, kw["encoder_num_conv_blocks"], kw["encoder_num_transformer_layers"],
                             kw["kernel"], kw["num_heads"], training, updates)
    for _ in range(forecast_steps):
        for q in processors:
            latent = wo.processor_forward(q, latent, kw["processor_num_layers"], kw["kernel"], kw["num_heads"])
    return decoder_forward(p, "decoder.", latent, kw["decoder_num_conv_blocks"], kw["decoder_num_transformer_layers"], kw["kernel"],
                           kw["num_heads"], training, updates)


# ---- the nested stand-in for dacite --------------------------------------------------------------------------------------------
def dacite_modules() -> dict:
    """``from_dict(data_class=, data=)``: every field required, plain classes type-checked, a dict converted for a dataclass-typed
    field and a list of dicts for ``List[dataclass]``; ``asdict`` as the reference calls it on the module."""
    mod = types.ModuleType("dacite")

    def convert(name, want, value):
        if dataclasses.is_dataclass(want):
            return value if isinstance(value, want) else from_dict(want, value)
        if typing.get_origin(want) is list:
            if not isinstance(value, list):
                raise TypeError('wrong value type for field "%s"' % name)
            return [convert(name, typing.get_args(want)[0], v) for v in value]
        if isinstance(want, type) and not isinstance(value, want):
            raise TypeError('wrong value type for field "%s"' % name)
        return value

    def from_dict(data_class, data, config=None):
        values = {}
        for f in dataclasses.fields(data_class):
            if f.name not in data:
                raise ValueError('missing value for field "%s"' % f.name)
            values[f.name] = convert(f.name, f.type, data[f.name])
        return data_class(**values)

    mod.from_dict, mod.asdict = from_dict, dataclasses.asdict
    return {"dacite": mod}


def type_name(t) -> str:
    """A field's type as recorded: the class name, or the ``typing`` form without module prefixes."""
    if isinstance(t, str):
        return t
    if isinstance(t, type):
        return t.__name__
    return re.sub(r"\w+\.", "", str(t))


# ---- recorded cases ----------------------------------------------------------------------------------------------------------------
MODEL_KW = dict(encoder=None, processors=None, decoder=None, timesteps=[1, 6], surface_channels=3, pressure_channels=4,
                pressure_levels=3, latent_dim=8, encoder_num_conv_blocks=2, encoder_num_transformer_layers=1, encoder_hidden_dim=4,
                decoder_num_conv_blocks=2, decoder_num_transformer_layers=1, decoder_hidden_dim=4, processor_num_layers=2,
                kernel=(3, 3, 3), num_heads=2)
FORECAST_STEPS = 2
# name -> (batch, (height, width), seed)
CASES = {"weathermesh_model_13x18": (2, (13, 18), 31), "weathermesh_model_24x32": (2, (24, 32), 32)}

CONFIG_JSON = {
    "encoder": dict(input_channels_2d=3, input_channels_3d=4, latent_dim=8, n_pressure_levels=3, num_conv_blocks=2, hidden_dim=4,
                    kernel_size=(3, 3, 3), num_heads=2, num_transformer_layers=1),
    "processors": [dict(latent_dim=8, n_layers=2, kernel=(3, 3, 3), num_heads=2)] * 2,
    "decoder": dict(latent_dim=8, output_channels_2d=3, output_channels_3d=4, n_conv_blocks=2, hidden_dim=4, kernel_size=(3, 3, 3),
                    num_heads=2, num_transformer_layers=1),
    **{k: v for k, v in MODEL_KW.items() if k not in ("encoder", "processors", "decoder")},
}


def case_inputs(name: str):
    batch, (h, w), seed = CASES[name]
    rs = np.random.RandomState(seed)
    surface = torch.from_numpy(rs.standard_normal((batch, MODEL_KW["surface_channels"], h, w)).astype(np.float32))
    pressure = torch.from_numpy(rs.standard_normal((batch, MODEL_KW["pressure_channels"], MODEL_KW["pressure_levels"], h, w))
                                .astype(np.float32))
    return surface, pressure


def build_model(cls, name: str):
    """``cls(**MODEL_KW)`` with the case's weights: the model from its seed, processor i from seed + 1 + i."""
    seed = CASES[name][2]
    model = fill_model_(cls(**MODEL_KW), seed)
    for i, proc in enumerate(model.processors):
        fill_(proc, seed + 1 + i)
    return model
