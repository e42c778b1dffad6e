"""Restatements of the reference's modulation layers (graph_weather/models/layers/stochastic_decomposition.py, film.py) and
of the noise function eps(key, i) that include/gw_amd.h specifies, written from the specification and not from the kernel.

``sdl`` / ``film_generate`` / ``film_apply`` are plain torch compositions in the dtype of their arguments (float64 for the
oracle, float32 on the CPU for the yardstick); ``eps`` is numpy: integers exactly, the transcendentals in float64.
"""
from __future__ import annotations

import zlib
from typing import Dict

import numpy as np
import torch

# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """``counter``: four uint32-valued arrays (or ints), ``key``: two; returns the four output words as uint64 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c


def split_key(key: int):
    """(low word, high word) of a 64-bit key given as a Python int (signed int64 values count modulo 2^64)."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    return key & MASK32, key >> 32


def eps(key: int, n: int, start: int = 0) -> np.ndarray:
    """eps(key, i) for i in [start, start + n) as float64."""
    j0, j1 = start // 4, (start + n + 3) // 4
    j = np.arange(j0, j1, dtype=np.uint64)
    w = philox4x32_10((j & np.uint64(MASK32), j >> np.uint64(32), 0, 0), split_key(key))
    u = [((v >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for v in w]
    out = np.empty((j1 - j0, 4), dtype=np.float64)
    for a, b, col in ((0, 1, 0), (2, 3, 2)):
        r = np.sqrt(-2.0 * np.log(u[a]))
        out[:, col] = r * np.cos(2.0 * np.pi * u[b])
        out[:, col + 1] = r * np.sin(2.0 * np.pi * u[b])
    return out.reshape(-1)[start - 4 * j0: start - 4 * j0 + n]


EPS_MAX = float(np.sqrt(2.0 * 25.0 * np.log(2.0)))  # u >= 2^-25


@torch.no_grad()
def fill_(module: torch.nn.Module, seed: int = 0) -> torch.nn.Module:
    """Per-key seeded parameters: Linear weights ~ N(0, 1 / fan_in), biases 0.1 N, ``alpha`` 0.5 + 0.25 N (the reference's zero
    initialisation of alpha would hide every error)."""
    for key, t in module.state_dict().items():
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        n = rs.standard_normal(tuple(t.shape))
        if key.endswith("alpha"):
            v = 0.5 + 0.25 * n
        elif t.dim() == 2:
            v = n / np.sqrt(t.shape[1])
        else:
            v = 0.1 * n
        t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.device))
    return module


def params64(module: torch.nn.Module) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().double() for k, v in module.state_dict().items()}


def sdl(sd: Dict[str, torch.Tensor], x: torch.Tensor, z: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """StochasticDecompositionLayer.forward with the noise given."""
    style = z @ sd["style_net.weight"].T + sd["style_net.bias"]
    shape = tuple(x.shape[:2]) + (1,) * (x.dim() - 2)
    return x + (sd["alpha"].reshape((1, -1) + (1,) * (x.dim() - 2)) * style.reshape(shape) * noise)


def film_generate(sd: Dict[str, torch.Tensor], batch_size: int, lead_time: int, feature_dim: int):
    """FiLMGenerator.forward: (gamma, beta)."""
    w1 = sd["network.0.weight"]
    one_hot = torch.zeros(batch_size, w1.shape[1], dtype=w1.dtype, device=w1.device)
    one_hot[:, lead_time] = 1.0
    h = torch.relu(one_hot @ w1.T + sd["network.0.bias"])
    gb = h @ sd["network.2.weight"].T + sd["network.2.bias"]
    return gb[:, :feature_dim], gb[:, feature_dim:]


def film_apply(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """FiLMApplier.forward."""
    shape = tuple(x.shape[:2]) + (1,) * (x.dim() - 2)
    return x * gamma.reshape(shape) + beta.reshape(shape)


# the fixture cases of scripts/gen_modulation_golden.py: name -> arguments
SDL_CASES = {  # (x shape, latent_dim, seed)
    "modulation_sdl_2x32x10": ((2, 32, 10), 16, 11),
    "modulation_sdl_2x32x16x16": ((2, 32, 16, 16), 16, 12),
    "modulation_sdl_2x32x8x16x16": ((2, 32, 8, 16, 16), 16, 13),
    "modulation_sdl_2x78x12x24": ((2, 78, 12, 24), 32, 14),
}
GENERATOR_CASES = {  # (num_lead_times, hidden_dim, feature_dim, batch, lead_time, seed)
    "modulation_gen_10_8_16_b4_t3": (10, 8, 16, 4, 3, 21),
    "modulation_gen_40_64_78_b2_t0": (40, 64, 78, 2, 0, 22),
    "modulation_gen_40_64_78_b2_t39": (40, 64, 78, 2, 39, 22),
    "modulation_gen_5_256_256_b3_t4": (5, 256, 256, 3, 4, 23),
}
APPLIER_CASES = {  # (x shape, seed)
    "modulation_film_4x16x8x8": ((4, 16, 8, 8), 31),
    "modulation_film_2x78x12x24": ((2, 78, 12, 24), 32),
    "modulation_film_3x256x37": ((3, 256, 37), 33),
    "modulation_film_2x16": ((2, 16), 34),
}


def sdl_inputs(shape, latent_dim: int, seed: int):
    """(x, z, noise) float32 CPU tensors of an SDL case: x and z from RandomState(seed), the noise from RandomState(seed + 1)."""
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    z = torch.from_numpy(rs.standard_normal((shape[0], latent_dim)).astype(np.float32))
    noise = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal(shape).astype(np.float32))
    return x, z, noise


def applier_inputs(shape, seed: int):
    """(x, gamma, beta) float32 CPU tensors of a FiLMApplier case."""
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    gamma = torch.from_numpy((1.0 + 0.5 * rs.standard_normal(shape[:2])).astype(np.float32))
    beta = torch.from_numpy(rs.standard_normal(shape[:2]).astype(np.float32))
    return x, gamma, beta
