"""Test helper (not a test file): torch restatements of 3-D neighbourhood attention and of WeatherMesh's processor, in any float
dtype, and torch-only stand-ins for the two packages the reference's ``weathermesh/processor.py`` imports and that are not
installed: ``natten`` (``NeighborhoodAttention3D``) and ``dacite`` (``from_dict`` / ``asdict`` on a flat dataclass).

NATTEN's semantics are restated from its documentation (0.20: ``NeighborhoodAttention3D(embed_dim, num_heads, kernel_size,
stride=1, dilation=1, is_causal=False, qkv_bias=True, qk_scale=None, proj_drop=0.0)``), not pinned against NATTEN: non-causal,
stride 1, dilation 1; per axis of length L with an odd kernel k <= L the query at i attends to the k consecutive indices from
``clamp(i - k // 2, 0, L - k)``; the neighbourhood is the product of the three ranges; softmax(scale q . k) over it weighs v.
"""
import dataclasses
import types

import numpy as np
import torch
from torch import nn


def window_start(i: int, k: int, length: int) -> int:
    return min(max(i - k // 2, 0), length - k)


def inverse_range(j: int, k: int, length: int):
    """(first, last) query whose window holds key j."""
    return (0 if j < k else j - k // 2), (length - 1 if j >= length - k else j + k // 2)


def axis_windows(length: int, k: int) -> torch.Tensor:
    """[length, k] int64: the indices each query attends to."""
    if k < 1 or k % 2 == 0 or k > length:
        raise ValueError("kernel %d on an axis of length %d" % (k, length))
    return torch.tensor([[window_start(i, k, length) + t for t in range(k)] for i in range(length)], dtype=torch.int64)


def neighbour_table(shape, kernel) -> torch.Tensor:
    """[D H W, kD kH kW] int64: the linear token indices of every query's neighbourhood, depth-major."""
    (D, H, W), (kd, kh, kw) = shape, kernel
    wd, wh, ww = axis_windows(D, kd), axis_windows(H, kh), axis_windows(W, kw)
    idx = (wd[:, None, None, :, None, None] * H + wh[None, :, None, None, :, None]) * W + ww[None, None, :, None, None, :]
    return idx.reshape(D * H * W, kd * kh * kw)


def na3d(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kernel, scale: float) -> torch.Tensor:
    """q, k, v [B, D, H, W, heads, head_dim] -> out of the same shape, in the dtype of q."""
    B, D, H, W, nh, dh = q.shape
    idx = neighbour_table((D, H, W), kernel)
    n, win = idx.shape
    qf, kf, vf = (t.reshape(B, n, nh, dh) for t in (q, k, v))
    kn = kf[:, idx.reshape(-1)].reshape(B, n, win, nh, dh)
    vn = vf[:, idx.reshape(-1)].reshape(B, n, win, nh, dh)
    s = torch.einsum("bnhd,bnwhd->bnhw", qf * scale, kn)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bnhw,bnwhd->bnhd", p, vn).reshape(B, D, H, W, nh, dh)


def dense_attention(q, k, v, scale: float) -> torch.Tensor:
    """Softmax attention of every token of a volume over all its tokens: q, k, v [B, D, H, W, heads, head_dim]."""
    B, D, H, W, nh, dh = q.shape
    qf, kf, vf = (t.reshape(B, -1, nh, dh) for t in (q, k, v))
    p = torch.softmax(torch.einsum("bnhd,bmhd->bhnm", qf * scale, kf), dim=-1)
    return torch.einsum("bhnm,bmhd->bnhd", p, vf).reshape(q.shape)


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(t) for t in v)


class NeighborhoodAttention3D(nn.Module):
    """The stand-in for ``natten.NeighborhoodAttention3D``: torch operations only, any float dtype."""

    def __init__(self, embed_dim, num_heads, kernel_size, stride=1, dilation=1, is_causal=False, qkv_bias=True, qk_scale=None,
                 proj_drop=0.0):
        super().__init__()
        assert embed_dim % num_heads == 0
        assert _triple(stride) == (1, 1, 1) and _triple(dilation) == (1, 1, 1) and not is_causal, "not restated"
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.scale = qk_scale or self.head_dim ** -0.5
        self.kernel_size, self.stride, self.dilation, self.is_causal = _triple(kernel_size), _triple(stride), _triple(dilation), is_causal
        self.qkv = nn.Linear(embed_dim, embed_dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(embed_dim, embed_dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        B, D, H, W, C = x.shape
        qkv = self.qkv(x).reshape(B, D, H, W, 3, self.num_heads, self.head_dim)
        out = na3d(qkv[:, :, :, :, 0], qkv[:, :, :, :, 1], qkv[:, :, :, :, 2], self.kernel_size, self.scale)
        return self.proj_drop(self.proj(out.reshape(B, D, H, W, C)))


def natten_modules() -> dict:
    mod = types.ModuleType("natten")
    mod.NeighborhoodAttention3D = NeighborhoodAttention3D
    return {"natten": mod}


def dacite_modules() -> dict:
    """``from_dict(data_class=, data=)`` on a flat dataclass (every field required, values type-checked against plain class
    annotations) and the ``asdict`` the reference calls on the module."""
    mod = types.ModuleType("dacite")

    def from_dict(data_class, data, config=None):
        values = {}
        for f in dataclasses.fields(data_class):
            if f.name not in data:
                raise ValueError('missing value for field "%s"' % f.name)
            if isinstance(f.type, type) and not isinstance(data[f.name], f.type):
                raise TypeError('wrong value type for field "%s"' % f.name)
            values[f.name] = data[f.name]
        return data_class(**values)

    mod.from_dict, mod.asdict = from_dict, dataclasses.asdict
    return {"dacite": mod}


def processor_forward(params: dict, x: torch.Tensor, n_layers: int, kernel, num_heads: int) -> torch.Tensor:
    """WeatherMeshProcessor.forward from a ``state_dict``-keyed table of tensors (differentiable, dtype of the tensors)."""
    B, D, H, W, C = x.shape
    dh = C // num_heads
    for i in range(n_layers):
        pre = "layers.%d." % i
        qkv = (x @ params[pre + "qkv.weight"].T + params[pre + "qkv.bias"]).reshape(B, D, H, W, 3, num_heads, dh)
        out = na3d(qkv[:, :, :, :, 0], qkv[:, :, :, :, 1], qkv[:, :, :, :, 2], _triple(kernel), dh ** -0.5)
        x = out.reshape(B, D, H, W, C) @ params[pre + "proj.weight"].T + params[pre + "proj.bias"]
    return x


# ---- recorded cases (scripts/gen_weathermesh_golden.py): name -> (constructor arguments, input shape, seed) ----------------------
CASES = {
    "weathermesh_processor_default_kernel": (dict(latent_dim=8, n_layers=2, num_heads=1), (1, 6, 8, 12, 8), 11),
    "weathermesh_processor_heads4": (dict(latent_dim=32, n_layers=3, num_heads=4, kernel=(3, 5, 5)), (2, 4, 6, 7, 32), 12),
}


def case_input(name: str) -> torch.Tensor:
    _, shape, seed = CASES[name]
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))
