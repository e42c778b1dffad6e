"""WeatherMesh's processor (``graph_weather/models/weathermesh/processor.py``): ``WeatherMeshProcessor``, its config and the
``NeighborhoodAttention3D`` layer it stacks, with the reference's constructor arguments, attribute names and ``state_dict`` keys.

The reference takes the layer from NATTEN (``natten.NeighborhoodAttention3D(embed_dim=, num_heads=, kernel_size=)``, the 0.20
signature).  NATTEN is not part of the reference tree; the semantics below are restated from NATTEN's documentation and NOT pinned
against NATTEN.  Input and output are channels-last ``[B, D, H, W, C]``.  ``qkv(x)`` is viewed ``[B, D, H, W, 3, heads, head_dim]``
(column ``s C + h head_dim + d`` is q, k or v ``s`` of head ``h``), ``out = proj(na3d(q, k, v))`` with the heads concatenated as
``h head_dim + d``.  Non-causal, stride 1, dilation 1: per axis of length ``L`` with an odd kernel ``k <= L`` the query at index
``i`` attends to the ``k`` consecutive indices from ``clamp(i - k // 2, 0, L - k)`` - near a border the window shifts inward and
keeps ``k`` keys (no padding, no truncation, no wrap-around); the neighbourhood is the product of the three ranges; per head
``softmax(scale q . k)`` over its ``kD kH kW`` keys weighs v.  No position bias, no attention dropout.

The attention is ``csrc/gw_na3d.hip``: a workgroup owns a tile of 8 x 8 neighbouring queries and stages the union of their windows
in LDS once per key plane; the backward recomputes the probabilities in a query-side launch (dq) and a key-side launch (dk, dv)
without atomics.  q, k and v are read in place as column blocks of the qkv product.  Even kernels, stride, dilation, causal masks
and projection dropout are not built (``NotImplementedError``).  fp32 only; there is no CPU path.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .gencast import _Linear
from .ops import on_device_of
from .wide import _L, _ld, _rows, _st

__all__ = ["NeighborhoodAttention3D", "WeatherMeshProcessor", "WeatherMeshProcessorConfig", "na3d_forward", "na3d_backward",
           "na3d", "window_start", "inverse_range", "MAX_HEAD_DIM"]

MAX_HEAD_DIM = 256  # include/gw_amd.h: gw_na3d_forward


def window_start(i: int, k: int, length: int) -> int:
    """First of the ``k`` indices the query at ``i`` attends to on an axis of ``length``."""
    return min(max(i - k // 2, 0), length - k)


def inverse_range(j: int, k: int, length: int) -> Tuple[int, int]:
    """(first, last) query that attends to the key at ``j``: longer than ``k`` within ``k // 2`` of a border."""
    return (0 if j < k else j - k // 2), (length - 1 if j >= length - k else j + k // 2)


def _triple(v, name: str) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(t) for t in v)
    if len(v) != 3:
        raise ValueError("graph_weather_amd: %s must be an int or three ints, got %r" % (name, v))
    return v


def _check(q, k, v, shape, kernel, heads: int) -> Tuple[int, int]:
    B, D, H, W = (int(s) for s in shape)
    C = int(q.shape[1])
    if heads < 1 or C % heads:
        raise ValueError("graph_weather_amd: the width of q (%d) must be a multiple of the heads (%d)" % (C, heads))
    for kk, L, axis in zip(kernel, (D, H, W), "DHW"):
        if kk < 1:
            raise ValueError("graph_weather_amd: kernel sizes must be at least 1, got %r" % (kernel,))
        if kk % 2 == 0:
            raise NotImplementedError("graph_weather_amd: even kernel sizes are not built, got %r" % (kernel,))
        if kk > L:
            raise ValueError("graph_weather_amd: kernel size %d exceeds the length %d of axis %s" % (kk, L, axis))
    if C // heads > MAX_HEAD_DIM:
        raise NotImplementedError("graph_weather_amd: the neighbourhood attention kernels take head_dim <= %d, got %d"
                                  % (MAX_HEAD_DIM, C // heads))
    rows = B * D * H * W
    if rows * heads >= 2 ** 31:
        raise NotImplementedError("graph_weather_amd: the neighbourhood attention kernels take tokens * heads < 2^31")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if tuple(t.shape) != (rows, C):
            raise RuntimeError("graph_weather_amd: neighbourhood attention expects %s [%d, %d], got %s" % (name, rows, C, tuple(t.shape)))
    return C, C // heads


def na3d_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, shape, kernel, heads: int, scale: float):
    """3-D neighbourhood attention (include/gw_amd.h: gw_na3d_forward): q, k, v [B D H W, heads head_dim] rows of the volume
    ``shape = (B, D, H, W)`` (views with a row stride are read in place) -> (out [rows, heads head_dim], lse [2, rows heads])."""
    q, k, v = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
    kernel = _triple(kernel, "kernel")
    C, dh = _check(q, k, v, shape, kernel, heads)
    B, D, H, W = (int(s) for s in shape)
    rows = B * D * H * W
    out = torch.empty((rows, C), dtype=torch.float32, device=q.device)
    lse = torch.empty((2, rows * heads), dtype=torch.float32, device=q.device)
    with on_device_of(out):
        _lib.check(_L().gw_na3d_forward(B, D, H, W, heads, dh, *kernel, float(scale), q.data_ptr(), _ld(q), k.data_ptr(), _ld(k),
                                        v.data_ptr(), _ld(v), out.data_ptr(), C, lse.data_ptr(), _st(out)), "gw_na3d_forward")
    return out, lse


def na3d_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, shape, kernel, heads: int, scale: float, out: torch.Tensor,
                  lse: torch.Tensor, dout: torch.Tensor, stacked: bool = False):
    """(dq, dk, dv) of ``na3d_forward``.  ``stacked``: the three are the column blocks of one [rows, 3 C] tensor (the layout of the
    qkv product), which is returned as a fourth value."""
    q, k, v, out, dout = _rows(q, "q"), _rows(k, "k"), _rows(v, "v"), _rows(out, "out"), _rows(dout, "dout")
    kernel = _triple(kernel, "kernel")
    C, dh = _check(q, k, v, shape, kernel, heads)
    B, D, H, W = (int(s) for s in shape)
    rows = B * D * H * W
    if out.shape != q.shape or dout.shape != q.shape:
        raise RuntimeError("graph_weather_amd: neighbourhood attention backward expects out and dout shaped like q %s, got %s and %s"
                           % (tuple(q.shape), tuple(out.shape), tuple(dout.shape)))
    if stacked:
        dqkv = torch.empty((rows, 3 * C), dtype=torch.float32, device=q.device)
        dq, dk, dv = dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]
    else:
        dqkv = None
        dq, dk, dv = (torch.empty((rows, C), dtype=torch.float32, device=q.device) for _ in range(3))
    delta = torch.empty((max(rows * heads, 1),), dtype=torch.float32, device=q.device)
    with on_device_of(dq):
        _lib.check(_L().gw_na3d_backward(B, D, H, W, heads, dh, *kernel, float(scale), q.data_ptr(), _ld(q), k.data_ptr(), _ld(k),
                                         v.data_ptr(), _ld(v), out.data_ptr(), _ld(out), dout.data_ptr(), _ld(dout), lse.data_ptr(),
                                         delta.data_ptr(), dq.data_ptr(), _ld(dq), dk.data_ptr(), _ld(dk), dv.data_ptr(), _ld(dv),
                                         _st(dq)), "gw_na3d_backward")
    return (dq, dk, dv, dqkv) if stacked else (dq, dk, dv)


class _NA3D(Function):
    """Neighbourhood attention on separate q, k, v rows (any row stride)."""

    @staticmethod
    def forward(ctx, q, k, v, shape, kernel, heads: int, scale: float):
        out, lse = na3d_forward(q, k, v, shape, kernel, heads, scale)
        ctx.meta = (tuple(shape), tuple(kernel), heads, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        shape, kernel, heads, scale = ctx.meta
        dq, dk, dv = na3d_backward(q, k, v, shape, kernel, heads, scale, out, lse, dout)
        return dq, dk, dv, None, None, None, None


class _NA3DStacked(Function):
    """Neighbourhood attention on q, k, v read in place as the column blocks of the qkv product [rows, 3 C]; the gradient is one
    stacked tensor too, each block written by the kernels through its leading dimension."""

    @staticmethod
    def forward(ctx, qkv, shape, kernel, heads: int, scale: float):
        C = int(qkv.shape[1]) // 3
        out, lse = na3d_forward(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], shape, kernel, heads, scale)
        ctx.meta = (tuple(shape), tuple(kernel), heads, scale, C)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        shape, kernel, heads, scale, C = ctx.meta
        dqkv = na3d_backward(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], shape, kernel, heads, scale, out, lse, dout, stacked=True)[3]
        return dqkv, None, None, None, None


def na3d(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, shape, kernel, heads: int, scale: float) -> torch.Tensor:
    """Differentiable 3-D neighbourhood attention on q, k, v [B D H W, heads head_dim] rows."""
    return _NA3D.apply(q, k, v, tuple(shape), _triple(kernel, "kernel"), heads, scale)


class NeighborhoodAttention3D(nn.Module):
    """Neighborhood Attention 3D Module (NATTEN 0.20's signature; semantics restated from its documentation, see the module
    docstring).  ``forward(x)``: x [B, D, H, W, C] -> [B, D, H, W, C]."""

    def __init__(self, embed_dim, num_heads, kernel_size, stride=1, dilation=1, is_causal=False, qkv_bias=True, qk_scale=None,
                 proj_drop=0.0):
        super().__init__()
        if num_heads < 1 or embed_dim % num_heads:
            raise ValueError("graph_weather_amd: embed_dim (%d) must be a multiple of num_heads (%d)" % (embed_dim, num_heads))
        kernel_size, stride, dilation = _triple(kernel_size, "kernel_size"), _triple(stride, "stride"), _triple(dilation, "dilation")
        causal = tuple(bool(c) for c in is_causal) if isinstance(is_causal, (tuple, list)) else (bool(is_causal),) * 3
        if any(k < 1 for k in kernel_size):
            raise ValueError("graph_weather_amd: kernel sizes must be at least 1, got %r" % (kernel_size,))
        if any(k % 2 == 0 for k in kernel_size):
            raise NotImplementedError("graph_weather_amd: even kernel sizes are not built, got %r" % (kernel_size,))
        if any(s != 1 for s in stride):
            raise NotImplementedError("graph_weather_amd: strided neighbourhood attention is not built, got stride %r" % (stride,))
        if any(d != 1 for d in dilation):
            raise NotImplementedError("graph_weather_amd: dilated neighbourhood attention is not built, got dilation %r" % (dilation,))
        if any(causal):
            raise NotImplementedError("graph_weather_amd: causal neighbourhood attention is not built, got is_causal %r" % (is_causal,))
        if proj_drop != 0.0:
            raise NotImplementedError("graph_weather_amd: projection dropout is not built, got proj_drop %r" % (proj_drop,))
        if embed_dim // num_heads > MAX_HEAD_DIM:
            raise NotImplementedError("graph_weather_amd: the neighbourhood attention kernels take head_dim <= %d, got %d"
                                      % (MAX_HEAD_DIM, embed_dim // num_heads))
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.scale = qk_scale or self.head_dim ** -0.5
        self.kernel_size = kernel_size
        self.stride = stride
        self.dilation = dilation
        self.is_causal = is_causal

        self.qkv = nn.Linear(embed_dim, embed_dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(embed_dim, embed_dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 5 or int(x.shape[-1]) != self.embed_dim:
            raise ValueError("graph_weather_amd: NeighborhoodAttention3D expects a rank-5 input [B, D, H, W, %d], got %s"
                             % (self.embed_dim, tuple(x.shape)))
        B, D, H, W, C = (int(s) for s in x.shape)
        for kk, L, axis in zip(self.kernel_size, (D, H, W), "DHW"):
            if kk > L:
                raise ValueError("graph_weather_amd: kernel size %d exceeds the length %d of axis %s" % (kk, L, axis))
        if not x.is_cuda:
            raise RuntimeError("graph_weather_amd: x must live on a HIP device (no CPU path exists)")
        if x.dtype != torch.float32:
            raise RuntimeError(f"graph_weather_amd: x must be float32, got {x.dtype}")
        qkv = _Linear.apply(x.reshape(-1, C), self.qkv.weight, self.qkv.bias, False)
        out = _NA3DStacked.apply(qkv, (B, D, H, W), self.kernel_size, self.num_heads, float(self.scale))
        return _Linear.apply(out, self.proj.weight, self.proj.bias, False).view(B, D, H, W, C)

    def extra_repr(self) -> str:
        return "head_dim=%d, num_heads=%d, kernel_size=%r, stride=%r, dilation=%r, is_causal=%r" % (
            self.head_dim, self.num_heads, self.kernel_size, self.stride, self.dilation, self.is_causal)


@dataclass
class WeatherMeshProcessorConfig:
    latent_dim: int
    n_layers: int
    kernel: tuple
    num_heads: int

    @staticmethod
    def from_json(json: dict) -> "WeatherMeshProcessorConfig":
        """The config of a flat dict, as the reference's ``dacite.from_dict`` builds it: every field is required, a value of
        another type than the field's is an error, further keys are ignored."""
        values = {}
        for f in dataclasses.fields(WeatherMeshProcessorConfig):
            if f.name not in json:
                raise ValueError('missing value for field "%s"' % f.name)
            want = tuple if f.name == "kernel" else int
            value = json[f.name]
            if not isinstance(value, want):
                raise TypeError('wrong value type for field "%s" - should be "%s" instead of value "%r" of type "%s"'
                                % (f.name, want.__name__, value, type(value).__name__))
            values[f.name] = value
        return WeatherMeshProcessorConfig(**values)

    def to_json(self) -> dict:
        return dataclasses.asdict(self)


class WeatherMeshProcessor(nn.Module):
    """The processor of WeatherMesh (processor.py): ``n_layers`` neighbourhood-attention layers applied in order to a
    channels-last latent volume x [B, D, H, W, latent_dim]."""

    def __init__(self, latent_dim, n_layers=10, kernel=(5, 7, 7), num_heads=8):
        super().__init__()
        self.layers = nn.ModuleList(NeighborhoodAttention3D(embed_dim=latent_dim, num_heads=num_heads, kernel_size=kernel)
                                    for _ in range(n_layers))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for layer in self.layers:
            x = layer(x)
        return x
