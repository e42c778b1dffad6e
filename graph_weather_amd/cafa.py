"""The CaFA models of the reference (``graph_weather/models/cafa/``): ``CaFAForecaster`` = patch-embedding encoder, a stack
of factorized (axial) transformer blocks, patch-expanding decoder.

Same constructor arguments, defaults, attribute names and ``state_dict`` keys (and their order) as the reference.  The
forecaster works on channels-last rows ``[(b h w), dim]`` from end to end: the encoder's ``Conv2d(kernel = stride = f)`` reads
the NCHW image as it lies and writes rows, the decoder's ``ConvTranspose2d`` reads rows and writes the NCHW image
(``csrc/gw_cafa.hip``; the reference's zero padding to a multiple of ``f`` and its crop are bounds predicates there), and the
attention along the height or the width of the token grid reads q, k, v in place from the rows of ``to_qkv`` through three
strides (``gw_attention_axial_*`` in ``csrc/gw_fengwu.hip``: the FengWu attention kernels, addressed by (outer, inner,
token)) - there is no ``b h w d -> (b w) h d`` copy and no padded copy.  LayerNorm, Linear and the residual adds are the
wide path's kernels (``wide.py``), the exact GELU is FengWu's.

The stand-alone classes keep the reference's tensor shapes (NCHW for encoder / processor / decoder, ``b h w d`` for the
attention classes); the layout change at their boundary is a torch permute.  fp32 only, ``dim_head <= 128``, dropout only
where it is the identity (``p == 0`` or ``eval()``); there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .fengwu_ghr import _check_dim_head, _Gelu, _ln, _need_hip
from .ops import on_device_of
from .wide import _Add, _L, _ld, _Linear, _rows, _st


# ---------------------------------------------------------------------------------------------------------------------
# axial attention
# ---------------------------------------------------------------------------------------------------------------------
def _axial(B: int, H: int, W: int, axis: int, ld: int) -> Tuple[int, int, int, Tuple[int, int, int]]:
    """(outer, inner, n, strides) of the sequences along ``axis`` of [B, H, W] rows with row stride ``ld``."""
    if axis == 1:
        return B, W, H, (H * W * ld, ld, W * ld)
    if axis == 2:
        return B, H, W, (H * W * ld, W * ld, ld)
    raise ValueError("Axis must be 1 (height) or 2 (width)")


def _i3(t) -> ctypes.Array:
    return (ctypes.c_int64 * 3)(*t)


def attention_axial_forward(qkv: torch.Tensor, B: int, H: int, W: int, axis: int, heads: int, dim_head: int, scale: float):
    """softmax(scale q k^T) v along the height (axis 1) or the width (axis 2) of the [B * H * W, 3 * heads * dim_head] rows of
    to_qkv, read in place -> (out [B * H * W, heads * dim_head] in the same (b h w) row order, log-sum-exp [2, pairs, n] with
    the pairs ordered (b, w, head) for axis 1 and (b, h, head) for axis 2)."""
    _check_dim_head(dim_head)
    _axial(B, H, W, axis, 0)  # a bad axis is reported before anything else
    qkv = _rows(qkv, "qkv")
    inner_dim = heads * dim_head
    if int(qkv.shape[0]) != B * H * W or int(qkv.shape[1]) != 3 * inner_dim:
        raise RuntimeError("graph_weather_amd: qkv must be [%d, %d], got %s" % (B * H * W, 3 * inner_dim, tuple(qkv.shape)))
    outer, inner, n, sq = _axial(B, H, W, axis, _ld(qkv))
    _, _, _, so = _axial(B, H, W, axis, inner_dim)
    out = torch.empty((B * H * W, inner_dim), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((2, outer * inner * heads, n), dtype=torch.float32, device=qkv.device)
    p = qkv.data_ptr()
    with on_device_of(out):
        _lib.check(_L().gw_attention_axial_forward(outer, inner, heads, n, dim_head, p, p + 4 * inner_dim, p + 8 * inner_dim, _i3(sq),
                                                   float(scale), out.data_ptr(), _i3(so), lse.data_ptr(), _st(out)),
                   "gw_attention_axial_forward")
    return out, lse


def attention_axial_backward(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, B: int, H: int, W: int,
                             axis: int, heads: int, dim_head: int, scale: float) -> torch.Tensor:
    """Gradient of ``attention_axial_forward`` with respect to qkv, laid out like qkv (dense rows)."""
    qkv, dout, out = _rows(qkv, "qkv"), _rows(dout, "dout"), _rows(out, "out")
    inner_dim = heads * dim_head
    outer, inner, n, sq = _axial(B, H, W, axis, _ld(qkv))
    so, sg, sd = (_axial(B, H, W, axis, ld)[3] for ld in (_ld(out), _ld(dout), 3 * inner_dim))
    dqkv = torch.empty((B * H * W, 3 * inner_dim), dtype=torch.float32, device=qkv.device)
    delta = torch.empty((outer * inner * heads, n), dtype=torch.float32, device=qkv.device)
    p, g = qkv.data_ptr(), dqkv.data_ptr()
    with on_device_of(dqkv):
        _lib.check(_L().gw_attention_axial_backward(outer, inner, heads, n, dim_head, p, p + 4 * inner_dim, p + 8 * inner_dim, _i3(sq),
                                                    float(scale), out.data_ptr(), _i3(so), dout.data_ptr(), _i3(sg), lse.data_ptr(),
                                                    delta.data_ptr(), g, g + 4 * inner_dim, g + 8 * inner_dim, _i3(sd), _st(dqkv)),
                   "gw_attention_axial_backward")
    return dqkv


class _AxialAttention(Function):
    @staticmethod
    def forward(ctx, qkv, B: int, H: int, W: int, axis: int, heads: int, dim_head: int, scale: float):
        out, lse = attention_axial_forward(qkv, B, H, W, axis, heads, dim_head, scale)
        ctx.meta = (B, H, W, axis, heads, dim_head, scale)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return (attention_axial_backward(qkv, out, lse, dout, *ctx.meta),) + (None,) * 7


# ---------------------------------------------------------------------------------------------------------------------
# patch embed / expand
# ---------------------------------------------------------------------------------------------------------------------
def _image(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_hip(t, name)
    if t.dim() != 4:
        raise RuntimeError(f"graph_weather_amd: {name} must be [batch, channels, height, width]")
    return t.contiguous()


def _patches(h: int, w: int, f: int) -> Tuple[int, int]:
    return -(-h // f), -(-w // f)


def _workspace(B: int, C: int, H: int, W: int, f: int, D: int, device) -> torch.Tensor:
    nbytes = int(_L().gw_patch_workspace_bytes(B, C, H, W, f, D))
    if nbytes == 0:
        _lib.check(-1, "gw_patch_workspace_bytes")
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=device)


def patch_embed_forward(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], f: int) -> torch.Tensor:
    """Conv2d(C, D, kernel = stride = f) of the image zero padded on the right and bottom to a multiple of f: x [B, C, H, W]
    -> rows [(b, oh, ow), D] with oh = ceil(H / f), ow = ceil(W / f)."""
    x, weight = _image(x, "x"), weight.contiguous()
    B, C, H, W = (int(s) for s in x.shape)
    D = int(weight.shape[0])
    if tuple(weight.shape) != (D, C, f, f):
        raise RuntimeError("graph_weather_amd: patch embedding expects a [%d, %d, %d, %d] weight, got %s" % (D, C, f, f, tuple(weight.shape)))
    oh, ow = _patches(H, W, f)
    out = torch.empty((B * oh * ow, D), dtype=torch.float32, device=x.device)
    with on_device_of(out):
        _lib.check(_L().gw_patch_embed_forward(B, C, H, W, f, D, x.data_ptr(), weight.data_ptr(),
                                               None if bias is None else bias.contiguous().data_ptr(), out.data_ptr(), D, _st(out)),
                   "gw_patch_embed_forward")
    return out


def patch_embed_backward(x: torch.Tensor, weight: torch.Tensor, dout: torch.Tensor, f: int, need_dx: bool = True, need_dw: bool = True):
    """(dx [B, C, H, W] or None, dweight, dbias or None, None) of ``patch_embed_forward``."""
    x, weight, dout = _image(x, "x"), weight.contiguous(), _rows(dout, "dout")
    B, C, H, W = (int(s) for s in x.shape)
    D = int(weight.shape[0])
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight) if need_dw else None
    db = torch.empty((D,), dtype=torch.float32, device=x.device) if need_dw else None
    ws = _workspace(B, C, H, W, f, D, x.device) if need_dw else None
    with on_device_of(x):
        _lib.check(_L().gw_patch_embed_backward(B, C, H, W, f, D, x.data_ptr(), weight.data_ptr(), dout.data_ptr(), _ld(dout),
                                                None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                                                None if dx is None else dx.data_ptr(), None if dw is None else dw.data_ptr(),
                                                None if db is None else db.data_ptr(), _st(x)), "gw_patch_embed_backward")
    return dx, dw, db


def patch_expand_forward(rows: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int, W: int,
                         f: int) -> torch.Tensor:
    """ConvTranspose2d(D, C, kernel = stride = f) cropped to H x W: rows [(b, oh, ow), D] -> [B, C, H, W]."""
    rows, weight = _rows(rows, "x"), weight.contiguous()
    D, C = int(weight.shape[0]), int(weight.shape[1])
    oh, ow = _patches(H, W, f)
    if tuple(weight.shape) != (D, C, f, f) or tuple(rows.shape) != (B * oh * ow, D):
        raise RuntimeError("graph_weather_amd: patch expansion expects [%d, %d] rows and a [%d, C, %d, %d] weight, got %s and %s"
                           % (B * oh * ow, D, D, f, f, tuple(rows.shape), tuple(weight.shape)))
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=rows.device)
    with on_device_of(out):
        _lib.check(_L().gw_patch_expand_forward(B, C, H, W, f, D, rows.data_ptr(), _ld(rows), weight.data_ptr(),
                                                None if bias is None else bias.contiguous().data_ptr(), out.data_ptr(), _st(out)),
                   "gw_patch_expand_forward")
    return out


def patch_expand_backward(rows: torch.Tensor, weight: torch.Tensor, dout: torch.Tensor, f: int, need_drows: bool = True,
                          need_dw: bool = True):
    """(d_rows, dweight, dbias) of ``patch_expand_forward``; dout is [B, C, H, W]."""
    rows, weight, dout = _rows(rows, "x"), weight.contiguous(), _image(dout, "dout")
    B, C, H, W = (int(s) for s in dout.shape)
    D = int(weight.shape[0])
    d_rows = torch.empty((int(rows.shape[0]), D), dtype=torch.float32, device=rows.device) if need_drows else None
    dw = torch.empty_like(weight) if need_dw else None
    db = torch.empty((C,), dtype=torch.float32, device=rows.device) if need_dw else None
    ws = _workspace(B, C, H, W, f, D, rows.device) if need_dw else None
    with on_device_of(dout):
        _lib.check(_L().gw_patch_expand_backward(B, C, H, W, f, D, rows.data_ptr(), _ld(rows), weight.data_ptr(), dout.data_ptr(),
                                                 None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                                                 None if d_rows is None else d_rows.data_ptr(), D, None if dw is None else dw.data_ptr(),
                                                 None if db is None else db.data_ptr(), _st(dout)), "gw_patch_expand_backward")
    return d_rows, dw, db


class _PatchEmbed(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, f: int):
        ctx.f = f
        ctx.save_for_backward(x, weight)
        return patch_embed_forward(x, weight, bias, f)

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        need_dw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (ctx.needs_input_grad[0] or need_dw):
            return None, None, None, None
        dx, dw, db = patch_embed_backward(x, weight, dout, ctx.f, ctx.needs_input_grad[0], need_dw)
        return dx, dw, db, None


class _PatchExpand(Function):
    @staticmethod
    def forward(ctx, rows, weight, bias, B: int, H: int, W: int, f: int):
        ctx.f = f
        ctx.save_for_backward(rows, weight)
        return patch_expand_forward(rows, weight, bias, B, H, W, f)

    @staticmethod
    def backward(ctx, dout):
        rows, weight = ctx.saved_tensors
        need_dw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (ctx.needs_input_grad[0] or need_dw):
            return (None,) * 7
        d_rows, dw, db = patch_expand_backward(rows, weight, dout, ctx.f, ctx.needs_input_grad[0], need_dw)
        return (d_rows, dw, db) + (None,) * 4


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def _to_rows(x: torch.Tensor) -> torch.Tensor:
    """b c h w -> (b h w) c"""
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b * h * w, c)


def _to_image(x2: torch.Tensor, b: int, h: int, w: int) -> torch.Tensor:
    """(b h w) c -> b c h w"""
    return x2.reshape(b, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _no_dropout(drop: nn.Dropout) -> None:
    if drop.training and drop.p > 0:
        raise NotImplementedError("graph_weather_amd: dropout > 0 in train() mode is not implemented (use dropout = 0 or eval())")


def _check_dropout(module: nn.Module) -> None:
    """Before anything else in a forward: the unsupported mode is reported whatever the input is."""
    for m in module.modules():
        if isinstance(m, nn.Dropout):
            _no_dropout(m)


def FeedFoward(dim, multiply=4, dropout=0.0):
    """Linear, GELU, Dropout, Linear, Dropout (the reference's spelling and Sequential numbering)."""
    inner_dim = int(dim * multiply)
    return nn.Sequential(
        nn.Linear(dim, inner_dim),
        nn.GELU(),
        nn.Dropout(dropout),
        nn.Linear(inner_dim, dim),
        nn.Dropout(dropout),
    )


def _ffn_rows(ffn: nn.Sequential, x2: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
    _no_dropout(ffn[2])
    _no_dropout(ffn[4])
    h = _Linear.apply(x2, ffn[0].weight, ffn[0].bias, False)
    h = _Gelu.apply(h)
    h = _Linear.apply(h, ffn[3].weight, ffn[3].bias, False)
    return h if residual is None else _Add.apply(h, residual)


class AxialAttention(nn.Module):
    """Multi-head self-attention along one axis of a ``b h w d`` feature map."""

    def __init__(self, dim, heads, dim_head=64, dropout=0.0):
        super().__init__()
        _check_dim_head(dim_head)
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head**-0.5
        inner_dim = dim_head * heads

        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Linear(inner_dim, dim)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, axis):
        if axis not in (1, 2):
            raise ValueError("Axis must be 1 (height) or 2 (width)")
        _check_dropout(self)
        _need_hip(x, "x")
        b, h, w, d = (int(s) for s in x.shape)
        return self.rows(x.reshape(b * h * w, d), b, h, w, axis, None).reshape(b, h, w, -1)

    def rows(self, x2: torch.Tensor, B: int, H: int, W: int, axis: int, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """to_out(attention along ``axis``(to_qkv(x))) (+ residual) on [(b h w), dim] rows."""
        if axis not in (1, 2):
            raise ValueError("Axis must be 1 (height) or 2 (width)")
        _need_hip(x2, "x")
        _no_dropout(self.dropout)
        qkv = _Linear.apply(x2, self.to_qkv.weight, None, False)
        o = _AxialAttention.apply(qkv, B, H, W, axis, self.heads, self.dim_head, self.scale)
        y = _Linear.apply(o, self.to_out.weight, self.to_out.bias, False)
        return y if residual is None else _Add.apply(y, residual)


class FactorizedAttention(nn.Module):
    """Height attention then width attention, each behind its LayerNorm and with its residual."""

    def __init__(self, dim, heads, dim_head=64, dropout=0.0):
        super().__init__()
        self.attn_height = AxialAttention(dim, heads, dim_head, dropout)
        self.attn_width = AxialAttention(dim, heads, dim_head, dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)

    def forward(self, x):
        _check_dropout(self)
        _need_hip(x, "x")
        b, h, w, d = (int(s) for s in x.shape)
        return self.rows(x.reshape(b * h * w, d), b, h, w).reshape(b, h, w, d)

    def rows(self, x2: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        _need_hip(x2, "x")
        x2 = self.attn_height.rows(_ln(self.norm1, x2), B, H, W, 1, x2)
        return self.attn_width.rows(_ln(self.norm2, x2), B, H, W, 2, x2)


class FactorizedTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head=64, feedforward_multiplier=4, dropout=0.0):
        super().__init__()
        self.attn = FactorizedAttention(dim, heads, dim_head, dropout)
        self.ffn = FeedFoward(dim, feedforward_multiplier, dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)

    def forward(self, x):
        _check_dropout(self)
        _need_hip(x, "x")
        b, h, w, d = (int(s) for s in x.shape)
        return self.rows(x.reshape(b * h * w, d), b, h, w).reshape(b, h, w, d)

    def rows(self, x2: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        _need_hip(x2, "x")
        x2 = _Add.apply(self.attn.rows(_ln(self.norm1, x2), B, H, W), x2)
        return _ffn_rows(self.ffn, _ln(self.norm2, x2), x2)


class CaFAProcessor(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, dim_head: int = 64, feedforward_multiplier: int = 4, dropout: float = 0.0):
        super().__init__()
        self.blocks = nn.ModuleList(
            [FactorizedTransformerBlock(dim, heads, dim_head, feedforward_multiplier, dropout) for _ in range(depth)]
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[batch, dim, height, width] -> the same shape."""
        _check_dropout(self)
        _need_hip(x, "x")
        b, _, h, w = (int(s) for s in x.shape)
        return _to_image(self.rows(_to_rows(x), b, h, w), b, h, w)

    def rows(self, x2: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        for block in self.blocks:
            x2 = block.rows(x2, B, H, W)
        return x2


class CaFAEncoder(nn.Module):
    def __init__(self, input_channels: int, model_dim: int, downsampling_factor: int = 1):
        super().__init__()
        self.encoder = nn.Conv2d(in_channels=input_channels, out_channels=model_dim, kernel_size=downsampling_factor,
                                 stride=downsampling_factor)

    @property
    def factor(self) -> int:
        return int(self.encoder.stride[0])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[batch, channels, height, width] -> [batch, model_dim, height // f, width // f] (Conv2d drops a ragged edge)."""
        _check_dropout(self)
        _need_hip(x, "x")
        f = self.factor
        b, _, h, w = (int(s) for s in x.shape)
        if h < f or w < f:
            raise RuntimeError("graph_weather_amd: the image is smaller than the downsampling factor")
        if h % f or w % f:
            x = x[:, :, :h // f * f, :w // f * f]
        return _to_image(self.rows(x), b, h // f, w // f)

    def rows(self, x: torch.Tensor) -> torch.Tensor:
        """[batch, channels, height, width], zero padded to a multiple of f -> [(b, ceil(h / f), ceil(w / f)), model_dim]."""
        return _PatchEmbed.apply(x, self.encoder.weight, self.encoder.bias, self.factor)


class CaFADecoder(nn.Module):
    def __init__(self, model_dim: int, output_channels: int, upsampling_factor: int = 1):
        super().__init__()
        self.decoder = nn.ConvTranspose2d(in_channels=model_dim, out_channels=output_channels, kernel_size=upsampling_factor,
                                          stride=upsampling_factor)

    @property
    def factor(self) -> int:
        return int(self.decoder.stride[0])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[batch, model_dim, height, width] -> [batch, output_channels, height * f, width * f]."""
        _check_dropout(self)
        _need_hip(x, "x")
        b, _, h, w = (int(s) for s in x.shape)
        return self.rows(_to_rows(x), b, h * self.factor, w * self.factor)

    def rows(self, x2: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """[(b, ceil(H / f), ceil(W / f)), model_dim] -> [B, output_channels, H, W] (the crop of the transposed convolution)."""
        return _PatchExpand.apply(x2, self.decoder.weight, self.decoder.bias, B, H, W, self.factor)


class CaFAForecaster(nn.Module):
    def __init__(
        self,
        input_channels: int,
        output_channels: int,
        model_dim: int = 256,
        downsampling_factor: int = 2,
        processor_depth: int = 6,
        num_heads: int = 8,
        dim_head: int = 64,
        feedforward_multiplier: int = 4,
        dropout: float = 0.0,
    ):
        super().__init__()
        self.downsampling_factor = downsampling_factor
        self.encoder = CaFAEncoder(input_channels=input_channels, model_dim=model_dim, downsampling_factor=downsampling_factor)
        self.processor = CaFAProcessor(dim=model_dim, depth=processor_depth, heads=num_heads, dim_head=dim_head,
                                       feedforward_multiplier=feedforward_multiplier, dropout=dropout)
        self.decoder = CaFADecoder(model_dim=model_dim, output_channels=output_channels, upsampling_factor=downsampling_factor)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[batch, input_channels, height, width] -> [batch, output_channels, height, width], any height and width."""
        _check_dropout(self)
        _need_hip(x, "x")
        if x.dim() != 4:
            raise RuntimeError("graph_weather_amd: x must be [batch, channels, height, width]")
        b, _, h, w = (int(s) for s in x.shape)
        oh, ow = _patches(h, w, self.downsampling_factor)
        x2 = self.encoder.rows(x)
        x2 = self.processor.rows(x2, b, oh, ow)
        return self.decoder.rows(x2, b, h, w)
