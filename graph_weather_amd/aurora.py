"""The Aurora models of the reference (``graph_weather/models/aurora/``): ``AuroraModel`` on unstructured points (point
encoder, a stack of post-norm self-attention layers, point decoder), ``EarthSystemLoss``, ``Swin3DEncoder``,
``PerceiverProcessor`` and ``Decoder3D``.

Same constructor arguments, defaults, attribute names and ``state_dict`` keys (and their order) as the reference.  The torch
containers ``nn.MultiheadAttention`` / ``nn.TransformerEncoderLayer`` / ``nn.Transformer`` are kept as parameter holders only - their forward is
never called.  Every model works on rows ``[(b, n), dim]``: Linear, LayerNorm and the residual adds are the wide path's forward
kernels (``wide.py``; their weight gradients come from the ordered kernels of ``csrc/gw_aurora.hip``, without atomics), the exact GELU and the attention are FengWu's (``csrc/gw_fengwu.hip``), reading q, k, v in place from the rows of
``in_proj``; ``PerceiverProcessor``'s key-padding mask is the MASKED form of those kernels (an additive 0 / -inf bias per
(sample, key)), its pooling ``gw_token_mean_*``.  The 3 x 3 x 3 convolutions are implicit GEMMs (``csrc/gw_conv3d.hip``) that address
volumes through strides: ``Swin3DEncoder.conv1`` writes the channels-last rows its LayerNorm reads (no ``b c d h w -> b d h w c``
copy) and ``Decoder3D`` reads its ``[batch, seq, embed_dim]`` input reinterpreted as ``[batch, embed_dim, D, H, W]`` in place.

``EarthSystemLoss`` is one autograd node over ``csrc/gw_aurora.hip``: the spatial term walks the point pairs in tiles (the
reference materialises ``[B, N, N, C]`` differences), the MSE and physical terms are streaming reductions, and the four scalars
come back together; the backward is one elementwise kernel.

fp32 only, ``dim_head <= 128``, dropout only where it is the identity (``p == 0`` or ``eval()``); there is no CPU path.  The
only torch arithmetic is on the raw inputs (the division of the coordinates by 180 / 90 and the conversion of masks).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function

from . import _lib
from .cafa import _i3
from .fengwu_ghr import _Attention, _check_dim_head, _Gelu, _need_hip
from .ops import on_device_of
from .wide import _Add, _L, _ld, _relu_mask, _rows, _st, layernorm_forward, linear_forward


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _workspace(nbytes: int, what: str, device) -> torch.Tensor:
    if nbytes == 0:
        _lib.check(-1, what)
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=device)


def gemm_tn_ordered(a: torch.Tensor, b: torch.Tensor, want_colsum: bool):
    """(a^T @ b [m, n], column sums of a [m] or None) for a [rows, m], b [rows, n]: row slabs added in one fixed order."""
    a, b = _rows(a, "a"), _rows(b, "b")
    rows, m, n = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    nbytes = int(_L().gw_gemm_tn_ordered_workspace_bytes(m, n, rows))
    ws = _workspace(nbytes, "gw_gemm_tn_ordered_workspace_bytes", a.device)
    c = torch.empty((m, n), dtype=torch.float32, device=a.device)
    colsum = torch.empty((m,), dtype=torch.float32, device=a.device) if want_colsum else None
    with on_device_of(c):
        _lib.check(_L().gw_gemm_tn_ordered(m, n, rows, a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), ws.data_ptr(), nbytes, c.data_ptr(), n,
                                           None if colsum is None else colsum.data_ptr(), _st(c)), "gw_gemm_tn_ordered")
    return c, colsum


def layernorm_backward_ordered(dn: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor):
    """(dy, dgamma, dbeta) of LayerNorm(y) (eps 1e-5) for the upstream gradient dn, the rows added in one fixed order."""
    dn, y = _rows(dn, "dout"), _rows(y, "y")
    rows, width = int(y.shape[0]), int(y.shape[1])
    nbytes = int(_L().gw_layernorm_backward_ordered_workspace_bytes(rows, width))
    ws = _workspace(nbytes, "gw_layernorm_backward_ordered_workspace_bytes", y.device)
    dy = torch.empty((rows, width), dtype=torch.float32, device=y.device)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    with on_device_of(dy):
        _lib.check(_L().gw_layernorm_backward_ordered(rows, width, dn.data_ptr(), _ld(dn), y.data_ptr(), _ld(y), gamma.contiguous().data_ptr(),
                                                      ws.data_ptr(), nbytes, dy.data_ptr(), width, dgamma.data_ptr(), dbeta.data_ptr(),
                                                      _st(dy)), "gw_layernorm_backward_ordered")
    return dy, dgamma, dbeta


class _Linear(Function):
    """nn.Linear (+ nn.ReLU) on the wide path's forward kernel; the weight and bias gradients come from ``gemm_tn_ordered``
    (``wide._Linear`` adds its row slabs with atomics), so every gradient of these models is bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, w, b, relu: bool):
        out = linear_forward(x, w, b, relu)
        ctx.relu, ctx.has_b = relu, b is not None
        ctx.save_for_backward(x, w, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, out = ctx.saved_tensors
        dz = _relu_mask(dout, out) if ctx.relu else _rows(dout, "dout")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear_forward(dz, w.detach().t().contiguous(), None, False)
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = gemm_tn_ordered(dz, x, ctx.has_b)
        return dx, dw, db, None


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, y, gamma, beta):
        ctx.save_for_backward(y, gamma)
        return layernorm_forward(y, gamma, beta, None)

    @staticmethod
    def backward(ctx, dout):
        y, gamma = ctx.saved_tensors
        return layernorm_backward_ordered(dout, y, gamma)


def _ln(norm: nn.LayerNorm, x2: torch.Tensor) -> torch.Tensor:
    if abs(norm.eps - 1e-5) > 0:
        raise RuntimeError("graph_weather_amd: LayerNorm eps must be 1e-5")
    return _LayerNorm.apply(x2, norm.weight, norm.bias)


def _seq_strides(n: int, ld: int):
    return _i3((n * ld, 0, ld))


def attention_masked_forward(qkv: torch.Tensor, key_bias: torch.Tensor, batch: int, heads: int, n: int, dim_head: int, scale: float):
    """``fengwu_ghr.attention_forward`` with ``key_bias`` [batch, n] (0 keeps a key, -inf drops it) added to the scaled scores of
    every head and query of a sample."""
    _check_dim_head(dim_head)
    qkv, key_bias = _rows(qkv, "qkv"), _rows(key_bias, "key_bias").contiguous()
    inner = heads * dim_head
    if tuple(qkv.shape) != (batch * n, 3 * inner) or tuple(key_bias.shape) != (batch, n):
        raise RuntimeError("graph_weather_amd: qkv must be [%d, %d] and key_bias [%d, %d], got %s and %s"
                           % (batch * n, 3 * inner, batch, n, tuple(qkv.shape), tuple(key_bias.shape)))
    out = torch.empty((batch * n, inner), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((2, batch * heads, n), dtype=torch.float32, device=qkv.device)
    p = qkv.data_ptr()
    with on_device_of(out):
        _lib.check(_L().gw_attention_masked_forward(batch, 1, heads, n, dim_head, p, p + 4 * inner, p + 8 * inner, _seq_strides(n, _ld(qkv)),
                                                    key_bias.data_ptr(), float(scale), out.data_ptr(), _seq_strides(n, inner),
                                                    lse.data_ptr(), _st(out)), "gw_attention_masked_forward")
    return out, lse


def attention_masked_backward(qkv: torch.Tensor, key_bias: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor,
                              batch: int, heads: int, n: int, dim_head: int, scale: float) -> torch.Tensor:
    """Gradient of ``attention_masked_forward`` with respect to qkv, laid out like qkv; dk and dv of a dropped key are zero."""
    qkv, dout, out, key_bias = _rows(qkv, "qkv"), _rows(dout, "dout"), _rows(out, "out"), _rows(key_bias, "key_bias").contiguous()
    inner = heads * dim_head
    dqkv = torch.empty((batch * n, 3 * inner), dtype=torch.float32, device=qkv.device)
    delta = torch.empty((batch * heads, n), dtype=torch.float32, device=qkv.device)
    p, g = qkv.data_ptr(), dqkv.data_ptr()
    with on_device_of(dqkv):
        _lib.check(_L().gw_attention_masked_backward(batch, 1, heads, n, dim_head, p, p + 4 * inner, p + 8 * inner,
                                                     _seq_strides(n, _ld(qkv)), key_bias.data_ptr(), float(scale), out.data_ptr(),
                                                     _seq_strides(n, _ld(out)), dout.data_ptr(), _seq_strides(n, _ld(dout)),
                                                     lse.data_ptr(), delta.data_ptr(), g, g + 4 * inner, g + 8 * inner,
                                                     _seq_strides(n, 3 * inner), _st(dqkv)), "gw_attention_masked_backward")
    return dqkv


class _MaskedAttention(Function):
    @staticmethod
    def forward(ctx, qkv, key_bias, batch: int, heads: int, n: int, dim_head: int, scale: float):
        out, lse = attention_masked_forward(qkv, key_bias, batch, heads, n, dim_head, scale)
        ctx.meta = (batch, heads, n, dim_head, scale)
        ctx.save_for_backward(qkv, key_bias, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, key_bias, out, lse = ctx.saved_tensors
        return (attention_masked_backward(qkv, key_bias, out, lse, dout, *ctx.meta),) + (None,) * 6


def token_mean_forward(x2: torch.Tensor, batch: int, tokens: int) -> torch.Tensor:
    """[(b, s), width] rows -> [batch, width]: the mean over the tokens of every sample."""
    x2 = _rows(x2, "x")
    if int(x2.shape[0]) != batch * tokens:
        raise RuntimeError("graph_weather_amd: token mean expects %d rows, got %d" % (batch * tokens, int(x2.shape[0])))
    width = int(x2.shape[1])
    out = torch.empty((batch, width), dtype=torch.float32, device=x2.device)
    with on_device_of(out):
        _lib.check(_L().gw_token_mean_forward(batch, tokens, width, x2.data_ptr(), _ld(x2), out.data_ptr(), width, _st(out)),
                   "gw_token_mean_forward")
    return out


def token_mean_backward(dout: torch.Tensor, batch: int, tokens: int) -> torch.Tensor:
    dout = _rows(dout, "dout")
    width = int(dout.shape[1])
    dx = torch.empty((batch * tokens, width), dtype=torch.float32, device=dout.device)
    with on_device_of(dx):
        _lib.check(_L().gw_token_mean_backward(batch, tokens, width, dout.data_ptr(), _ld(dout), dx.data_ptr(), width, _st(dx)),
                   "gw_token_mean_backward")
    return dx


class _TokenMean(Function):
    @staticmethod
    def forward(ctx, x2, batch: int, tokens: int):
        ctx.meta = (batch, tokens)
        return token_mean_forward(x2, batch, tokens)

    @staticmethod
    def backward(ctx, dout):
        return token_mean_backward(dout, *ctx.meta), None, None


def relu_forward(x2: torch.Tensor) -> torch.Tensor:
    x2 = _rows(x2, "x").contiguous()
    y = torch.empty_like(x2)
    with on_device_of(y):
        _lib.check(_L().gw_relu_forward(x2.numel(), x2.data_ptr(), y.data_ptr(), _st(y)), "gw_relu_forward")
    return y


class _Relu(Function):
    @staticmethod
    def forward(ctx, x2):
        y = relu_forward(x2)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        return _relu_mask(dout, y)


def row_scale(x2: torch.Tensor, factor: torch.Tensor) -> torch.Tensor:
    """out[r, :] = x[r, :] * factor[r]"""
    x2 = _rows(x2, "x")
    rows, width = int(x2.shape[0]), int(x2.shape[1])
    _need_hip(factor, "mask")
    factor = factor.reshape(-1).contiguous()
    if int(factor.numel()) != rows:
        raise RuntimeError("graph_weather_amd: the mask has %d entries for %d points" % (int(factor.numel()), rows))
    out = torch.empty((rows, width), dtype=torch.float32, device=x2.device)
    with on_device_of(out):
        _lib.check(_L().gw_row_scale(rows, width, x2.data_ptr(), _ld(x2), factor.data_ptr(), out.data_ptr(), width, _st(out)),
                   "gw_row_scale")
    return out


class _RowScale(Function):
    @staticmethod
    def forward(ctx, x2, factor):
        ctx.save_for_backward(factor)
        return row_scale(x2, factor)

    @staticmethod
    def backward(ctx, dout):
        (factor,) = ctx.saved_tensors
        return row_scale(dout, factor), None


def earth_loss_forward(pred: torch.Tensor, target: Optional[torch.Tensor], points: torch.Tensor, spatial: bool, alpha: float,
                       beta: float, gamma: float):
    """(out [4] = (total, mse, spatial, physical), pair rows G [n, channels] or None, stats [2]) of ``gw_earth_loss_forward``."""
    B, N, C = (int(s) for s in pred.shape)
    dev = pred.device
    nbytes = int(_L().gw_earth_loss_workspace_bytes(B, N, C))
    if nbytes == 0:
        _lib.check(-1, "gw_earth_loss_workspace_bytes")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    stats = torch.empty((2,), dtype=torch.float32, device=dev)
    G = torch.empty((N, C), dtype=torch.float32, device=dev) if spatial else None
    with on_device_of(out):
        _lib.check(_L().gw_earth_loss_forward(B, N, C, pred.data_ptr(), None if target is None else target.data_ptr(), points.data_ptr(),
                                              1 if spatial else 0, float(alpha), float(beta), float(gamma), ws.data_ptr(), nbytes,
                                              out.data_ptr(), None if G is None else G.data_ptr(), stats.data_ptr(), _st(out)),
                   "gw_earth_loss_forward")
    return out, G, stats


def earth_loss_backward(pred: torch.Tensor, target: Optional[torch.Tensor], points: torch.Tensor, spatial: bool, alpha: float,
                        beta: float, gamma: float, G: Optional[torch.Tensor], stats: torch.Tensor, gout: torch.Tensor,
                        need_dpred: bool, need_dtarget: bool):
    B, N, C = (int(s) for s in pred.shape)
    dpred = torch.empty_like(pred) if need_dpred else None
    dtarget = torch.empty_like(pred) if need_dtarget else None
    gout = gout.contiguous()
    with on_device_of(pred):
        _lib.check(_L().gw_earth_loss_backward(B, N, C, pred.data_ptr(), None if target is None else target.data_ptr(), points.data_ptr(),
                                               1 if spatial else 0, float(alpha), float(beta), float(gamma),
                                               None if G is None else G.data_ptr(), stats.data_ptr(), gout.data_ptr(),
                                               None if dpred is None else dpred.data_ptr(),
                                               None if dtarget is None else dtarget.data_ptr(), _st(pred)), "gw_earth_loss_backward")
    return dpred, dtarget


class _EarthLoss(Function):
    """The four scalars as one [4] tensor (total, mse, spatial, physical); an upstream gradient on each is accepted."""

    @staticmethod
    def forward(ctx, pred, target, points, spatial: bool, alpha: float, beta: float, gamma: float):
        out, G, stats = earth_loss_forward(pred, target, points, spatial, alpha, beta, gamma)
        ctx.meta = (spatial, alpha, beta, gamma)
        ctx.save_for_backward(pred, target, points, G, stats)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, target, points, G, stats = ctx.saved_tensors
        need_t = target is not None and ctx.needs_input_grad[1]
        if not (ctx.needs_input_grad[0] or need_t):
            return (None,) * 7
        dpred, dtarget = earth_loss_backward(pred, target, points, *ctx.meta, G, stats, gout, ctx.needs_input_grad[0], need_t)
        return (dpred, dtarget) + (None,) * 5


def _ncdhw(c: int, v: int):
    return _i3((c * v, v, 1))


def _rows3(c_ld: int, v: int):
    return _i3((v * c_ld, 1, c_ld))


def conv3d_forward(x: torch.Tensor, stride_x, weight: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, stride_out,
                   batch: int, cin: int, cout: int, dhw, transposed: bool) -> torch.Tensor:
    d, h, w = dhw
    with on_device_of(out):
        _lib.check(_L().gw_conv3d_forward(batch, cin, cout, d, h, w, 1 if transposed else 0, x.data_ptr(), stride_x, weight.data_ptr(),
                                          None if bias is None else bias.contiguous().data_ptr(), out.data_ptr(), stride_out, _st(out)),
                   "gw_conv3d_forward")
    return out


def conv3d_backward(x: torch.Tensor, stride_x, weight: torch.Tensor, dout: torch.Tensor, stride_dout, dx: Optional[torch.Tensor],
                    stride_dx, batch: int, cin: int, cout: int, dhw, transposed: bool, need_dw: bool):
    """(dweight, dbias) or (None, None); dx is filled in place when given."""
    d, h, w = dhw
    dw = db = ws = None
    nbytes = 0
    if need_dw:
        nbytes = int(_L().gw_conv3d_workspace_bytes(batch, cin, cout, d, h, w, 1 if transposed else 0))
        if nbytes == 0:
            _lib.check(-1, "gw_conv3d_workspace_bytes")
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device)
        dw = torch.empty_like(weight)
        db = torch.empty((cout,), dtype=torch.float32, device=x.device)
    with on_device_of(x):
        _lib.check(_L().gw_conv3d_backward(batch, cin, cout, d, h, w, 1 if transposed else 0, x.data_ptr(), stride_x, weight.data_ptr(),
                                           dout.data_ptr(), stride_dout, None if ws is None else ws.data_ptr(), nbytes,
                                           None if dx is None else dx.data_ptr(), stride_dx, None if dw is None else dw.data_ptr(),
                                           None if db is None else db.data_ptr(), _st(x)), "gw_conv3d_backward")
    return dw, db


class _Conv3dRows(Function):
    """nn.Conv3d(k 3, p 1, s 1): x [B, cin, D, H, W] -> channels-last rows [(b, d, h, w), cout]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, cin, D, H, W = (int(s) for s in x.shape)
        cout, V = int(weight.shape[0]), D * H * W
        out = torch.empty((B * V, cout), dtype=torch.float32, device=x.device)
        conv3d_forward(x, _ncdhw(cin, V), weight, bias, out, _rows3(cout, V), B, cin, cout, (D, H, W), False)
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        B, cin, D, H, W = (int(s) for s in x.shape)
        cout, V = int(weight.shape[0]), D * H * W
        need_dw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (ctx.needs_input_grad[0] or need_dw):
            return None, None, None
        dout = _rows(dout, "dout")
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, db = conv3d_backward(x, _ncdhw(cin, V), weight, dout, _rows3(_ld(dout), V), dx, _ncdhw(cin, V), B, cin, cout, (D, H, W),
                                 False, need_dw)
        return dx, dw, db


class _ConvTranspose3d(Function):
    """nn.ConvTranspose3d(k 3, p 1, s 1) on NCDHW tensors."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, cin, D, H, W = (int(s) for s in x.shape)
        cout, V = int(weight.shape[1]), D * H * W
        out = torch.empty((B, cout, D, H, W), dtype=torch.float32, device=x.device)
        conv3d_forward(x, _ncdhw(cin, V), weight, bias, out, _ncdhw(cout, V), B, cin, cout, (D, H, W), True)
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        B, cin, D, H, W = (int(s) for s in x.shape)
        cout, V = int(weight.shape[1]), D * H * W
        need_dw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (ctx.needs_input_grad[0] or need_dw):
            return None, None, None
        dout = dout.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, db = conv3d_backward(x, _ncdhw(cin, V), weight, dout, _ncdhw(cout, V), dx, _ncdhw(cin, V), B, cin, cout, (D, H, W), True,
                                 need_dw)
        return dx, dw, db


def _conv_input(x: torch.Tensor, channels: int, name: str) -> torch.Tensor:
    _need_hip(x, name)
    if x.dim() != 5 or int(x.shape[1]) != channels:
        raise RuntimeError("graph_weather_amd: %s must be [batch, %d, depth, height, width], got %s" % (name, channels, tuple(x.shape)))
    return x.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------------
def _check_dropout(module: nn.Module) -> None:
    """Before anything else in a forward: the unsupported mode is reported whatever the input is."""
    if not module.training:
        return
    for m in module.modules():
        p = m.p if isinstance(m, nn.Dropout) else (m.dropout if isinstance(m, nn.MultiheadAttention) else 0.0)
        if p > 0:
            raise NotImplementedError("graph_weather_amd: dropout > 0 in train() mode is not implemented (use dropout = 0 or eval())")


def _mha_rows(mha: nn.MultiheadAttention, x2: torch.Tensor, batch: int, n: int, key_bias: Optional[torch.Tensor]) -> torch.Tensor:
    """out_proj(attention(in_proj(x))) of a self-attention over the n rows of every sample; x2 [(b, n), embed_dim]."""
    heads = int(mha.num_heads)
    dim_head = int(mha.embed_dim) // heads
    qkv = _Linear.apply(x2, mha.in_proj_weight, mha.in_proj_bias, False)
    if key_bias is None:
        o = _Attention.apply(qkv, batch, heads, n, dim_head, dim_head**-0.5)
    else:
        o = _MaskedAttention.apply(qkv, key_bias, batch, heads, n, dim_head, dim_head**-0.5)
    return _Linear.apply(o, mha.out_proj.weight, mha.out_proj.bias, False)


def _check_mha(mha: nn.MultiheadAttention) -> None:
    _check_dim_head(int(mha.embed_dim) // int(mha.num_heads))


def _encoder_layer_rows(layer: nn.TransformerEncoderLayer, x2: torch.Tensor, batch: int, n: int,
                        key_bias: Optional[torch.Tensor]) -> torch.Tensor:
    """A post-norm ``nn.TransformerEncoderLayer``: norm1(x + attention(x)), norm2(x + linear2(act(linear1(x))))."""
    if layer.norm_first:
        raise NotImplementedError("graph_weather_amd: norm_first transformer layers are not implemented")
    x2 = _ln(layer.norm1, _Add.apply(x2, _mha_rows(layer.self_attn, x2, batch, n, key_bias)))
    if layer.activation is F.relu or isinstance(layer.activation, nn.ReLU):
        h = _Linear.apply(x2, layer.linear1.weight, layer.linear1.bias, True)
    elif layer.activation is F.gelu or isinstance(layer.activation, nn.GELU):
        h = _Gelu.apply(_Linear.apply(x2, layer.linear1.weight, layer.linear1.bias, False))
    else:
        raise NotImplementedError("graph_weather_amd: transformer activations other than relu and gelu are not implemented")
    h = _Linear.apply(h, layer.linear2.weight, layer.linear2.bias, False)
    return _ln(layer.norm2, _Add.apply(x2, h))


# ---------------------------------------------------------------------------------------------------------------------
# AuroraModel
# ---------------------------------------------------------------------------------------------------------------------
class PointEncoder(nn.Module):
    def __init__(self, input_features: int, embed_dim: int, max_seq_len: int = 1024):
        super().__init__()
        self.input_dim = input_features + 2  # Account for lat/lon coordinates
        self.max_seq_len = max_seq_len
        self.coord_encoder = nn.Sequential(
            nn.Linear(2, embed_dim // 2),
            nn.LayerNorm(embed_dim // 2),
            nn.ReLU(),
            nn.Linear(embed_dim // 2, embed_dim),
        )
        self.feature_encoder = nn.Sequential(
            nn.Linear(input_features, embed_dim),
            nn.LayerNorm(embed_dim),
            nn.ReLU(),
            nn.Linear(embed_dim, embed_dim),
        )
        self.norm = nn.LayerNorm(embed_dim)

    def forward(self, points: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
        _need_hip(points, "points")
        _need_hip(features, "features")
        if points.shape[1] > self.max_seq_len:
            points = points[:, : self.max_seq_len, :]
            features = features[:, : self.max_seq_len, :]
        b, n = int(points.shape[0]), int(points.shape[1])
        return self.rows(points, features.reshape(b * n, -1)).reshape(b, n, -1)

    @staticmethod
    def _branch(seq: nn.Sequential, x2: torch.Tensor) -> torch.Tensor:
        h = _Linear.apply(x2, seq[0].weight, seq[0].bias, False)
        h = _Relu.apply(_ln(seq[1], h))
        return _Linear.apply(h, seq[3].weight, seq[3].bias, False)

    def rows(self, points: torch.Tensor, features2: torch.Tensor) -> torch.Tensor:
        """points [b, n, 2] in degrees, features [(b, n), input_features] -> [(b, n), embed_dim]."""
        normalized = torch.stack([points[..., 0] / 180.0, points[..., 1] / 90.0], dim=-1)  # on the raw input, as the reference
        coord = self._branch(self.coord_encoder, normalized.reshape(-1, 2))
        feat = self._branch(self.feature_encoder, features2)
        return _ln(self.norm, _Add.apply(coord, feat))


class PointDecoder(nn.Module):
    """Decodes latent representations back to point features."""

    def __init__(self, embed_dim: int, output_features: int):
        super().__init__()
        self.decoder = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, output_features))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _need_hip(x, "x")
        shape = x.shape
        return self.rows(x.reshape(-1, shape[-1])).reshape(*shape[:-1], -1)

    def rows(self, x2: torch.Tensor) -> torch.Tensor:
        h = _Linear.apply(x2, self.decoder[0].weight, self.decoder[0].bias, True)
        return _Linear.apply(h, self.decoder[2].weight, self.decoder[2].bias, False)


class SelfAttentionLayer(nn.Module):
    def __init__(self, embed_dim: int):
        super().__init__()
        self.attention = nn.MultiheadAttention(embed_dim, num_heads=8)  # the parameters only: its forward is never called
        _check_mha(self.attention)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.ffn = nn.Sequential(nn.Linear(embed_dim, 4 * embed_dim), nn.ReLU(), nn.Linear(4 * embed_dim, embed_dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _need_hip(x, "x")
        b, n, d = (int(s) for s in x.shape)
        return self.rows(x.reshape(b * n, d), b, n).reshape(b, n, d)

    def rows(self, x2: torch.Tensor, batch: int, n: int) -> torch.Tensor:
        x2 = _ln(self.norm1, _Add.apply(x2, _mha_rows(self.attention, x2, batch, n, None)))
        h = _Linear.apply(x2, self.ffn[0].weight, self.ffn[0].bias, True)
        h = _Linear.apply(h, self.ffn[2].weight, self.ffn[2].bias, False)
        return _ln(self.norm2, _Add.apply(x2, h))


class PointCloudProcessor(nn.Module):
    """Processes point cloud data using self-attention layers."""

    def __init__(self, embed_dim: int, num_layers: int = 4):
        super().__init__()
        self.layers = nn.ModuleList([SelfAttentionLayer(embed_dim) for _ in range(num_layers)])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _need_hip(x, "x")
        b, n, d = (int(s) for s in x.shape)
        return self.rows(x.reshape(b * n, d), b, n).reshape(b, n, d)

    def rows(self, x2: torch.Tensor, batch: int, n: int) -> torch.Tensor:
        for layer in self.layers:
            x2 = layer.rows(x2, batch, n)
        return x2


class AuroraModel(nn.Module):
    def __init__(
        self,
        input_features: int,
        output_features: int,
        latent_dim: int = 256,
        num_layers: int = 4,
        max_points: int = 10000,
        max_seq_len: int = 1024,
        use_checkpointing: bool = False,
    ):
        super().__init__()
        self.max_points = max_points
        self.max_seq_len = max_seq_len
        self.input_features = input_features
        self.output_features = output_features
        self.encoder = PointEncoder(input_features, latent_dim, max_seq_len)
        self.processor = PointCloudProcessor(latent_dim, num_layers)
        self.decoder = PointDecoder(latent_dim, output_features)
        self.use_checkpointing = use_checkpointing
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, points: torch.Tensor, features: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if points.shape[1] > self.max_points:
            raise ValueError(f"Number of points ({points.shape[1]}) exceeds maximum ({self.max_points})")
        _need_hip(points, "points")
        _need_hip(features, "features")
        b, n_in = int(points.shape[0]), int(points.shape[1])
        factor = None
        if mask is not None:
            factor = mask.float().reshape(-1)
            points = _RowScale.apply(points.reshape(b * n_in, -1), factor).reshape(points.shape)
            features = _RowScale.apply(features.reshape(b * n_in, -1), factor).reshape(features.shape)
        if n_in > self.max_seq_len:  # the encoder's truncation
            points = points[:, : self.max_seq_len, :]
            features = features[:, : self.max_seq_len, :]
        n = int(points.shape[1])
        x2 = self.encoder.rows(points, features.reshape(b * n, -1))
        if self.use_checkpointing and self.training:
            from torch.utils.checkpoint import checkpoint

            x2 = checkpoint(self.processor.rows, x2, b, n, use_reentrant=False)
        else:
            x2 = self.processor.rows(x2, b, n)
        out2 = self.decoder.rows(x2)
        if factor is not None:
            out2 = _RowScale.apply(out2, factor)  # with truncated points this raises, as the reference's broadcast does
        return out2.reshape(b, n, -1)


class EarthSystemLoss(nn.Module):
    def __init__(self, alpha: float = 0.5, beta: float = 0.3, gamma: float = 0.2):
        super().__init__()
        self.alpha = alpha
        self.beta = beta
        self.gamma = gamma

    @staticmethod
    def _inputs(pred, target, points):
        _need_hip(pred, "pred")
        _need_hip(points, "points")
        if pred.dim() != 3 or points.dim() != 3 or int(points.shape[-1]) != 2 or tuple(points.shape[:2]) != tuple(pred.shape[:2]):
            raise RuntimeError("graph_weather_amd: EarthSystemLoss expects pred [batch, points, channels] and points [batch, points, 2]")
        if target is not None:
            _need_hip(target, "target")
            if tuple(target.shape) != tuple(pred.shape):
                raise RuntimeError("graph_weather_amd: pred and target must have the same shape")
            target = target.contiguous()
        return pred.contiguous(), target, points.contiguous()

    @staticmethod
    def _one_sample(points):
        if int(points.shape[0]) != 1:  # the reference's view of a [B N, B N] distance matrix as [B, N, N] fails
            raise RuntimeError("graph_weather_amd: the spatial correlation loss takes one sample (batch size 1), as the reference")

    def spatial_correlation_loss(self, pred: torch.Tensor, target: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
        self._one_sample(points)
        pred, target, points = self._inputs(pred, target, points)
        return _EarthLoss.apply(pred, target, points, True, self.alpha, self.beta, self.gamma)[2]

    def physical_loss(self, pred: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
        """Calculate physical consistency loss - ensures predictions follow basic physical laws"""
        pred, _, points = self._inputs(pred, None, points)
        return _EarthLoss.apply(pred, None, points, False, self.alpha, self.beta, self.gamma)[3]

    def forward(self, pred: torch.Tensor, target: torch.Tensor, points: torch.Tensor) -> dict:
        self._one_sample(points)
        pred, target, points = self._inputs(pred, target, points)
        out = _EarthLoss.apply(pred, target, points, True, self.alpha, self.beta, self.gamma)
        return {
            "total_loss": out[0],
            "mse_loss": out[1],
            "spatial_correlation_loss": out[2],
            "physical_loss": out[3],
        }


# ---------------------------------------------------------------------------------------------------------------------
# Swin3DEncoder, Decoder3D
# ---------------------------------------------------------------------------------------------------------------------
class Swin3DEncoder(nn.Module):
    """Conv3d, LayerNorm, then the four post-norm encoder layers and the final norm of an ``nn.Transformer`` over all voxels of a
    sample (the reference performs no windowing).  The transformer's decoder half is held as parameters only, as there."""

    def __init__(self, in_channels=1, embed_dim=96):
        super().__init__()
        self.conv1 = nn.Conv3d(in_channels, embed_dim, kernel_size=3, padding=1, stride=1)
        self.norm = nn.LayerNorm(embed_dim)
        self.swin_transformer = nn.Transformer(  # the parameters only: its forward is never called
            d_model=embed_dim,
            nhead=8,
            num_encoder_layers=4,
            num_decoder_layers=4,
            dim_feedforward=embed_dim * 4,
        )
        for layer in self.swin_transformer.encoder.layers:
            _check_mha(layer.self_attn)
        self.embed_dim = embed_dim

    def forward(self, x):
        """[batch, in_channels, d, h, w] -> [batch, d * h * w, embed_dim]"""
        _check_dropout(self)
        x = _conv_input(x, int(self.conv1.in_channels), "x")
        b, _, d, h, w = (int(s) for s in x.shape)
        return self.transformer_rows(self.normalization_rows(self.convolution_rows(x)), b, d * h * w).reshape(b, d * h * w, -1)

    def convolution_rows(self, x: torch.Tensor) -> torch.Tensor:
        """conv1 -> channels-last rows [(b, d, h, w), embed_dim]"""
        return _Conv3dRows.apply(x, self.conv1.weight, self.conv1.bias)

    def normalization_rows(self, x2: torch.Tensor) -> torch.Tensor:
        return _ln(self.norm, x2)

    def transformer_rows(self, x2: torch.Tensor, batch: int, n: int) -> torch.Tensor:
        enc = self.swin_transformer.encoder
        for layer in enc.layers:
            x2 = _encoder_layer_rows(layer, x2, batch, n, None)
        return x2 if enc.norm is None else _ln(enc.norm, x2)

    def convolution(self, x):
        """Apply 3D convolution: b c d h w -> b embed_dim d h w."""
        _check_dropout(self)
        x = _conv_input(x, int(self.conv1.in_channels), "x")
        b, _, d, h, w = (int(s) for s in x.shape)
        return self.convolution_rows(x).reshape(b, d, h, w, -1).permute(0, 4, 1, 2, 3).contiguous()

    def normalization_layer(self, x):
        """b c d h w -> b d h w c, normalised over c."""
        _check_dropout(self)
        _need_hip(x, "x")
        b, c, d, h, w = (int(s) for s in x.shape)
        return self.normalization_rows(x.permute(0, 2, 3, 4, 1).reshape(b * d * h * w, c)).reshape(b, d, h, w, c)

    def transformer_encoder(self, x, spatial_dims):
        """b d h w c -> b d h w c through the encoder."""
        _check_dropout(self)
        _need_hip(x, "x")
        d, h, w = spatial_dims
        b, c = int(x.shape[0]), int(x.shape[-1])
        return self.transformer_rows(x.reshape(b * d * h * w, c), b, d * h * w).reshape(b, d, h, w, c)


class Decoder3D(nn.Module):
    """The latent rows reinterpreted (a view, not a transpose) as [batch, embed_dim, D, H, W], then ConvTranspose3d(k 3, p 1)."""

    def __init__(self, output_channels=1, embed_dim=96, target_shape=(32, 32, 32)):
        super().__init__()
        self.embed_dim = embed_dim
        self.target_shape = target_shape
        self.deconv1 = nn.ConvTranspose3d(embed_dim, output_channels, kernel_size=3, padding=1, stride=1)

    def forward(self, x):
        """[batch, seq_len, embed_dim] -> [batch, output_channels, *target_shape]"""
        batch_size = x.shape[0]
        depth, height, width = self.target_shape
        x = x.view(batch_size, self.embed_dim, depth, height, width)  # raises RuntimeError on a non-contiguous input, as the reference
        _need_hip(x, "x")
        return _ConvTranspose3d.apply(x, self.deconv1.weight, self.deconv1.bias)


# ---------------------------------------------------------------------------------------------------------------------
# PerceiverProcessor
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ProcessorConfig:
    input_dim: int = 256  # Match Swin3D output
    latent_dim: int = 512
    d_model: int = 256  # Match input_dim for consistency
    max_seq_len: int = 4096
    num_self_attention_layers: int = 6
    num_cross_attention_layers: int = 2
    num_attention_heads: int = 8
    hidden_dropout: float = 0.1
    attention_dropout: float = 0.1
    qk_head_dim: Optional[int] = 32
    activation_fn: str = "gelu"
    layer_norm_eps: float = 1e-12

    def __post_init__(self):
        if self.input_dim <= 0:
            raise ValueError("input_dim must be positive")
        if self.max_seq_len <= 0:
            raise ValueError("max_seq_len must be positive")
        if self.num_attention_heads <= 0:
            raise ValueError("num_attention_heads must be positive")
        if not 0 <= self.hidden_dropout <= 1:
            raise ValueError("hidden_dropout must be between 0 and 1")
        if not 0 <= self.attention_dropout <= 1:
            raise ValueError("attention_dropout must be between 0 and 1")


class PerceiverProcessor(nn.Module):
    def __init__(self, config: Optional[ProcessorConfig] = None):
        super().__init__()
        self.config = config or ProcessorConfig()
        self.input_projection = nn.Linear(self.config.input_dim, self.config.d_model)
        # the parameters only (layer_norm_eps and attention_dropout of the config are unused, as in the reference)
        self.encoder = nn.TransformerEncoder(
            nn.TransformerEncoderLayer(
                d_model=self.config.d_model,
                nhead=self.config.num_attention_heads,
                dim_feedforward=self.config.d_model * 4,
                dropout=self.config.hidden_dropout,
                activation=self.config.activation_fn,
            ),
            num_layers=self.config.num_self_attention_layers,
            enable_nested_tensor=False,  # a torch fast-path switch without a parameter (sequence-first layers cannot use it anyway)
        )
        for layer in self.encoder.layers:
            _check_mha(layer.self_attn)
        self.output_projection = nn.Linear(self.config.d_model, self.config.latent_dim)

    def forward(self, x, attention_mask=None):
        _check_dropout(self)
        if x.dim() != 3:  # the reference's rearrange "b s h w -> b (s h w) c" names an axis its input does not have
            raise RuntimeError("graph_weather_amd: PerceiverProcessor expects [batch, sequence, input_dim], got %d dimensions" % x.dim())
        _need_hip(x, "x")
        b, s, d = (int(v) for v in x.shape)
        key_bias = None
        if attention_mask is not None:  # True keeps a key: an additive 0 / -inf bias on the keys of every query and head
            if tuple(attention_mask.shape) != (b, s):
                raise RuntimeError("graph_weather_amd: attention_mask must be [batch, sequence]")
            key_bias = torch.zeros((b, s), dtype=torch.float32, device=x.device).masked_fill(~attention_mask.to(x.device).bool(),
                                                                                             float("-inf"))
        x2 = _Linear.apply(x.reshape(b * s, d), self.input_projection.weight, self.input_projection.bias, False)
        for layer in self.encoder.layers:
            x2 = _encoder_layer_rows(layer, x2, b, s, key_bias)
        x2 = _Linear.apply(x2, self.output_projection.weight, self.output_projection.bias, False)
        return _TokenMean.apply(x2, b, s)


__version__ = "0.1.0"

# Default configurations for different model sizes (the reference's table: its keys are not AuroraModel's arguments, so
# create_model raises TypeError unless every one of them is overridden - there as here)
MODEL_CONFIGS = {
    "tiny": {"in_channels": 1, "out_channels": 1, "embed_dim": 48, "latent_dim": 256, "spatial_shape": (16, 16, 16), "max_seq_len": 2048},
    "base": {"in_channels": 1, "out_channels": 1, "embed_dim": 96, "latent_dim": 512, "spatial_shape": (32, 32, 32), "max_seq_len": 4096},
    "large": {"in_channels": 1, "out_channels": 1, "embed_dim": 192, "latent_dim": 1024, "spatial_shape": (64, 64, 64),
              "max_seq_len": 8192},
}


def create_model(config="base", **kwargs):
    """An AuroraModel from a named configuration, keywords overriding it."""
    if config not in MODEL_CONFIGS:
        raise ValueError(f"Unknown configuration: {config}. Choose from {list(MODEL_CONFIGS.keys())}")
    model_config = MODEL_CONFIGS[config].copy()
    model_config.update(kwargs)
    return AuroraModel(**model_config)


def create_loss(alpha=0.5, beta=0.3, gamma=0.2):
    """An EarthSystemLoss with the given weights."""
    return EarthSystemLoss(alpha=alpha, beta=beta, gamma=gamma)


__all__ = [
    "AuroraModel",
    "EarthSystemLoss",
    "Swin3DEncoder",
    "Decoder3D",
    "PerceiverProcessor",
]
