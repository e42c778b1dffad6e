"""The WeatherMesh model (``graph_weather/models/weathermesh``): ``ConvDownBlock`` and ``ConvUpBlock`` (layers.py),
``WeatherMeshEncoder`` (encoder.py), ``WeatherMeshDecoder`` (decoder.py) and ``WeatherMesh`` (weathermesh2.py) with their configs,
with the reference's constructor arguments, attribute names, ``state_dict`` keys and key order.  The processor and the
``NeighborhoodAttention3D`` layer are those of ``weathermesh.py``.

The children of a block are real ``nn.Conv2d/3d(bias=False)`` and ``nn.BatchNorm2d/3d``, so reference checkpoints load with
``strict=True``; they hold the parameters and buffers and are never called.  A block's forward is one ``autograd.Function`` on
the kernels of ``csrc/gw_convnd.hip``::

    y1 = conv1(x)                      stride 1        st1 = statistics of bn1 over y1
    y2 = conv2(gelu(bn1(y1)))          the block's stride; the normalised and activated copy is formed on load, never stored
    ys = skip(x)                       1 x 1, the block's stride
    out = gelu(bn2(y2) + bn_skip(ys))  one launch

Saved for the backward are x (the upsampled x of a ``ConvUpBlock``), y1, y2, ys and the three statistics tables [4, C]
(scale, shift, mean, rstd) - no normalised or activated copy.  The backward recomputes gelu' from them: one reduction launch and
one apply launch per BatchNorm pair, a weight gradient per convolution (slab partials added in order) and the data gradients, run
per input-parity class where the stride is 2.  A ``ConvUpBlock`` materialises the 2 x upsampled volume once (conv1 and the 1 x 1
skip both read it).  fp32 only; there is no CPU path.

Quirks of the reference that are kept:

* ``WeatherMesh.processors`` is a plain Python list: the processors are absent from ``state_dict()`` and ``parameters()``, and
  ``.to()`` / ``.cuda()`` / ``.train()`` / ``.eval()`` do not reach them - move and switch them yourself.
* The decoder doubles ``n_conv_blocks`` times what the encoder halved with ``(L - 1) // 2 + 1``: the output height and width are
  ``2^n H'``, larger than the input's when H or W is not a multiple of ``2^n``.
* ``n_pressure_levels`` is accepted and unused.

``to_latent`` and ``split`` are 1 x 1 x 1 convolutions, hence pointwise: ``to_latent`` reads the pressure volume and the surface
plane where they lie and writes the D planes and the surface plane (the LAST depth index) of the channels-last latent
[B, D + 1, H', W', latent_dim] in two launches - there is no ``torch.cat`` and no rearrange copy; ``split`` reads the latent rows
in place and writes the pressure volume and the surface plane as two contiguous tensors.
"""
import ctypes
import dataclasses
import typing
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .ops import on_device_of
from .wide import _L, _st
from .weathermesh import NeighborhoodAttention3D, WeatherMeshProcessor, WeatherMeshProcessorConfig

__all__ = ["ConvDownBlock", "ConvUpBlock", "WeatherMeshEncoder", "WeatherMeshEncoderConfig", "WeatherMeshDecoder",
           "WeatherMeshDecoderConfig", "WeatherMesh", "WeatherMeshConfig", "WeatherMeshOutput", "conv_out_length", "convnd_forward",
           "convnd_dgrad", "convnd_wgrad", "bn_stats", "tail_forward", "tail_backward", "upsample2x_forward", "upsample2x_backward",
           "UPSAMPLE_TAPS"]

# output 2 i reads (i - 1, i) with these weights, output 2 i + 1 reads (i, i + 1) with them reversed; indices clamped to the axis
UPSAMPLE_TAPS = (0.25, 0.75)


def conv_out_length(length: int, stride: int) -> int:
    """Output length of the padded 3-tap (padding 1) and of the unpadded 1-tap convolution with ``stride``."""
    return (length - 1) // stride + 1


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _need_hip(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"graph_weather_amd: {name} must live on a HIP device (no CPU path exists)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"graph_weather_amd: {name} must be float32, got {t.dtype}")


def _i3(t) -> ctypes.Array:
    return (ctypes.c_int64 * 3)(*(int(v) for v in t))


def _triple(v, rank: int, name: str) -> Tuple[int, int, int]:
    """An int or ``rank`` ints as (depth, height, width); a 2-D value gets depth 1."""
    v = (int(v),) * rank if isinstance(v, int) else tuple(int(t) for t in v)
    if len(v) != rank:
        raise ValueError("graph_weather_amd: %s must be an int or %d ints, got %r" % (name, rank, v))
    return (1,) * (3 - rank) + v


def _vol(t: torch.Tensor):
    """(tensor, (batch, channel, voxel) strides, (D, H, W)) of a [B, C, (D,) H, W] tensor; a view whose voxels are evenly spaced
    (NCDHW, channels-last, a range of depth planes of a larger buffer) is taken as it lies, anything else is copied."""
    for attempt in range(2):
        sizes, strides = tuple(t.shape[2:]), tuple(t.stride()[2:])
        sv = next((s for n, s in zip(reversed(sizes), reversed(strides)) if n > 1), 1)
        expect, ok = sv, sv > 0
        for n, s in zip(reversed(sizes), reversed(strides)):
            ok = ok and (n == 1 or s == expect)
            expect *= n
        if ok:
            break
        t = t.contiguous()
    dhw = (1,) * (3 - len(sizes)) + tuple(int(n) for n in sizes)
    return t, (int(t.stride(0)), int(t.stride(1)), int(sv)), dhw


def _geo(batch: int, cin: int, cout: int, dhw, kernel, stride) -> ctypes.Array:
    return (ctypes.c_int32 * 12)(batch, cin, cout, *dhw, *kernel, *stride)


def _kernel_of(weight: torch.Tensor) -> Tuple[int, int, int]:
    return (1,) * (5 - weight.dim()) + tuple(int(k) for k in weight.shape[2:])


def _out_shape(x_shape, cout: int, stride) -> Tuple[int, ...]:
    rank = len(x_shape) - 2
    return (int(x_shape[0]), cout) + tuple(conv_out_length(int(n), s) for n, s in zip(x_shape[2:], stride[3 - rank:]))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def convnd_forward(x: torch.Tensor, weight: torch.Tensor, stride, bias: Optional[torch.Tensor] = None,
                   bn: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Conv2d / nn.Conv3d(kernel 1 or 3, padding k // 2, stride 1 or 2 per axis) of x [B, cin, (D,) H, W] (include/gw_amd.h:
    gw_convnd_forward).  ``bn``: a statistics table [4, cin]; the convolution then reads gelu(x scale + shift).  ``out``: a
    [B, cout, ...] view to write into (any evenly spaced layout), else a new contiguous tensor."""
    _need_hip(x, "x")
    rank = x.dim() - 2
    stride = _triple(stride, rank, "stride")
    x, sx, dhw = _vol(x)
    weight = weight.contiguous()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    shape = _out_shape(x.shape, cout, stride)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape:
        raise RuntimeError("graph_weather_amd: out must be %s, got %s" % (shape, tuple(out.shape)))
    o, so, _ = _vol(out)
    if o is not out:
        raise RuntimeError("graph_weather_amd: the voxels of out must be evenly spaced")
    geo = _geo(int(x.shape[0]), cin, cout, dhw, _kernel_of(weight), stride)
    with on_device_of(x):
        _lib.check(_L().gw_convnd_forward(geo, _lib.CONVND_A_PLAIN if bn is None else _lib.CONVND_A_BN_GELU, x.data_ptr(), _i3(sx),
                                          _ptr(bn), None if bn is None else bn[1].data_ptr(), weight.data_ptr(),
                                          None if bias is None else bias.contiguous().data_ptr(), out.data_ptr(), _i3(so), _st(x)),
                   "gw_convnd_forward")
    return out


def convnd_dgrad(dout: torch.Tensor, weight: torch.Tensor, stride, x_shape, dx: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """The gradient at the convolution's input [B, cin, (D,) H, W] = ``x_shape`` from dout (gw_convnd_dgrad): one launch per
    parity class of the strided axes.  ``dx`` (with ``accumulate``: added to) may be an evenly spaced view."""
    _need_hip(dout, "dout")
    rank = dout.dim() - 2
    stride = _triple(stride, rank, "stride")
    weight = weight.contiguous()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if dx is None:
        dx = torch.empty(tuple(int(s) for s in x_shape), dtype=torch.float32, device=dout.device)
    dout, sd, _ = _vol(dout)
    d, sdx, dhw = _vol(dx)
    if d is not dx:
        raise RuntimeError("graph_weather_amd: the voxels of dx must be evenly spaced")
    geo = _geo(int(dx.shape[0]), cin, cout, dhw, _kernel_of(weight), stride)
    with on_device_of(dout):
        _lib.check(_L().gw_convnd_dgrad(geo, dout.data_ptr(), _i3(sd), weight.data_ptr(), dx.data_ptr(), _i3(sdx),
                                        1 if accumulate else 0, _st(dout)), "gw_convnd_dgrad")
    return dx


def convnd_wgrad(x: torch.Tensor, dout: torch.Tensor, weight_shape, stride, bn: Optional[torch.Tensor] = None,
                 need_bias: bool = False):
    """(dweight, dbias or None) of the convolution from its input x (read through ``bn`` like the forward) and dout
    (gw_convnd_wgrad): slab partials in a workspace, added in slab order."""
    _need_hip(x, "x")
    rank = x.dim() - 2
    stride = _triple(stride, rank, "stride")
    x, sx, dhw = _vol(x)
    dout, sd, _ = _vol(dout)
    cout, cin = int(weight_shape[0]), int(weight_shape[1])
    kernel = (1,) * (3 - rank) + tuple(int(k) for k in weight_shape[2:])
    geo = _geo(int(x.shape[0]), cin, cout, dhw, kernel, stride)
    nbytes = int(_L().gw_convnd_workspace_bytes(geo))
    if nbytes == 0:
        _lib.check(-1, "gw_convnd_workspace_bytes")
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device)
    dw = torch.empty(tuple(int(s) for s in weight_shape), dtype=torch.float32, device=x.device)
    db = torch.empty((cout,), dtype=torch.float32, device=x.device) if need_bias else None
    with on_device_of(x):
        _lib.check(_L().gw_convnd_wgrad(geo, _lib.CONVND_A_PLAIN if bn is None else _lib.CONVND_A_BN_GELU, x.data_ptr(), _i3(sx),
                                        _ptr(bn), None if bn is None else bn[1].data_ptr(), dout.data_ptr(), _i3(sd), ws.data_ptr(),
                                        nbytes, dw.data_ptr(), _ptr(db), _st(x)), "gw_convnd_wgrad")
    return dw, db


def _values_per_channel(shape) -> int:
    n = int(shape[0])
    for s in shape[2:]:
        n *= int(s)
    return n


def bn_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float, training: bool,
             running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor]) -> torch.Tensor:
    """The statistics table [4, C] = (scale, shift, mean, rstd) of a BatchNorm over x [B, C, ...] (gw_convnd_bn_stats).
    ``training``: batch statistics, and the running buffers (when given) are updated in place; else the table is that of the
    running buffers and x is not read."""
    _need_hip(x, "x")
    if training and _values_per_channel(x.shape) == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (torch.Size(x.shape),))
    x, sx, dhw = _vol(x)
    C = int(x.shape[1])
    stats = torch.empty((4, C), dtype=torch.float32, device=x.device)
    with on_device_of(x):
        _lib.check(_L().gw_convnd_bn_stats(int(x.shape[0]), C, dhw[0] * dhw[1] * dhw[2], 1 if training else 0, x.data_ptr(), _i3(sx),
                                           gamma.data_ptr(), beta.data_ptr(), float(eps), float(momentum), _ptr(running_mean),
                                           _ptr(running_var), stats.data_ptr(), _st(x)), "gw_convnd_bn_stats")
    return stats


def tail_forward(y2: torch.Tensor, st2: torch.Tensor, ys: Optional[torch.Tensor] = None, sts: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gelu(y2 scale2 + shift2 + ys scales + shifts) (gw_convnd_tail_forward); ``ys`` None: the first two terms."""
    _need_hip(y2, "y2")
    y2, s2, dhw = _vol(y2)
    if out is None:
        out = torch.empty(tuple(y2.shape), dtype=torch.float32, device=y2.device)
    o, so, _ = _vol(out)
    if o is not out or tuple(out.shape) != tuple(y2.shape):
        raise RuntimeError("graph_weather_amd: out must be shaped like y2 with evenly spaced voxels")
    ss = None
    if ys is not None:
        ys, ss, _ = _vol(ys)
    with on_device_of(y2):
        _lib.check(_L().gw_convnd_tail_forward(int(y2.shape[0]), int(y2.shape[1]), dhw[0] * dhw[1] * dhw[2], y2.data_ptr(), _i3(s2),
                                               st2.data_ptr(), _ptr(ys), None if ss is None else _i3(ss), _ptr(sts), out.data_ptr(),
                                               _i3(so), _st(y2)), "gw_convnd_tail_forward")
    return out


def tail_backward(dout: torch.Tensor, y2: torch.Tensor, st2: torch.Tensor, ys: Optional[torch.Tensor], sts: Optional[torch.Tensor],
                  training: bool):
    """(sums [4, C], dy2, dys) of ``tail_forward`` (gw_convnd_tail_backward): sums = (d beta2, d gamma2, d betas, d gammas), the last
    two and dys only with ``ys``."""
    _need_hip(dout, "dout")
    dout, sd, _ = _vol(dout)
    y2, s2, dhw = _vol(y2)
    C = int(y2.shape[1])
    sums = torch.empty((4, C), dtype=torch.float32, device=y2.device)
    dy2 = torch.empty(tuple(y2.shape), dtype=torch.float32, device=y2.device)
    dys = ss = None
    if ys is not None:
        ys, ss, _ = _vol(ys)
        dys = torch.empty(tuple(ys.shape), dtype=torch.float32, device=y2.device)
    with on_device_of(y2):
        _lib.check(_L().gw_convnd_tail_backward(int(y2.shape[0]), C, dhw[0] * dhw[1] * dhw[2], 1 if training else 0, dout.data_ptr(),
                                                _i3(sd), y2.data_ptr(), _i3(s2), st2.data_ptr(), _ptr(ys),
                                                None if ss is None else _i3(ss), _ptr(sts), sums.data_ptr(), dy2.data_ptr(),
                                                _i3(_vol(dy2)[1]), _ptr(dys), None if dys is None else _i3(_vol(dys)[1]), _st(y2)),
                   "gw_convnd_tail_backward")
    return sums, dy2, dys


def _upsample(x: torch.Tensor, out: torch.Tensor, backward: bool) -> torch.Tensor:
    lo, hi = (out, x) if backward else (x, out)
    x, sx, _ = _vol(x)
    _, so, _ = _vol(out)
    dhw = _vol(lo)[2]
    with on_device_of(x):
        _lib.check(_L().gw_convnd_upsample2x(int(lo.shape[0]), int(lo.shape[1]), *dhw, 1 if backward else 0, x.data_ptr(), _i3(sx),
                                             out.data_ptr(), _i3(so), _st(x)), "gw_convnd_upsample2x")
    return out


def upsample2x_forward(x: torch.Tensor) -> torch.Tensor:
    """F.interpolate(scale_factor=2, mode="bilinear") of [B, C, H, W], or (1, 2, 2) trilinear of [B, C, D, H, W]; align_corners
    False (gw_convnd_upsample2x).  x may be an evenly spaced view."""
    _need_hip(x, "x")
    shape = tuple(int(s) for s in x.shape[:-2]) + (2 * int(x.shape[-2]), 2 * int(x.shape[-1]))
    return _upsample(x, torch.empty(shape, dtype=torch.float32, device=x.device), False)


def upsample2x_backward(dout: torch.Tensor) -> torch.Tensor:
    """The gradient at the source of ``upsample2x_forward``: every source voxel gathers the (at most 4 x 4) upsampled voxels that
    read it, with the clamped border reads included."""
    _need_hip(dout, "dout")
    shape = tuple(int(s) for s in dout.shape[:-2]) + (int(dout.shape[-2]) // 2, int(dout.shape[-1]) // 2)
    return _upsample(dout, torch.empty(shape, dtype=torch.float32, device=dout.device), True)


# ---------------------------------------------------------------------------------------------------------------------
# the residual block
# ---------------------------------------------------------------------------------------------------------------------
class _Norm:
    """What the block's Function needs of a BatchNorm child besides its parameters."""

    def __init__(self, bn: nn.modules.batchnorm._BatchNorm):
        self.eps, self.momentum = bn.eps, bn.momentum
        self.batch = bn.training or bn.running_mean is None
        self.running_mean, self.running_var = bn.running_mean, bn.running_var

    def stats(self, y, gamma, beta):
        return bn_stats(y, gamma, beta, self.eps, self.momentum, self.batch, self.running_mean, self.running_var)


class _ResBlock(Function):
    """gelu(bn2(conv2(gelu(bn1(conv1(x))))) + bn_skip(skip(x))), on the upsampled x when ``up``."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, ws, gs, bs, stride, up: bool, n1: _Norm, n2: _Norm, nsk: _Norm):
        xin = upsample2x_forward(x) if up else x
        y1 = convnd_forward(xin, w1, 1)
        st1 = n1.stats(y1, g1, b1)
        y2 = convnd_forward(y1, w2, stride, bn=st1)
        st2 = n2.stats(y2, g2, b2)
        ys = convnd_forward(xin, ws, stride)
        sts = nsk.stats(ys, gs, bs)
        out = tail_forward(y2, st2, ys, sts)
        ctx.meta = (stride, up, n1.batch, n2.batch)
        ctx.save_for_backward(xin, y1, y2, ys, st1, st2, sts, w1, w2, ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        xin, y1, y2, ys, st1, st2, sts, w1, w2, ws = ctx.saved_tensors
        stride, up, batch1, batch2 = ctx.meta
        sums, dy2, dys = tail_backward(dout, y2, st2, ys, sts, batch2)
        dw2, _ = convnd_wgrad(y1, dy2, w2.shape, stride, bn=st1)
        da1 = convnd_dgrad(dy2, w2, stride, y1.shape)
        sums1, dy1, _ = tail_backward(da1, y1, st1, None, None, batch1)
        dw1, _ = convnd_wgrad(xin, dy1, w1.shape, 1)
        dws, _ = convnd_wgrad(xin, dys, ws.shape, stride)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = convnd_dgrad(dy1, w1, 1, xin.shape)
            convnd_dgrad(dys, ws, stride, xin.shape, dx=dx, accumulate=True)
            if up:
                dx = upsample2x_backward(dx)
        return (dx, dw1, sums1[1], sums1[0], dw2, sums[1], sums[0], dws, sums[3], sums[2]) + (None,) * 5


def _check_block(kernel_size, padding, groups, activation) -> None:
    if groups != 1:
        raise NotImplementedError("graph_weather_amd: grouped convolutions are not built, got groups %r" % (groups,))
    if any(k != 3 for k in (kernel_size if isinstance(kernel_size, (tuple, list)) else (kernel_size,))):
        raise NotImplementedError("graph_weather_amd: block kernel sizes other than 3 are not built, got %r" % (kernel_size,))
    if any(p != 1 for p in (padding if isinstance(padding, (tuple, list)) else (padding,))):
        raise NotImplementedError("graph_weather_amd: block paddings other than 1 are not built, got %r" % (padding,))
    if not isinstance(activation, nn.GELU) or activation.approximate != "none":
        raise NotImplementedError("graph_weather_amd: activations other than nn.GELU(approximate='none') are not built, got %r"
                                  % (activation,))


class _ResidualBlock(nn.Module):
    """The forward both blocks share; the children are named by the subclasses."""

    _skip = ("", "")  # names of the 1 x 1 convolution and of its BatchNorm

    def _run(self, x: torch.Tensor, stride, up: bool) -> torch.Tensor:
        rank = 3 if isinstance(self.conv1, nn.Conv3d) else 2
        skip, bn_skip = getattr(self, self._skip[0]), getattr(self, self._skip[1])
        if x.dim() != rank + 2 or int(x.shape[1]) != self.conv1.in_channels:
            raise ValueError("graph_weather_amd: %s expects [batch, %d, %s], got %s"
                             % (type(self).__name__, self.conv1.in_channels, "depth, height, width" if rank == 3 else "height, width",
                                tuple(x.shape)))
        norms = [_Norm(self.bn1), _Norm(self.bn2), _Norm(bn_skip)]
        if norms[1].batch != norms[2].batch:
            raise NotImplementedError("graph_weather_amd: bn2 and the skip's BatchNorm in different modes are not built")
        if any(n.batch and n.momentum is None for n in norms):
            raise NotImplementedError("graph_weather_amd: BatchNorm with momentum=None (cumulative average) is not built")
        spatial = tuple(int(s) * (2 if up and i >= rank - 2 else 1) for i, s in enumerate(x.shape[2:]))
        s3 = _triple(stride, rank, "stride")
        inner = (int(x.shape[0]), self.conv1.out_channels) + spatial
        outer = _out_shape(inner, self.conv2.out_channels, s3)
        for n, shape in zip(norms, (inner, outer, outer)):
            if n.batch and _values_per_channel(shape) == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (torch.Size(shape),))
        _need_hip(x, "x")
        out = _ResBlock.apply(x, self.conv1.weight, self.bn1.weight, self.bn1.bias, self.conv2.weight, self.bn2.weight, self.bn2.bias,
                              skip.weight, bn_skip.weight, bn_skip.bias, s3[3 - rank:], up, *norms)
        for bn in (self.bn1, self.bn2, bn_skip):
            if bn.training and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
        return out


class ConvDownBlock(_ResidualBlock):
    """Downsampling convolutional block with residual connection (layers.py); 2-D or 3-D inputs.
    ``act(bn2(conv2(act(bn1(conv1(x))))) + bn_down(downsample(x)))``: conv1 has stride 1, conv2 and downsample the block's."""

    _skip = ("downsample", "bn_down")

    def __init__(self, in_channels: int, out_channels: int, is_3d: bool = False, kernel_size: int = 3, stride: int = 2,
                 padding: int = 1, groups: int = 1, activation: nn.Module = nn.GELU()):
        super().__init__()
        _check_block(kernel_size, padding, groups, activation)
        rank = 3 if is_3d else 2
        if any(s not in (1, 2) for s in _triple(stride, rank, "stride")):
            raise NotImplementedError("graph_weather_amd: strides other than 1 and 2 are not built, got %r" % (stride,))
        Conv = nn.Conv3d if is_3d else nn.Conv2d
        Norm = nn.BatchNorm3d if is_3d else nn.BatchNorm2d
        self.conv1 = Conv(in_channels, out_channels, kernel_size=kernel_size, stride=1, padding=padding, groups=groups, bias=False)
        self.bn1 = Norm(out_channels)
        self.activation1 = activation
        self.conv2 = Conv(out_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, groups=groups,
                          bias=False)
        self.bn2 = Norm(out_channels)
        self.activation2 = activation
        self.downsample = Conv(in_channels, out_channels, kernel_size=1, stride=stride, bias=False)
        self.bn_down = Norm(out_channels)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, self.conv2.stride, False)


class ConvUpBlock(_ResidualBlock):
    """Upsampling convolutional block with residual connection (layers.py): 2 x bilinear upsampling of height and width, then
    the residual pattern of ``ConvDownBlock`` at stride 1 with conv1 in -> in, conv2 in -> out and the 1 x 1 ``upsample``."""

    _skip = ("upsample", "bn_up")

    def __init__(self, in_channels: int, out_channels: int, is_3d: bool = False, kernel_size: int = 3, scale_factor: int = 2,
                 padding: int = 1, groups: int = 1, activation: nn.Module = nn.GELU()):
        super().__init__()
        _check_block(kernel_size, padding, groups, activation)
        if scale_factor != 2:
            raise NotImplementedError("graph_weather_amd: scale factors other than 2 are not built, got %r" % (scale_factor,))
        Conv = nn.Conv3d if is_3d else nn.Conv2d
        Norm = nn.BatchNorm3d if is_3d else nn.BatchNorm2d
        self.is_3d = is_3d
        self.scale_factor = scale_factor
        self.conv1 = Conv(in_channels, in_channels, kernel_size=kernel_size, stride=1, padding=padding, groups=groups, bias=False)
        self.bn1 = Norm(in_channels)
        self.activation1 = activation
        self.conv2 = Conv(in_channels, out_channels, kernel_size=kernel_size, stride=1, padding=padding, groups=groups, bias=False)
        self.bn2 = Norm(out_channels)
        self.activation2 = activation
        self.upsample = Conv(in_channels, out_channels, kernel_size=1, stride=1, bias=False)
        self.bn_up = Norm(out_channels)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, 1, True)


# ---------------------------------------------------------------------------------------------------------------------
# to_latent and split: pointwise convolutions between the two towers' tensors and the channels-last latent rows
# ---------------------------------------------------------------------------------------------------------------------
def _latent_views(latent: torch.Tensor):
    """The pressure planes [:, :-1] and the surface plane [:, -1] of a contiguous latent [B, D + 1, H, W, L] as channel-first
    views [B, L, D, H, W] and [B, L, H, W] (channel stride 1: the rows are read and written in place)."""
    vol = latent.permute(0, 4, 1, 2, 3)
    return vol[:, :, :-1], vol[:, :, -1]


class _ToLatent(Function):
    """Conv3d(C, L, 1) of cat([pressure, surface.unsqueeze(2)], 2), rearranged "B C D H W -> B D H W C"."""

    @staticmethod
    def forward(ctx, pressure, surface, weight, bias):
        B, C, D, H, W = (int(s) for s in pressure.shape)
        latent = torch.empty((B, D + 1, H, W, int(weight.shape[0])), dtype=torch.float32, device=pressure.device)
        lp, ls = _latent_views(latent)
        convnd_forward(pressure, weight, 1, bias=bias, out=lp)
        convnd_forward(surface, weight.view(weight.shape[:2] + (1, 1)), 1, bias=bias, out=ls)
        ctx.save_for_backward(pressure, surface, weight)
        return latent

    @staticmethod
    def backward(ctx, dlatent):
        pressure, surface, weight = ctx.saved_tensors
        dp, ds = _latent_views(dlatent.contiguous())
        w2 = weight.view(weight.shape[:2] + (1, 1))
        dwp, dbp = convnd_wgrad(pressure, dp, weight.shape, 1, need_bias=True)
        dws, dbs = convnd_wgrad(surface, ds, w2.shape, 1, need_bias=True)
        dpress = convnd_dgrad(dp, weight, 1, pressure.shape) if ctx.needs_input_grad[0] else None
        dsurf = convnd_dgrad(ds, w2, 1, surface.shape) if ctx.needs_input_grad[1] else None
        return dpress, dsurf, dwp + dws.view(weight.shape), dbp + dbs


class _Split(Function):
    """Conv3d(L, C, 1) of the latent rearranged "B D H W C -> B C D H W", returned as its planes [:-1] and its plane [-1]."""

    @staticmethod
    def forward(ctx, latent, weight, bias):
        latent = latent.contiguous()
        lp, ls = _latent_views(latent)
        w2 = weight.view(weight.shape[:2] + (1, 1))
        pressure, surface = convnd_forward(lp, weight, 1, bias=bias), convnd_forward(ls, w2, 1, bias=bias)
        ctx.save_for_backward(latent, weight)
        return pressure, surface

    @staticmethod
    def backward(ctx, dpressure, dsurface):
        latent, weight = ctx.saved_tensors
        lp, ls = _latent_views(latent)
        w2 = weight.view(weight.shape[:2] + (1, 1))
        dwp, dbp = convnd_wgrad(lp, dpressure, weight.shape, 1, need_bias=True)
        dws, dbs = convnd_wgrad(ls, dsurface, w2.shape, 1, need_bias=True)
        dlatent = None
        if ctx.needs_input_grad[0]:
            dlatent = torch.empty_like(latent)
            dlp, dls = _latent_views(dlatent)
            convnd_dgrad(dpressure, weight, 1, lp.shape, dx=dlp)
            convnd_dgrad(dsurface, w2, 1, ls.shape, dx=dls)
        return dlatent, dwp + dws.view(weight.shape), dbp + dbs


# ---------------------------------------------------------------------------------------------------------------------
# configs
# ---------------------------------------------------------------------------------------------------------------------
_PLAIN = {"int": int, "tuple": tuple}


def _convert(name: str, want, value):
    """``value`` as a field of type ``want``, as ``dacite.from_dict`` converts it: a dict for a dataclass, a list of converted
    items for ``List[...]``, anything else type-checked and kept."""
    if isinstance(want, str):
        want = _PLAIN.get(want, object)
    if dataclasses.is_dataclass(want):
        if isinstance(value, want):
            return value
        if isinstance(value, dict):
            return _from_dict(want, value)
    elif typing.get_origin(want) is list:
        if isinstance(value, list):
            return [_convert(name, typing.get_args(want)[0], v) for v in value]
    elif isinstance(value, want):
        return value
    raise TypeError('wrong value type for field "%s" - should be "%s" instead of value "%r" of type "%s"'
                    % (name, getattr(want, "__name__", str(want)), value, type(value).__name__))


def _from_dict(cls, data: dict):
    """Every field is required, values are type-checked, further keys are ignored."""
    values = {}
    for f in dataclasses.fields(cls):
        if f.name not in data:
            raise ValueError('missing value for field "%s"' % f.name)
        values[f.name] = _convert(f.name, f.type, data[f.name])
    return cls(**values)


@dataclass
class WeatherMeshEncoderConfig:
    input_channels_2d: int
    input_channels_3d: int
    latent_dim: int
    n_pressure_levels: int
    num_conv_blocks: int
    hidden_dim: int
    kernel_size: tuple
    num_heads: int
    num_transformer_layers: int

    @staticmethod
    def from_json(json: dict) -> "WeatherMeshEncoderConfig":
        return _from_dict(WeatherMeshEncoderConfig, json)

    def to_json(self) -> dict:
        return dataclasses.asdict(self)


@dataclass
class WeatherMeshDecoderConfig:
    latent_dim: int
    output_channels_2d: int
    output_channels_3d: int
    n_conv_blocks: int
    hidden_dim: int
    kernel_size: tuple
    num_heads: int
    num_transformer_layers: int

    @staticmethod
    def from_json(json: dict) -> "WeatherMeshDecoderConfig":
        return _from_dict(WeatherMeshDecoderConfig, json)

    def to_json(self) -> dict:
        return dataclasses.asdict(self)


@dataclass
class WeatherMeshConfig:
    encoder: WeatherMeshEncoderConfig
    processors: List[WeatherMeshProcessorConfig]
    decoder: WeatherMeshDecoderConfig
    timesteps: List[int]
    surface_channels: int
    pressure_channels: int
    pressure_levels: int
    latent_dim: int
    encoder_num_conv_blocks: int
    encoder_num_transformer_layers: int
    encoder_hidden_dim: int
    decoder_num_conv_blocks: int
    decoder_num_transformer_layers: int
    decoder_hidden_dim: int
    processor_num_layers: int
    kernel: tuple
    num_heads: int

    @staticmethod
    def from_json(json: dict) -> "WeatherMeshConfig":
        return _from_dict(WeatherMeshConfig, json)

    def to_json(self) -> dict:
        return dataclasses.asdict(self)


@dataclass
class WeatherMeshOutput:
    surface: torch.Tensor
    pressure: torch.Tensor


# ---------------------------------------------------------------------------------------------------------------------
# encoder, decoder, model
# ---------------------------------------------------------------------------------------------------------------------
class WeatherMeshEncoder(nn.Module):
    """encoder.py: ``num_conv_blocks`` 2-D down blocks on the surface field [B, input_channels_2d, H, W], as many 3-D down blocks
    with stride (1, 2, 2) on the pressure volume [B, input_channels_3d, D, H, W], ``to_latent`` over the pressure planes with the
    surface plane appended as the last depth index, then ``num_transformer_layers`` of neighbourhood attention on the
    channels-last latent [B, D + 1, H', W', latent_dim]."""

    def __init__(self, input_channels_2d: int, input_channels_3d: int, latent_dim: int, n_pressure_levels: int,
                 num_conv_blocks: int = 3, hidden_dim: int = 256, kernel_size: tuple = (5, 7, 7), num_heads: int = 8,
                 num_transformer_layers: int = 3):
        super().__init__()
        self.surface_path = nn.ModuleList(
            [ConvDownBlock(input_channels_2d if i == 0 else hidden_dim * (2 ** i), hidden_dim * (2 ** (i + 1)))
             for i in range(num_conv_blocks)])
        self.pressure_path = nn.ModuleList(
            [ConvDownBlock(input_channels_3d if i == 0 else hidden_dim * (2 ** i), hidden_dim * (2 ** (i + 1)), stride=(1, 2, 2),
                           is_3d=True) for i in range(num_conv_blocks)])
        self.transformer_layers = nn.ModuleList(
            [NeighborhoodAttention3D(embed_dim=latent_dim, kernel_size=kernel_size, num_heads=num_heads)
             for _ in range(num_transformer_layers)])
        self.to_latent = nn.Conv3d(hidden_dim * (2 ** num_conv_blocks), latent_dim, kernel_size=1)

    def forward(self, surface: torch.Tensor, pressure: torch.Tensor) -> torch.Tensor:
        if surface.dim() != 4 or pressure.dim() != 5 or surface.shape[0] != pressure.shape[0] or surface.shape[2:] != pressure.shape[3:]:
            raise ValueError("graph_weather_amd: WeatherMeshEncoder expects surface [B, C2, H, W] and pressure [B, C3, D, H, W], got %s "
                             "and %s" % (tuple(surface.shape), tuple(pressure.shape)))
        for block in self.surface_path:
            surface = block(surface)
        for block in self.pressure_path:
            pressure = block(pressure)
        _need_hip(surface, "surface")
        _need_hip(pressure, "pressure")
        if int(pressure.shape[1]) != self.to_latent.in_channels:
            raise ValueError("graph_weather_amd: to_latent expects %d channels, got %d" % (self.to_latent.in_channels, pressure.shape[1]))
        latent = _ToLatent.apply(pressure, surface, self.to_latent.weight, self.to_latent.bias)
        for transformer in self.transformer_layers:
            latent = transformer(latent)
        return latent


class WeatherMeshDecoder(nn.Module):
    """decoder.py: ``num_transformer_layers`` of neighbourhood attention on the latent [B, D + 1, H', W', latent_dim], ``split``,
    then ``n_conv_blocks`` 3-D up blocks on the planes [:-1] and as many 2-D up blocks on the plane [-1].  Returns
    (surface [B, output_channels_2d, 2^n H', 2^n W'], pressure [B, output_channels_3d, D, 2^n H', 2^n W']), contiguous."""

    def __init__(self, latent_dim, output_channels_2d, output_channels_3d, n_conv_blocks=3, hidden_dim=256,
                 kernel_size: tuple = (5, 7, 7), num_heads: int = 8, num_transformer_layers: int = 3):
        super().__init__()
        self.transformer_layers = nn.ModuleList(
            [NeighborhoodAttention3D(embed_dim=latent_dim, num_heads=num_heads, kernel_size=kernel_size)
             for _ in range(num_transformer_layers)])
        self.split = nn.Conv3d(latent_dim, hidden_dim * (2 ** n_conv_blocks), kernel_size=1)
        self.pressure_path = nn.ModuleList(
            [ConvUpBlock(hidden_dim * (2 ** (i + 1)), hidden_dim * (2 ** i) if i > 0 else output_channels_3d, is_3d=True)
             for i in reversed(range(n_conv_blocks))])
        self.surface_path = nn.ModuleList(
            [ConvUpBlock(hidden_dim * (2 ** (i + 1)), hidden_dim * (2 ** i) if i > 0 else output_channels_2d)
             for i in reversed(range(n_conv_blocks))])

    def forward(self, latent: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if latent.dim() != 5 or int(latent.shape[-1]) != self.split.in_channels or int(latent.shape[1]) < 2:
            raise ValueError("graph_weather_amd: WeatherMeshDecoder expects a latent [B, D + 1, H, W, %d] with D >= 1, got %s"
                             % (self.split.in_channels, tuple(latent.shape)))
        for transformer in self.transformer_layers:
            latent = transformer(latent)
        _need_hip(latent, "latent")
        pressure_features, surface_features = _Split.apply(latent, self.split.weight, self.split.bias)
        for block in self.pressure_path:
            pressure_features = block(pressure_features)
        for block in self.surface_path:
            surface_features = block(surface_features)
        return surface_features, pressure_features


class WeatherMesh(nn.Module):
    """weathermesh2.py: encoder, ``forecast_steps`` rounds over all processors, decoder.  ``processors`` is a plain list (see the
    module docstring): not in ``state_dict()``, not moved by ``.to()``."""

    def __init__(self, encoder: Optional[nn.Module], processors: Optional[List[nn.Module]], decoder: Optional[nn.Module],
                 timesteps: List[int], surface_channels: Optional[int], pressure_channels: Optional[int], pressure_levels: Optional[int],
                 latent_dim: Optional[int], encoder_num_conv_blocks: Optional[int], encoder_num_transformer_layers: Optional[int],
                 encoder_hidden_dim: Optional[int], decoder_num_conv_blocks: Optional[int],
                 decoder_num_transformer_layers: Optional[int], decoder_hidden_dim: Optional[int], processor_num_layers: Optional[int],
                 kernel: Optional[tuple], num_heads: Optional[int]):
        super().__init__()
        if encoder is not None:
            self.encoder = encoder
        else:
            self.encoder = WeatherMeshEncoder(input_channels_2d=surface_channels, input_channels_3d=pressure_channels,
                                              latent_dim=latent_dim, n_pressure_levels=pressure_levels,
                                              num_conv_blocks=encoder_num_conv_blocks, hidden_dim=encoder_hidden_dim, kernel_size=kernel,
                                              num_heads=num_heads, num_transformer_layers=encoder_num_transformer_layers)
        if processors is not None:
            assert len(processors) == len(timesteps), "Number of processors must match number of timesteps"
            self.processors = processors
        else:
            self.processors = [WeatherMeshProcessor(latent_dim=latent_dim, n_layers=processor_num_layers, kernel=kernel,
                                                    num_heads=num_heads) for _ in range(len(timesteps))]
        if decoder is not None:
            self.decoder = decoder
        else:
            self.decoder = WeatherMeshDecoder(latent_dim=latent_dim, output_channels_2d=surface_channels,
                                              output_channels_3d=pressure_channels, n_conv_blocks=decoder_num_conv_blocks,
                                              hidden_dim=decoder_hidden_dim, kernel_size=kernel, num_heads=num_heads,
                                              num_transformer_layers=decoder_num_transformer_layers)
        self.timesteps = timesteps

    def forward(self, surface: torch.Tensor, pressure: torch.Tensor, forecast_steps: int) -> WeatherMeshOutput:
        latent = self.encoder(surface, pressure)
        for _ in range(forecast_steps):
            for processor in self.processors:
                latent = processor(latent)
        surface_out, pressure_out = self.decoder(latent)
        return WeatherMeshOutput(surface=surface_out, pressure=pressure_out)
