"""``ThermalizerLayer`` / ``AdaptiveUNet`` (reference ``graph_weather/models/layers/thermalizer.py``) on the HIP kernels of
``csrc/gw_thermal.hip``.

Same submodule names, ``state_dict`` keys, attributes, grid inference, errors and warning as the reference.  Activations
live as NHWC pixel rows ``[B * H * W, C]`` (the processor's node rows already are that), so the layer reads its input in place
and never permutes.  Every convolution is an implicit GEMM on fp32 MFMAs; GroupNorm + ReLU are applied by the consumer's
operand load; ``cat`` is two producers writing channel slices of one buffer; the noisy input and the two position channels
are formed by the first convolution's load and never stored, and the last stage writes ``(noisy - s1 * eps_hat) / sa``.

The thermalizer always runs in fp32, whatever ``set_compute_dtype`` chose for the message-passing MLPs (fp32, bf16x3 or
bf16): at 1 degree, batch 2 its matrix work is about 3.5 GFLOP against the forecast step's 766 GFLOP.

The noise is drawn with ``torch.randn`` on the device in row layout (plumbing: graph replays draw fresh noise through torch's
graph-safe generator); ``last_noise`` keeps the noise rows of the latest call (after a graph replay: that replay's buffer).
"""
from __future__ import annotations

import functools
import math
import warnings
from typing import List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from ._lib import (GwThermalConvArgs, GwThermalTaps, THERMAL_A_DIFFUSE, THERMAL_A_GN_RELU, THERMAL_A_PLAIN, THERMAL_E_DIFFUSE,
                   THERMAL_E_STORE, THERMAL_ROWS_AXPY, THERMAL_ROWS_FINALIZE, THERMAL_ROWS_SCALE)
from .ops import _stream, on_device_of

class _V:
    """Pixel rows of an image batch: ``t`` holds them from column ``off`` on, ``ld`` floats apart, ``c`` channels."""

    __slots__ = ("t", "off", "ld", "c", "B", "H", "W")

    def __init__(self, t: torch.Tensor, off: int, ld: int, c: int, B: int, H: int, W: int):
        self.t, self.off, self.ld, self.c, self.B, self.H, self.W = t, off, ld, c, B, H, W

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * self.off

    @property
    def rows(self) -> int:
        return self.B * self.H * self.W


def _new(B, H, W, C, dev, zero=False) -> _V:
    t = (torch.zeros if zero else torch.empty)(B * H * W, C, dtype=torch.float32, device=dev)
    return _V(t, 0, C, C, B, H, W)


@functools.lru_cache(maxsize=4096)
def _live(taps: Tuple[Tuple[int, int], ...], scale: int, q: int, size: int) -> Tuple[Tuple[int, int], ...]:
    """The (input offset, weight index) taps that hit the image for some GEMM pixel q in [0, q)."""
    return tuple(t for t in taps if any(0 <= scale * i + t[0] < size for i in range(q)))


def _taps(live) -> GwThermalTaps:
    tp = GwThermalTaps()
    tp.n = len(live)
    for i, (o, w) in enumerate(live):
        tp.in_off[i] = o
        tp.w_idx[i] = w
    return tp


def _check(rc, what):
    _lib.check(rc, what)


class _Ends:
    """The diffusion step around the score model: clean rows ``x`` (ld), noise rows ``eps`` [rows, F], sa, s1."""

    __slots__ = ("x", "ld", "eps", "sa", "s1", "F")

    def __init__(self, x, ld, eps, sa, s1, F):
        self.x, self.ld, self.eps, self.sa, self.s1, self.F = x, ld, eps, sa, s1, F


def _conv_call(inp: _V, a_mode: int, ss, w: torch.Tensor, wstr, bias, geo, cin: int, cout: int, out_t, ld_out: int,
               ends: Optional[_Ends], e_mode: int) -> GwThermalConvArgs:
    (in_h, in_w), (out_h, out_w), (q_h, q_w), (si_h, si_w), (so_h, so_w), (oo_h, oo_w), ty, tx = geo
    a = GwThermalConvArgs()
    a.batch, a.in_h, a.in_w, a.out_h, a.out_w, a.q_h, a.q_w = inp.B, in_h, in_w, out_h, out_w, q_h, q_w
    a.in_scale_h, a.in_scale_w, a.out_scale_h, a.out_scale_w, a.out_off_h, a.out_off_w = si_h, si_w, so_h, so_w, oo_h, oo_w
    a.ty, a.tx = _taps(ty), _taps(tx)
    a.cin, a.cout, a.a_mode, a.e_mode = cin, cout, a_mode, e_mode
    a.a, a.ld_a = inp.ptr, inp.ld
    if ss is not None:
        a.a_scale, a.a_shift = ss[0].data_ptr(), ss[1].data_ptr()
    a.w = w.data_ptr()
    a.w_stride_y, a.w_stride_x, a.w_stride_ci, a.w_stride_co = wstr
    a.bias = None if bias is None else bias.data_ptr()
    a.out, a.ld_out = out_t, ld_out
    if ends is not None:
        a.features, a.eps, a.sa, a.s1 = ends.F, ends.eps.data_ptr(), ends.sa, ends.s1
        a.x, a.ld_x = ends.x.data_ptr(), ends.ld
    return a


def _conv_geo(B, H, W, k):
    p = k // 2
    taps = tuple((t - p, t) for t in range(k))
    return ((H, W), (H, W), (H, W), (1, 1), (1, 1), (0, 0), _live(taps, 1, H, H), _live(taps, 1, W, W))


def _tap_major(w: torch.Tensor, ci_dim: int, co_dim: int):
    """The weight as [ky][kx][GEMM ci][GEMM co] (a copy, so that the 64 lanes of a B-tile load read 64 consecutive floats)
    and its strides (y, x, ci, co)."""
    wt = w.detach().permute(2, 3, ci_dim, co_dim).contiguous()
    k, _, ci, co = (int(s) for s in wt.shape)
    return wt, (k * ci * co, ci * co, co, 1)


def _conv_args(inp: _V, a_mode, ss, w, bias, out: Optional[_V], ends=None, e_mode=THERMAL_E_STORE, out_ptr=None, ld_out=None,
               packed=None):
    """Arguments of Conv2d(w) on ``inp``.  ``packed`` = _tap_major(w, 1, 0) for a forward launch; without it the weight strides
    are w's own (OIHW), the layout the weight gradient is written in."""
    co, ci, k, _ = (int(s) for s in w.shape)
    geo = _conv_geo(inp.B, inp.H, inp.W, k)
    wt, wstr = packed if packed is not None else (w, (k, 1, k * k, ci * k * k))
    return _conv_call(inp, a_mode, ss, wt, wstr, bias, geo, ci, co,
                      out.ptr if out_ptr is None else out_ptr, out.ld if ld_out is None else ld_out, ends, e_mode)


def conv(inp: _V, a_mode, ss, w, bias, out: Optional[_V] = None, ends=None, e_mode=THERMAL_E_STORE, out_ptr=None, ld_out=None):
    """Conv2d(k, padding k // 2) of ``inp`` (through its GroupNorm + ReLU when ``ss`` is given) -> ``out``."""
    if out is None and out_ptr is None:
        out = _new(inp.B, inp.H, inp.W, int(w.shape[0]), inp.t.device)
    packed = _tap_major(w, 1, 0)
    a = _conv_args(inp, a_mode, ss, w, bias, out, ends, e_mode, out_ptr, ld_out, packed=packed)
    _check(_lib.lib().gw_thermal_conv_forward(a, _stream(inp.t)), "gw_thermal_conv_forward")
    return out


def _wgrad(a: GwThermalConvArgs, dw: torch.Tensor, dev):
    L = _lib.lib()
    nb = L.gw_thermal_conv_wgrad_workspace_bytes(a)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    _check(L.gw_thermal_conv_wgrad(a, ws.data_ptr(), nb, dw.data_ptr(), _stream(dw)), "gw_thermal_conv_wgrad")


def colsum(g: _V, out: torch.Tensor):
    L = _lib.lib()
    nb = L.gw_thermal_colsum_workspace_bytes(g.rows, g.c)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=out.device)
    _check(L.gw_thermal_colsum(g.rows, g.c, g.ptr, g.ld, ws.data_ptr(), nb, out.data_ptr(), _stream(out)), "gw_thermal_colsum")


def conv_backward(inp: _V, a_mode, ss, w, g: _V, want_dx: bool, dx_channels: int, ends=None, want_bias=True):
    """Gradients of ``conv``: (dx [rows, dx_channels] dense or None, dw, db).  ``g`` = gradient of the conv output."""
    co, ci, k, _ = (int(s) for s in w.shape)
    dev = inp.t.device
    dw = torch.zeros_like(w)
    a = _conv_args(inp, a_mode, ss, w, None, None, ends, THERMAL_E_STORE, out_ptr=g.ptr, ld_out=g.ld)
    _wgrad(a, dw, dev)
    db = None
    if want_bias:
        db = torch.empty(co, dtype=torch.float32, device=dev)
        colsum(g, db)
    dx = None
    if want_dx:
        p = k // 2
        taps = tuple((t - p, k - 1 - t) for t in range(k))
        H, W = inp.H, inp.W
        geo = ((H, W), (H, W), (H, W), (1, 1), (1, 1), (0, 0), _live(taps, 1, H, H), _live(taps, 1, W, W))
        dx = _new(inp.B, H, W, dx_channels, dev)
        wt, wstr = _tap_major(w, 0, 1)  # GEMM ci = the conv's output channel
        b = _conv_call(g, THERMAL_A_PLAIN, None, wt, wstr, None, geo, co, dx_channels, dx.ptr, dx.ld, None, THERMAL_E_STORE)
        _check(_lib.lib().gw_thermal_conv_forward(b, _stream(dx.t)), "gw_thermal_conv_forward (input gradient)")
    return dx, dw, db


_PARITY_TAPS = {0: ((0, 1),), 1: ((1, 0), (0, 2))}  # ConvTranspose2d(3, 2, 1, 1): output 2q + r reads input q + off, weight idx


def _convt_geo(B, H, W, ry, rx):
    ty = _live(_PARITY_TAPS[ry], 1, H, H)
    tx = _live(_PARITY_TAPS[rx], 1, W, W)
    return ((H, W), (2 * H, 2 * W), (H, W), (1, 1), (2, 2), (ry, rx), ty, tx)


def conv_transpose(inp: _V, ss, w, bias, out_ptr: int, ld_out: int, ends=None, e_mode=THERMAL_E_STORE):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) of relu(GroupNorm(inp)) as four output-parity convolutions
    writing the 2H x 2W image at ``out_ptr`` (row stride ld_out)."""
    ci, co = int(w.shape[0]), int(w.shape[1])
    L = _lib.lib()
    wt, wstr = _tap_major(w, 0, 1)
    for ry in (0, 1):
        for rx in (0, 1):
            geo = _convt_geo(inp.B, inp.H, inp.W, ry, rx)
            a = _conv_call(inp, THERMAL_A_GN_RELU, ss, wt, wstr, bias, geo, ci, co, out_ptr, ld_out, ends, e_mode)
            _check(L.gw_thermal_conv_forward(a, _stream(inp.t)), "gw_thermal_conv_forward (transpose)")


def conv_transpose_backward(inp: _V, ss, w, g: _V):
    """Gradients of ``conv_transpose``: (dx = gradient of relu(GroupNorm(inp)) [rows, ci] dense, dw, db)."""
    ci, co = int(w.shape[0]), int(w.shape[1])
    dev = inp.t.device
    dw = torch.zeros_like(w)
    for ry in (0, 1):
        for rx in (0, 1):
            geo = _convt_geo(inp.B, inp.H, inp.W, ry, rx)
            a = _conv_call(inp, THERMAL_A_GN_RELU, ss, w, (3, 1, co * 9, 9), None, geo, ci, co, g.ptr, g.ld, None,
                           THERMAL_E_STORE)
            _wgrad(a, dw, dev)
    db = torch.empty(co, dtype=torch.float32, device=dev)
    colsum(g, db)
    H, W = inp.H, inp.W
    taps = ((-1, 0), (0, 1), (1, 2))  # input q reads output 2q + k - 1 through weight k
    geo = ((2 * H, 2 * W), (H, W), (H, W), (2, 2), (1, 1), (0, 0), _live(taps, 2, H, 2 * H), _live(taps, 2, W, 2 * W))
    dx = _new(inp.B, H, W, ci, dev)
    gin = _V(g.t, g.off, g.ld, co, inp.B, 2 * H, 2 * W)
    wt, wstr = _tap_major(w, 1, 0)  # GEMM ci = the transpose's output channel
    b = _conv_call(gin, THERMAL_A_PLAIN, None, wt, wstr, None, geo, co, ci, dx.ptr, dx.ld, None, THERMAL_E_STORE)
    _check(_lib.lib().gw_thermal_conv_forward(b, _stream(dx.t)), "gw_thermal_conv_forward (transpose input gradient)")
    return dx, dw, db


def group_norm(x: _V, gn: nn.GroupNorm):
    """Statistics of GroupNorm(x): (stats [B, G, 2] = (mean, rstd), scale [B, C], shift [B, C])."""
    L = _lib.lib()
    B, C, G = x.B, x.c, int(gn.num_groups)
    dev = x.t.device
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=dev)
    scale = torch.empty(B * C, dtype=torch.float32, device=dev)
    shift = torch.empty(B * C, dtype=torch.float32, device=dev)
    nb = L.gw_thermal_groupnorm_workspace_bytes(B, x.H * x.W, C, G)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    _check(L.gw_thermal_groupnorm_forward(B, x.H * x.W, C, G, x.ptr, x.ld, gn.weight.data_ptr(), gn.bias.data_ptr(), float(gn.eps),
                                          ws.data_ptr(), nb, stats.data_ptr(), scale.data_ptr(), shift.data_ptr(), _stream(x.t)),
           "gw_thermal_groupnorm_forward")
    return stats, (scale, shift)


def group_norm_backward(x: _V, gn: nn.GroupNorm, stats, ss, dy: _V):
    """dy = gradient of relu(GroupNorm(x)) -> (dx [rows, C] dense, dgamma, dbeta)."""
    L = _lib.lib()
    B, C, G = x.B, x.c, int(gn.num_groups)
    dev = x.t.device
    dx = _new(B, x.H, x.W, C, dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    nb = L.gw_thermal_groupnorm_workspace_bytes(B, x.H * x.W, C, G)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    _check(L.gw_thermal_groupnorm_backward(B, x.H * x.W, C, G, x.ptr, x.ld, ss[0].data_ptr(), ss[1].data_ptr(), stats.data_ptr(),
                                           gn.weight.data_ptr(), dy.ptr, dy.ld, ws.data_ptr(), nb, dx.ptr, dgamma.data_ptr(),
                                           dbeta.data_ptr(), _stream(dx.t)), "gw_thermal_groupnorm_backward")
    return dx, dgamma, dbeta


def _pooled(n: int) -> int:
    return (n - 1) // 2 + 1


def max_pool(x: _V, ss, out: _V) -> torch.Tensor:
    idx = torch.empty(out.rows, x.c, dtype=torch.int32, device=x.t.device)
    _check(_lib.lib().gw_thermal_maxpool_forward(x.B, x.H, x.W, x.c, x.ptr, x.ld, ss[0].data_ptr(), ss[1].data_ptr(), out.ptr, out.ld,
                                                 idx.data_ptr(), _stream(x.t)), "gw_thermal_maxpool_forward")
    return idx


def max_pool_backward(x: _V, idx, g1: _V, g2: Optional[_V]) -> _V:
    dx = _new(x.B, x.H, x.W, x.c, x.t.device)
    _check(_lib.lib().gw_thermal_maxpool_backward(x.B, x.H, x.W, x.c, idx.data_ptr(), g1.ptr, g1.ld, None if g2 is None else g2.ptr,
                                                  0 if g2 is None else g2.ld, dx.ptr, _stream(dx.t)), "gw_thermal_maxpool_backward")
    return dx


def resize(x: _V, out: _V):
    _check(_lib.lib().gw_thermal_resize_forward(x.B, x.H, x.W, out.H, out.W, x.c, x.ptr, x.ld, out.ptr, out.ld, _stream(x.t)),
           "gw_thermal_resize_forward")


def resize_backward(x: _V, g: _V) -> _V:
    dx = _new(x.B, x.H, x.W, x.c, x.t.device)
    _check(_lib.lib().gw_thermal_resize_backward(x.B, x.H, x.W, g.H, g.W, x.c, g.ptr, g.ld, dx.ptr, _stream(dx.t)),
           "gw_thermal_resize_backward")
    return dx


def rows_op(mode: int, rows: int, F: int, sa: float, s1: float, p, ld_p, q, ld_q, r, ld_r, out, ld_out, like: torch.Tensor):
    _check(_lib.lib().gw_thermal_rows(mode, rows, F, sa, s1, p, ld_p, q, ld_q, r, ld_r, out, ld_out, _stream(like)), "gw_thermal_rows")


# ------------------------------------------------------------------------------------------------------------ score model


def _simple_params(net: nn.Sequential) -> List[torch.Tensor]:
    return [net[0].weight, net[0].bias, net[1].weight, net[1].bias, net[3].weight, net[3].bias, net[4].weight, net[4].bias,
            net[6].weight, net[6].bias, net[7].weight, net[7].bias, net[9].weight, net[9].bias]


_UNET_BLOCKS = ("conv1", "conv2", "conv3", "upconv3", "upconv2", "upconv1")


def _layers(name: str) -> Tuple[int, ...]:
    return (0, 1, 3, 4, 6) if name.startswith("up") else (0, 1, 3, 4)  # (contract blocks end in a MaxPool2d)


def _unet_params(m: "AdaptiveUNet") -> List[torch.Tensor]:
    ps = []
    for name in _UNET_BLOCKS:
        blk = getattr(m, name)
        for i in _layers(name):
            ps += [blk[i].weight, blk[i].bias]
    return ps


def _first_input(x: _V, ends: Optional[_Ends]):
    return THERMAL_A_PLAIN if ends is None else THERMAL_A_DIFFUSE


def _simple_forward(m: "AdaptiveUNet", x: _V, ends, out_t, ld_out, tape):
    net = m.simple_net
    cin0 = int(net[0].weight.shape[1])
    x0 = _V(x.t, x.off, x.ld, cin0, x.B, x.H, x.W)
    h = conv(x0, _first_input(x, ends), None, net[0].weight, net[0].bias, ends=ends)
    st, ss = group_norm(h, net[1])
    tape += [(h, st, ss)]
    for ci, gi in ((3, 4), (6, 7)):
        h = conv(h, THERMAL_A_GN_RELU, ss, net[ci].weight, net[ci].bias)
        st, ss = group_norm(h, net[gi])
        tape += [(h, st, ss)]
    conv(h, THERMAL_A_GN_RELU, ss, net[9].weight, net[9].bias, out_ptr=out_t.data_ptr(), ld_out=ld_out, ends=ends,
         e_mode=THERMAL_E_STORE if ends is None else THERMAL_E_DIFFUSE)


def _simple_backward(m: "AdaptiveUNet", x: _V, ends, g: _V, tape, want_dx: bool):
    net = m.simple_net
    cin0 = int(net[0].weight.shape[1])
    grads = [None] * 14
    (h0, st0, ss0), (h1, st1, ss1), (h2, st2, ss2) = tape
    d, grads[12], grads[13] = conv_backward(h2, THERMAL_A_GN_RELU, ss2, net[9].weight, g, True, h2.c)
    d, grads[10], grads[11] = group_norm_backward(h2, net[7], st2, ss2, d)
    d, grads[8], grads[9] = conv_backward(h1, THERMAL_A_GN_RELU, ss1, net[6].weight, d, True, h1.c)
    d, grads[6], grads[7] = group_norm_backward(h1, net[4], st1, ss1, d)
    d, grads[4], grads[5] = conv_backward(h0, THERMAL_A_GN_RELU, ss0, net[3].weight, d, True, h0.c)
    d, grads[2], grads[3] = group_norm_backward(h0, net[1], st0, ss0, d)
    x0 = _V(x.t, x.off, x.ld, cin0, x.B, x.H, x.W)
    dx_c = cin0 if ends is None else ends.F  # the position channels take no gradient
    dx, grads[0], grads[1] = conv_backward(x0, _first_input(x, ends), None, net[0].weight, d, want_dx, dx_c, ends=ends)
    return dx, grads


def _block_forward(blk: nn.Sequential, x: _V, a_mode, ss, ends=None):
    """The two (Conv, GroupNorm, ReLU) stages of a contract / expand block: returns ((h1, st1, ss1), (h2, st2, ss2))."""
    h1 = conv(x, a_mode, ss, blk[0].weight, blk[0].bias, ends=ends)
    st1, s1 = group_norm(h1, blk[1])
    h2 = conv(h1, THERMAL_A_GN_RELU, s1, blk[3].weight, blk[3].bias)
    st2, s2 = group_norm(h2, blk[4])
    return (h1, st1, s1), (h2, st2, s2)


def _block_backward(blk: nn.Sequential, x: _V, a_mode, ss, rec, d: _V, want_dx: bool, dx_c: int, ends=None):
    """Reverse of _block_forward: ``d`` = gradient of relu(GroupNorm(h2)); returns (dx, [grads of blk 0, 1, 3, 4 w / b])."""
    (h1, st1, s1), (h2, st2, s2) = rec
    g = [None] * 8
    d, g[6], g[7] = group_norm_backward(h2, blk[4], st2, s2, d)
    d, g[4], g[5] = conv_backward(h1, THERMAL_A_GN_RELU, s1, blk[3].weight, d, True, h1.c)
    d, g[2], g[3] = group_norm_backward(h1, blk[1], st1, s1, d)
    dx, g[0], g[1] = conv_backward(x, a_mode, ss, blk[0].weight, d, want_dx, dx_c, ends=ends)
    return dx, g


def _unet_forward(m: "AdaptiveUNet", x: _V, ends, out_t, ld_out, tape):
    dev = x.t.device
    B, H0, W0 = x.B, x.H, x.W
    cin0 = int(m.conv1[0].weight.shape[1])
    x0 = _V(x.t, x.off, x.ld, cin0, B, H0, W0)
    c1w, c2w, c3w = (int(getattr(m, n)[0].weight.shape[0]) for n in ("conv1", "conv2", "conv3"))
    u3w, u2w, u1w = (int(getattr(m, n)[6].weight.shape[1]) for n in ("upconv3", "upconv2", "upconv1"))
    H1, W1 = _pooled(H0), _pooled(W0)
    H2, W2 = _pooled(H1), _pooled(W1)
    H3, W3 = _pooled(H2), _pooled(W2)
    # cat buffers: [up | skip] channel slices of one row buffer per level
    cat1 = torch.empty(B * H1 * W1, u2w + c1w, dtype=torch.float32, device=dev)
    cat2 = torch.empty(B * H2 * W2, u3w + c2w, dtype=torch.float32, device=dev)
    c1 = _V(cat1, u2w, u2w + c1w, c1w, B, H1, W1)
    c2 = _V(cat2, u3w, u3w + c2w, c2w, B, H2, W2)
    c3 = _new(B, H3, W3, c3w, dev)
    r1 = _block_forward(m.conv1, x0, _first_input(x, ends), None, ends=ends)
    i1 = max_pool(r1[1][0], r1[1][2], c1)
    r2 = _block_forward(m.conv2, c1, THERMAL_A_PLAIN, None)
    i2 = max_pool(r2[1][0], r2[1][2], c2)
    r3 = _block_forward(m.conv3, c2, THERMAL_A_PLAIN, None)
    i3 = max_pool(r3[1][0], r3[1][2], c3)
    ups = []
    for name, inp, tgt, width in (("upconv3", c3, (cat2, H2, W2), u3w), ("upconv2", _V(cat2, 0, cat2.shape[1], cat2.shape[1], B, H2, W2),
                                                                        (cat1, H1, W1), u2w)):
        blk = getattr(m, name)
        rec = _block_forward(blk, inp, THERMAL_A_PLAIN, None)
        h2 = rec[1]
        t_buf, th, tw = tgt
        if (2 * inp.H, 2 * inp.W) == (th, tw):
            conv_transpose(h2[0], h2[2], blk[6].weight, blk[6].bias, t_buf.data_ptr(), int(t_buf.shape[1]))
            up = None
        else:
            up = _new(B, 2 * inp.H, 2 * inp.W, width, dev)
            conv_transpose(h2[0], h2[2], blk[6].weight, blk[6].bias, up.ptr, up.ld)
            resize(up, _V(t_buf, 0, int(t_buf.shape[1]), width, B, th, tw))
        ups.append((inp, rec, up))
    inp1 = _V(cat1, 0, cat1.shape[1], cat1.shape[1], B, H1, W1)
    rec1 = _block_forward(m.upconv1, inp1, THERMAL_A_PLAIN, None)
    h2 = rec1[1]
    blk = m.upconv1
    if (2 * H1, 2 * W1) == (H0, W0):
        conv_transpose(h2[0], h2[2], blk[6].weight, blk[6].bias, out_t.data_ptr(), ld_out, ends=ends,
                       e_mode=THERMAL_E_STORE if ends is None else THERMAL_E_DIFFUSE)
        up1 = None
    else:
        up1 = _new(B, 2 * H1, 2 * W1, u1w, dev)
        conv_transpose(h2[0], h2[2], blk[6].weight, blk[6].bias, up1.ptr, up1.ld)
        if ends is None:
            resize(up1, _V(out_t, 0, ld_out, u1w, B, H0, W0))
        else:
            eh = _new(B, H0, W0, u1w, dev)
            resize(up1, eh)
            rows_op(THERMAL_ROWS_FINALIZE, eh.rows, ends.F, ends.sa, ends.s1, ends.x.data_ptr(), ends.ld, ends.eps.data_ptr(), ends.F,
                    eh.ptr, eh.ld, out_t.data_ptr(), ld_out, out_t)
    ups.append((inp1, rec1, up1))
    tape += [x0, (r1, i1, c1), (r2, i2, c2), (r3, i3, c3), ups]


def _unet_backward(m: "AdaptiveUNet", x: _V, ends, g: _V, tape, want_dx: bool):
    x0, (r1, i1, c1), (r2, i2, c2), (r3, i3, c3), ups = tape
    B, H0, W0 = x0.B, x0.H, x0.W
    grads = {}

    def put(name, gl, gt=None):
        blk = [name + s for s in (".0.w", ".0.b", ".1.w", ".1.b", ".3.w", ".3.b", ".4.w", ".4.b")]
        grads.update(zip(blk, gl))
        if gt is not None:
            grads[name + ".6.w"], grads[name + ".6.b"] = gt

    # upconv1: convT (+ resize) to the original size
    inp1, rec1, up1 = ups[2]
    blk = m.upconv1
    h2 = rec1[1]
    if up1 is not None:
        g = resize_backward(up1, g)
    d, dwt, dbt = conv_transpose_backward(h2[0], h2[2], blk[6].weight, g)
    dcat1, gl = _block_backward(blk, inp1, THERMAL_A_PLAIN, None, rec1, d, True, inp1.c)
    put("upconv1", gl, (dwt, dbt))
    u2w = inp1.c - c1.c
    # upconv2: its output went to dcat1[:, :u2w]
    inp2, rec2, up2 = ups[1]
    blk = m.upconv2
    gup = _V(dcat1.t, 0, dcat1.ld, u2w, B, c1.H, c1.W)
    if up2 is not None:
        gup = resize_backward(up2, gup)
    d, dwt, dbt = conv_transpose_backward(rec2[1][0], rec2[1][2], blk[6].weight, gup)
    dcat2, gl = _block_backward(blk, inp2, THERMAL_A_PLAIN, None, rec2, d, True, inp2.c)
    put("upconv2", gl, (dwt, dbt))
    u3w = inp2.c - c2.c
    inp3, rec3, up3 = ups[0]
    blk = m.upconv3
    gup = _V(dcat2.t, 0, dcat2.ld, u3w, B, c2.H, c2.W)
    if up3 is not None:
        gup = resize_backward(up3, gup)
    d, dwt, dbt = conv_transpose_backward(rec3[1][0], rec3[1][2], blk[6].weight, gup)
    dc3, gl = _block_backward(blk, inp3, THERMAL_A_PLAIN, None, rec3, d, True, inp3.c)
    put("upconv3", gl, (dwt, dbt))
    # contract path: pooled outputs take the gradient of the next block and of their cat slice
    d = max_pool_backward(r3[1][0], i3, dc3, None)
    dc2, gl = _block_backward(m.conv3, c2, THERMAL_A_PLAIN, None, r3, d, True, c2.c)
    put("conv3", gl)
    d = max_pool_backward(r2[1][0], i2, dc2, _V(dcat2.t, u3w, dcat2.ld, c2.c, B, c2.H, c2.W))
    dc1, gl = _block_backward(m.conv2, c1, THERMAL_A_PLAIN, None, r2, d, True, c1.c)
    put("conv2", gl)
    d = max_pool_backward(r1[1][0], i1, dc1, _V(dcat1.t, u2w, dcat1.ld, c1.c, B, c1.H, c1.W))
    dx_c = x0.c if ends is None else ends.F
    dx, gl = _block_backward(m.conv1, x0, _first_input(x, ends), None, r1, d, want_dx, dx_c, ends=ends)
    put("conv1", gl)
    out = []
    for name in _UNET_BLOCKS:
        for i in _layers(name):
            out += [grads["%s.%d.w" % (name, i)], grads["%s.%d.b" % (name, i)]]
    return dx, out


def _use_simple(H: int, W: int) -> bool:
    return min(H, W) <= 4


class _ScoreFunction(torch.autograd.Function):
    """rows out = score model (or the whole diffusion step when ``eps`` is given) of the image batch in ``x`` rows.
    spec = (model, B, H, W, F or None, sa, s1); params = the running branch's parameters (others get no gradient)."""

    @staticmethod
    def forward(ctx, x, eps, spec, *params):
        m, B, H, W, F, sa, s1 = spec
        dev = x.device
        ld = int(x.stride(0))
        xv = _V(x, 0, ld, int(x.shape[1]), B, H, W)
        ends = None if eps is None else _Ends(x, ld, eps, sa, s1, F)
        cout = int(m.out_channels)
        out = torch.empty(B * H * W, cout, dtype=torch.float32, device=dev)
        tape = []
        with on_device_of(x):
            (_simple_forward if _use_simple(H, W) else _unet_forward)(m, xv, ends, out, cout, tape)
        ctx.spec, ctx.tape, ctx.ends = spec, tape, ends
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        m, B, H, W, F, sa, s1 = ctx.spec
        ends = ctx.ends
        xv = _V(x, 0, int(x.stride(0)), int(x.shape[1]), B, H, W)
        want_dx = ctx.needs_input_grad[0]
        cout = int(m.out_channels)
        if not (gout.stride(-1) == 1 and gout.stride(0) >= cout):
            gout = gout.contiguous()
        with on_device_of(x):
            if ends is not None:  # d pred / d eps_hat = -s1 / sa
                ge = torch.empty(B * H * W, cout, dtype=torch.float32, device=x.device)
                rows_op(THERMAL_ROWS_SCALE, B * H * W, cout, float(-s1 / sa), 0.0, gout.data_ptr(), int(gout.stride(0)), None, 0,
                        None, 0, ge.data_ptr(), cout, ge)
                g = _V(ge, 0, cout, cout, B, H, W)
            else:
                g = _V(gout, 0, int(gout.stride(0)), cout, B, H, W)
            fn = _simple_backward if _use_simple(H, W) else _unet_backward
            dnet, grads = fn(m, xv, ends, g, ctx.tape, want_dx)
            dx = None
            if want_dx:
                if ends is None:
                    dx = dnet.t
                else:  # d pred / d x = 1 + sa * (d eps_hat / d noisy)^T ... through the net
                    dx = torch.empty(B * H * W, F, dtype=torch.float32, device=x.device)
                    rows_op(THERMAL_ROWS_AXPY, B * H * W, F, float(sa), 0.0, gout.data_ptr(), int(gout.stride(0)), dnet.ptr, dnet.ld,
                            None, 0, dx.data_ptr(), F, dx)
        ctx.tape = None
        return (dx, None, None) + tuple(grads)


def _check_rows(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise RuntimeError("graph_weather_amd: %s must be on a HIP device - there is no CPU path" % what)
    if x.dtype != torch.float32:
        raise RuntimeError("graph_weather_amd: %s must be float32 (the thermalizer runs in fp32)" % what)


def _rows(x: torch.Tensor) -> torch.Tensor:
    return x if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


class AdaptiveUNet(nn.Module):
    """thermalizer.py AdaptiveUNet: ``simple_net`` when min(H, W) <= 4, else the three-level UNet."""

    def __init__(self, in_channels: int, out_channels: int) -> None:
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.conv1 = self._contract_block(in_channels, 32, 7, 3)
        self.conv2 = self._contract_block(32, 64, 3, 1)
        self.conv3 = self._contract_block(64, 128, 3, 1)
        self.upconv3 = self._expand_block(128, 64, 3, 1)
        self.upconv2 = self._expand_block(64 * 2, 32, 3, 1)
        self.upconv1 = self._expand_block(32 * 2, out_channels, 3, 1)
        self.simple_net = nn.Sequential(
            nn.Conv2d(in_channels, 64, 3, padding=1), nn.GroupNorm(8, 64), nn.ReLU(),
            nn.Conv2d(64, 128, 3, padding=1), nn.GroupNorm(8, 128), nn.ReLU(),
            nn.Conv2d(128, 64, 3, padding=1), nn.GroupNorm(8, 64), nn.ReLU(),
            nn.Conv2d(64, out_channels, 3, padding=1),
        )

    def params_for(self, H: int, W: int) -> List[torch.Tensor]:
        return _simple_params(self.simple_net) if _use_simple(H, W) else _unet_params(self)

    def forward_rows(self, x: torch.Tensor, B: int, H: int, W: int, eps: Optional[torch.Tensor] = None, sa: float = 1.0,
                     s1: float = 0.0) -> torch.Tensor:
        """NHWC rows [B * H * W, C] in -> rows out.  With ``eps`` the whole diffusion step: x holds the clean F-channel rows
        (any row stride), the output is (noisy - s1 * eps_hat) / sa."""
        _check_rows(x, "x")
        x = _rows(x)
        F = int(x.shape[1]) if eps is not None else None
        spec = (self, int(B), int(H), int(W), F, float(sa), float(s1))
        return _ScoreFunction.apply(x, eps, spec, *self.params_for(H, W))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """NCHW [B, C, H, W] like the reference (converted to rows inside)."""
        if x.dim() != 4:
            raise ValueError("AdaptiveUNet expects [B, C, H, W], got %s" % (tuple(x.shape),))
        B, C, H, W = (int(s) for s in x.shape)
        if C != self.in_channels:
            raise RuntimeError("AdaptiveUNet: expected %d input channels, got %d" % (self.in_channels, C))
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
        y = self.forward_rows(rows, B, H, W)
        return y.reshape(B, H, W, self.out_channels).permute(0, 3, 1, 2)

    def _contract_block(self, in_channels, out_channels, kernel_size, padding):
        return nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding),
            nn.GroupNorm(min(8, out_channels), out_channels), nn.ReLU(),
            nn.Conv2d(out_channels, out_channels, kernel_size=kernel_size, padding=padding),
            nn.GroupNorm(min(8, out_channels), out_channels), nn.ReLU(),
            nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
        )

    def _expand_block(self, in_channels, out_channels, kernel_size, padding):
        return nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding),
            nn.GroupNorm(min(8, out_channels), out_channels), nn.ReLU(),
            nn.Conv2d(out_channels, out_channels, kernel_size, padding=padding),
            nn.GroupNorm(min(8, out_channels), out_channels), nn.ReLU(),
            nn.ConvTranspose2d(out_channels, out_channels, kernel_size=3, stride=2, padding=1, output_padding=1),
        )


def timestep(t, timesteps: int) -> int:
    """thermalizer.py: ``t`` an int or a tensor (``.long()``), clamped to [0, timesteps - 1]; anything else: TypeError."""
    if isinstance(t, int):
        v = int(t)
    elif isinstance(t, torch.Tensor):
        if t.numel() != 1:
            raise ValueError("graph_weather_amd: the thermalizer takes one timestep for the whole call, got %d" % t.numel())
        v = int(t.detach().reshape(-1)[0].long().item())
    else:
        raise TypeError("Timestep t must be int or torch.Tensor")
    return min(max(v, 0), timesteps - 1)


class ThermalizerLayer(nn.Module):
    """thermalizer.py ThermalizerLayer: one denoising step of the rows ``x`` [batch * H * W, F] at timestep ``t``."""

    def __init__(self, input_dim: int = 256, timesteps: int = 1000) -> None:
        super().__init__()
        self.score_model = AdaptiveUNet(input_dim + 2, input_dim)  # +2 for the (x, y) position channels
        self.timesteps = timesteps
        self.betas = self._cosine_beta_schedule(timesteps)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, axis=0)
        self.last_noise: Optional[torch.Tensor] = None

    def coefficients(self, t: int) -> Tuple[float, float]:
        """(sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t)), computed in fp64."""
        ac = float(self.alphas_cumprod[t])
        return math.sqrt(ac), math.sqrt(1.0 - ac)

    def forward(self, x: torch.Tensor, t, height: int = None, width: int = None, batch: int = None,
                noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """thermalizer.py forward on rows [batch * height * width, F] (read in place through their row stride).  ``noise``
        (rows [rows, F]) replaces the fresh draw."""
        total_nodes, features = x.shape
        if batch is None:
            batch = 1
            nodes = total_nodes
        else:
            nodes = total_nodes // batch
        if height is None or width is None:
            warnings.warn(
                """ThermalizerLayer assumes nodes are on a regular 2D grid when
                   inferring shape from node count.
                   For irregular graphs or non-uniform layouts, pass (height, width) explicitly.""",
                UserWarning,
            )
            height, width = self._infer_grid_dimensions(nodes)
        nodes = height * width
        if batch * nodes != total_nodes:
            raise ValueError(
                f"Dimension mismatch: batch({batch}) * height({height}) * "
                f"width({width}) = {batch * nodes} != total_nodes({total_nodes})"
            )
        t = timestep(t, self.timesteps)
        if self.score_model.in_channels != features + 2:
            raise RuntimeError("ThermalizerLayer(input_dim=%d) got rows of %d features" % (self.score_model.in_channels - 2, features))
        _check_rows(x, "x")
        x = _rows(x)
        if noise is None:
            noise = torch.randn(total_nodes, features, dtype=torch.float32, device=x.device)
        elif tuple(noise.shape) != (total_nodes, features) or noise.dtype != torch.float32 or noise.device != x.device:
            raise ValueError("noise must be float32 rows [%d, %d] on %s" % (total_nodes, features, x.device))
        noise = noise.detach().contiguous()
        self.last_noise = noise
        sa, s1 = self.coefficients(t)
        return self.score_model.forward_rows(x, batch, height, width, eps=noise, sa=sa, s1=s1)

    def _cosine_beta_schedule(self, timesteps: int, s: float = 0.008) -> torch.Tensor:
        """Cosine schedule (https://openreview.net/forum?id=-NEXDKk8gZ), float64, clipped to [0, 0.999]."""
        steps = timesteps + 1
        x = torch.linspace(0, timesteps, steps, dtype=torch.float64)
        alphas_cumprod = torch.cos(((x / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2
        alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
        betas = 1 - (alphas_cumprod[1:] / alphas_cumprod[:-1])
        return torch.clip(betas, 0, 0.999)

    def _infer_grid_dimensions(self, total_nodes: int) -> Tuple[int, int]:
        return infer_grid_dimensions(total_nodes)

    def _get_position_encoding(self, H: int, W: int, B: int, device) -> torch.Tensor:
        """[B, 2, H, W] (x, y) in [0, 1] - the channels the first convolution's load generates (kept for API parity)."""
        y = torch.linspace(0, 1, steps=H, device=device).view(1, H, 1).expand(1, H, W)
        x = torch.linspace(0, 1, steps=W, device=device).view(1, 1, W).expand(1, H, W)
        return torch.stack([x, y], dim=1).expand(B, 2, H, W)


def infer_grid_dimensions(total_nodes: int) -> Tuple[int, int]:
    """thermalizer.py _infer_grid_dimensions: a near-square factorisation for N <= 16, else the divisor h in
    [sqrt(N) - 5, sqrt(N) + 5] with the smallest |h - w| (first on a tie), else (1, N)."""
    if total_nodes <= 16:
        sqrt_nodes = int(math.sqrt(total_nodes))
        if sqrt_nodes * sqrt_nodes == total_nodes:
            return sqrt_nodes, sqrt_nodes
        for h in range(1, total_nodes + 1):
            if total_nodes % h == 0:
                w = total_nodes // h
                if abs(h - w) <= 2:
                    return h, w
        return 1, total_nodes
    sqrt_nodes = int(math.sqrt(total_nodes))
    best_diff = float("inf")
    best_h, best_w = 1, total_nodes
    for h in range(max(1, sqrt_nodes - 5), sqrt_nodes + 6):
        if total_nodes % h == 0:
            w = total_nodes // h
            diff = abs(h - w)
            if diff < best_diff:
                best_diff = diff
                best_h, best_w = h, w
    return best_h, best_w
