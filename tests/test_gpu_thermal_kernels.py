"""The kernels of graph_weather_amd/csrc/gw_thermal.hip one by one, through the wrappers of graph_weather_amd/thermalizer.py,
against the float64 per-operation references of tests/thermal_oracle.py (tied to ``score`` / ``thermalize`` by
tests/test_thermalizer_host.py).

Idioms (those of tests/test_gpu_cafa.py): wherever a wrapper takes a pointer and a row stride the operand is a channel slice of a
wider NaN-filled allocation; after the call the padding is still NaN and the written extent is finite; every case runs twice and
the two results are ``torch.equal`` (the file uses no float atomics).

Bars.  A pure selection or copy is compared bitwise.  For everything else the yardstick is the float32 CPU evaluation of the same
reference on the same inputs against its float64 evaluation; a kernel may err at most 4 x that yardstick (the margin
``_check_gradient`` of test_gpu_cafa.py gives MFMA summation order), with a floor of 1e-6 of the reference's maximum.  Every
figure is printed before it is asserted ("ratio" = error / max(yardstick, a quarter of the floor), so the bar is ratio 4).

Two checks have another floor, the input gradient (conv_nt_kernel<PLAIN, STORE> with flipped taps) and the bias gradient (colsum)
of test_conv_backward: max(1e-6, 2^-24 sqrt(K)) of the reference's maximum, K the number of terms an output element sums
(taps x cout, and pixels).  With the fixed 1e-6 they fail on an MI355X, the first at 4.03 x its yardstick and 1.02e-6 of the
maximum (3 x 3 taps, 130 channels: K = 1170), the second at 4.17 x and 1.32e-6 (one column of 1000 pixels whose sum cancels to
4.1 where sqrt(1000) = 32 is typical).  Both are plain float32 sums: K roundings of relative size u = 2^-24 add up like a random
walk to about sqrt(K) u of the sum's scale (Higham & Mary, "A new approach to probabilistic rounding error analysis", 2019), so
above K = 281 a fixed 1e-6 asks for more than the number format gives.  The float32 yardstick does not stand in for it there:
torch's CPU sum is pairwise and its GEMM keeps several accumulators, so their error grows like log K, while colsum adds 64 rows
per wave in turn and the MFMA chain adds K / 4 steps into one accumulator.  K comes from the case, never from a result; the
largest such floor is 4.8e-6 (K = 6370), and a dropped tap or slab tail is an error of the order of 1 / sqrt(K) of the maximum,
thousands of times that.  Every other check of the module, the other sums included, keeps the fixed floor: they meet it.

Reach.  Every conv_nt_kernel / conv_tn_kernel instantiation and every rows_kernel mode is compared by value:

    conv_nt_kernel<PLAIN, STORE>        test_conv_forward[plain-store-*], input gradients of test_conv_backward / test_conv_transpose
    conv_nt_kernel<PLAIN, DIFFUSE>      test_conv_forward[plain-diffuse-*]
    conv_nt_kernel<GN_RELU, STORE>      test_conv_forward[gn_relu-store-*], test_conv_transpose
    conv_nt_kernel<GN_RELU, DIFFUSE>    test_conv_forward[gn_relu-diffuse-*], test_conv_transpose[2-7-5-17-33]
    conv_nt_kernel<DIFFUSE, STORE>      test_conv_forward[diffuse-store-*]
    conv_nt_kernel<DIFFUSE, DIFFUSE>    test_conv_forward[diffuse-diffuse-*]
    conv_tn_kernel<PLAIN>               test_conv_backward[plain-*]
    conv_tn_kernel<GN_RELU>             test_conv_backward[gn_relu-*], test_conv_transpose
    conv_tn_kernel<DIFFUSE>             test_conv_backward[diffuse-*]
    rows_kernel FINALIZE / SCALE / AXPY test_rows_op[finalize-*] / [scale-*] / [axpy-*]

Preconditions checked on the float64 reference alone, before any kernel result is looked at: no GroupNorm pre-activation of
test_group_norm_backward has |z| < 1e-5 (the ReLU mask is a sign test), and in test_max_pool_general at most 1 % of the windows
of a case have their top two values closer than 1e-5 of the maximum (only there the indices are not compared).

Measured on an MI355X (1870 comparisons), worst ratio per kernel under the bars above, with its case; the bar is 4.  The cases
added since that run have no figure here: the (2, 5, 7) shape of test_conv_backward and test_group_norm_backward_mask_at_zero.

    conv_nt<plain,store>                2.0  (k3 1x9x15 70->130)      conv_tn<plain> dw               1.7  (k7 1x5x13 70->130)
    conv_nt<plain,diffuse>              3.0  (k3 1x9x15 70->130)      conv_tn<gn_relu> dw             1.1  (k1 1x5x13 5->30)
    conv_nt<gn_relu,store>              1.8  (k3 1x9x15 70->130)      conv_tn<diffuse> dw             1.4  (k1 1x5x13 5->30)
    conv_nt<gn_relu,diffuse>            1.3  (k3 1x9x15 70->130)      conv_tn<gn_relu> transpose dw   1.0  (2x7x5 8->8)
    conv_nt<diffuse,store>              1.9  (k3 1x9x15 34->65)       colsum db, test_conv_backward   3.6  (k3 1x5x13 1->1)
    conv_nt<diffuse,diffuse>            1.4  (k3 1x9x15 34->32)       colsum (test_colsum)            2.0  (255x1)
    conv_nt<plain,store> dx             2.6  (k3 1x25x40 17->65)      gn_stats mean / rstd            0.9 / 1.8  (1x9x1024/8, mean 1e3)
    conv_nt<gn_relu,store> transpose    1.6  (2x7x5 64->32)           gn_stats scale / shift          1.8 / 1.9  (1x9x1024/8, mean 1e3)
    conv_nt<gn_relu,diffuse> transpose  0.5  (2x7x5 17->33)           gn_bwd dx / dgamma / dbeta      0.6 / 0.8 / 0.9
    conv_nt<plain,store> transpose dx   1.6  (1x3x2 64->32)           maxpool_fwd (general)           0.1  (1x5x5x64)
    resize_fwd / resize_bwd             1.1 / 1.0  (4x6->3x5)         resize adjoint identity         0.2  (2x2->1x1)
    rows_kernel finalize / scale / axpy 0.7 / 0.4 / 0.4

Both preconditions held for the committed seeds: the smallest |pre-activation| of test_group_norm_backward is 2.6e-5 (case
2x515x128/8), and no window of test_max_pool_general is a near-tie (0 % in every case).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from graph_weather_amd import _lib
from graph_weather_amd import thermalizer as th
from graph_weather_amd._lib import (THERMAL_A_DIFFUSE, THERMAL_A_GN_RELU, THERMAL_A_PLAIN, THERMAL_E_DIFFUSE, THERMAL_E_STORE,
                                    THERMAL_ROWS_AXPY, THERMAL_ROWS_FINALIZE, THERMAL_ROWS_SCALE)

from . import thermal_oracle as to

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
A_MODES = {"plain": THERMAL_A_PLAIN, "gn_relu": THERMAL_A_GN_RELU, "diffuse": THERMAL_A_DIFFUSE}
E_MODES = {"store": THERMAL_E_STORE, "diffuse": THERMAL_E_DIFFUSE}
TIMES = (0, 500, 999)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------


def _gen(*key) -> torch.Generator:
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _wide(data: torch.Tensor, off: int, right: int) -> torch.Tensor:
    """``data`` [rows, c] as columns [off, off + c) of a NaN-filled [rows, off + c + right] device buffer."""
    rows, c = data.shape
    buf = torch.full((rows, off + c + right), NAN, dtype=torch.float32, device=DEV)
    buf[:, off:off + c] = data.to(DEV)
    return buf


def _blank(rows: int, c: int, off: int, right: int) -> torch.Tensor:
    return torch.full((rows, off + c + right), NAN, dtype=torch.float32, device=DEV)


def _v(buf: torch.Tensor, off: int, c: int, B: int, H: int, W: int) -> th._V:
    assert buf.shape[0] == B * H * W
    return th._V(buf, off, int(buf.shape[1]), c, B, H, W)


def _extent(buf: torch.Tensor, off: int, c: int, allow_nan: bool = False) -> torch.Tensor:
    """The written slice, after asserting that the padding is still NaN and (unless told otherwise) the slice finite."""
    torch.cuda.synchronize()
    assert torch.isnan(buf[:, :off]).all() and torch.isnan(buf[:, off + c:]).all(), "padding overwritten"
    got = buf[:, off:off + c].clone()
    if not allow_nan:
        assert torch.isfinite(got).all(), "%d of %d elements of the extent not written" % (int((~torch.isfinite(got)).sum()), got.numel())
    return got


def _twice(run):
    """run() -> tuple of device tensors; called twice, the results must be bitwise equal.  Returns the first."""
    first = run()
    second = run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    return first


U32 = 2.0 ** -24  # unit roundoff of float32


def _figures(kernel, what, got, ref64, yard32, depth=1):
    """``depth``: the number of terms every output element sums, given only by the two checks the module docstring names."""
    ref64 = ref64.detach()
    got64 = got.detach().cpu().double().reshape(ref64.shape)
    scale = ref64.abs().max().item() if ref64.numel() else 0.0
    yard = (yard32.detach().double().reshape(ref64.shape) - ref64).abs().max().item()
    err = (got64 - ref64).abs().max().item()
    floor = max(1e-6, U32 * math.sqrt(depth)) * scale
    bar = max(4.0 * yard, floor)
    ratio = err / max(yard, floor / 4.0) if max(yard, floor) > 0 else (0.0 if err == 0 else math.inf)
    print("thermal[%s] %s: error %.3e, yardstick %.3e, bar %.3e (maximum %.3e), ratio %.2f" % (kernel, what, err, yard, bar, scale, ratio))
    return err, bar


def _check(kernel, what, got, ref64, yard32, failures=None, depth=1):
    err, bar = _figures(kernel, what, got, ref64, yard32, depth)
    if failures is None:
        assert err <= bar, (kernel, what, err, bar)
    elif not err <= bar:
        failures.append((kernel, what, err, bar))


def _affine(g, B, C):
    """Per-(sample, channel) scale and shift of either sign; every fifth channel (from 2 on) is dead: x * scale + shift < 0 for
    every |x| < 90."""
    sign = torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
    scale = sign * (0.5 + torch.rand(B, C, generator=g))
    shift = 0.3 * torch.randn(B, C, generator=g)
    dead = torch.arange(C) % 5 == 2
    scale[:, dead] = 0.1
    shift[:, dead] = -10.0
    return scale, shift


def _operand(a_mode, x, ss, eps, sa, s1, B, H, W):
    if a_mode == THERMAL_A_PLAIN:
        return x
    if a_mode == THERMAL_A_GN_RELU:
        return to.affine_relu_rows(x, ss[0], ss[1], B)
    return to.diffuse_rows(x, eps, sa, s1, B, H, W)


def _cast(dt, *ts):
    return tuple(None if t is None else t.detach().clone().to(dt) for t in ts)


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV).contiguous() for t in ts)


# ---------------------------------------------------------------------------------------------------------------------
# conv_nt_kernel: Conv2d forward, all six (operand, epilogue) pairs
# ---------------------------------------------------------------------------------------------------------------------
# M = 1, 5, 105 (a batch boundary inside a 64-pixel tile), 128, 135, 12; images with H or W < k // 2 + 1 drop live taps
CONV_SHAPES = [(1, 1, 1), (1, 1, 5), (3, 5, 7), (2, 8, 8), (1, 9, 15), (2, 3, 2)]
CONV_CHANNELS = [(1, 1), (5, 30), (16, 64), (17, 65), (70, 130)]
DIFFUSE_F = {1: 1, 3: 30, 32: 65}  # features -> cout of the A_DIFFUSE cases with a plain store


def _conv_channels(a_mode, e_mode):
    """(cin, cout, features or None)"""
    if a_mode == THERMAL_A_DIFFUSE:
        return [(f + 2, f if e_mode == THERMAL_E_DIFFUSE else co, f) for f, co in DIFFUSE_F.items()]
    return [(ci, co, co if e_mode == THERMAL_E_DIFFUSE else None) for ci, co in CONV_CHANNELS]


def _conv_inputs(key, a_mode, e_mode, k, B, H, W, cin, cout, feat):
    g = _gen(*key)
    M = B * H * W
    stored = feat if a_mode == THERMAL_A_DIFFUSE else cin
    d = {"x": torch.randn(M, stored, generator=g), "w": torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k),
         "b": 0.1 * torch.randn(cout, generator=g), "ss": None, "eps": None, "xc": None}
    if a_mode == THERMAL_A_GN_RELU:
        d["ss"] = _affine(g, B, cin)
    if feat is not None:
        d["eps"] = torch.randn(M, feat, generator=g)
    if e_mode == THERMAL_E_DIFFUSE:
        d["xc"] = torch.randn(M, feat, generator=g)
    return d


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("e_name", list(E_MODES))
@pytest.mark.parametrize("a_name", list(A_MODES))
def test_conv_forward(a_name, e_name, k):
    a_mode, e_mode = A_MODES[a_name], E_MODES[e_name]
    diffusing = a_mode == THERMAL_A_DIFFUSE or e_mode == THERMAL_E_DIFFUSE
    failures = []
    for si, (B, H, W) in enumerate(CONV_SHAPES):
        for cin, cout, feat in _conv_channels(a_mode, e_mode):
            for t in (TIMES if diffusing else (500,)):
                what = "k%d %dx%dx%d %d->%d t%d" % (k, B, H, W, cin, cout, t)
                d = _conv_inputs((1, a_mode, e_mode, k, si, cin, cout, t), a_mode, e_mode, k, B, H, W, cin, cout, feat)
                sa, s1 = to.coefficients(t)

                def ref(dt):
                    x, w, b, eps, xc = _cast(dt, d["x"], d["w"], d["b"], d["eps"], d["xc"])
                    ss = None if d["ss"] is None else _cast(dt, *d["ss"])
                    v = to.conv_rows(_operand(a_mode, x, ss, eps, sa, s1, B, H, W), w, b, B, H, W)
                    return to.rows_finalize(xc, eps, v, sa, s1) if e_mode == THERMAL_E_DIFFUSE else v

                M = B * H * W
                xbuf = _wide(d["x"], 3, 2)
                inp = _v(xbuf, 3, d["x"].shape[1], B, H, W)
                w, b, eps = _dev(d["w"], d["b"], d["eps"])
                ss = None if d["ss"] is None else _dev(d["ss"][0].reshape(-1), d["ss"][1].reshape(-1))
                ends = None
                if feat is not None:
                    if d["xc"] is not None:
                        cbuf = _wide(d["xc"], 1, 4)  # the clean rows of the epilogue: ld_x > F
                        ends = th._Ends(cbuf[:, 1:1 + feat], int(cbuf.shape[1]), eps, sa, s1, feat)
                    else:
                        ends = th._Ends(xbuf[:, 3:3 + feat], int(xbuf.shape[1]), eps, sa, s1, feat)

                def run():
                    obuf = _blank(M, cout, 2, 3)
                    th.conv(inp, a_mode, ss, w, b, _v(obuf, 2, cout, B, H, W), ends=ends, e_mode=e_mode)
                    return (_extent(obuf, 2, cout),)

                (got,) = _twice(run)
                assert torch.isnan(xbuf[:, :3]).all() and torch.isnan(xbuf[:, -2:]).all()
                _check("conv_nt<%s,%s>" % (a_name, e_name), what, got, ref(torch.float64), ref(torch.float32), failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# conv_tn_kernel + wgrad_reduce_kernel + colsum + conv_nt_kernel<PLAIN, STORE> with flipped taps: Conv2d backward
# ---------------------------------------------------------------------------------------------------------------------
# M = 1, 64, 65 and 1000 (25 x 40: with few tiles split_of cuts 16 slabs of 64 pixels, the last ragged and cut mid-row), and
# M = 70 in two samples, so that the per-(sample, channel) scale of conv_tn_kernel<GN_RELU> is indexed with b > 0
BWD_SHAPES = [(1, 1, 1), (1, 8, 8), (1, 5, 13), (1, 25, 40), (2, 5, 7)]


def _live_mask(k, H, W):
    """[k, k] True where the tap reaches a pixel of the image for some output pixel."""
    ly = torch.tensor([abs(t - k // 2) <= H - 1 for t in range(k)])
    lx = torch.tensor([abs(t - k // 2) <= W - 1 for t in range(k)])
    return ly[:, None] & lx[None, :]


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("a_name", list(A_MODES))
def test_conv_backward(a_name, k):
    a_mode = A_MODES[a_name]
    failures = []
    for si, (B, H, W) in enumerate(BWD_SHAPES):
        for cin, cout, feat in _conv_channels(a_mode, THERMAL_E_STORE):
            t = TIMES[(si + cin) % 3]
            what = "k%d %dx%dx%d %d->%d t%d" % (k, B, H, W, cin, cout, t)
            d = _conv_inputs((2, a_mode, k, si, cin, cout), a_mode, THERMAL_E_STORE, k, B, H, W, cin, cout, feat)
            M = B * H * W
            gy = torch.randn(M, cout, generator=_gen(3, a_mode, k, si, cin, cout))
            sa, s1 = to.coefficients(t)
            dxc = feat if a_mode == THERMAL_A_DIFFUSE else cin  # the position channels take no gradient

            def ref(dt):
                x, w, b, eps, g = _cast(dt, d["x"], d["w"], d["b"], d["eps"], gy)
                ss = None if d["ss"] is None else _cast(dt, *d["ss"])
                a = _operand(a_mode, x, ss, eps, sa, s1, B, H, W).detach().requires_grad_()
                w.requires_grad_()
                b.requires_grad_()
                to.conv_rows(a, w, b, B, H, W).backward(g)
                return a.grad[:, :dxc], w.grad, b.grad

            xbuf = _wide(d["x"], 3, 2)
            inp = _v(xbuf, 3, d["x"].shape[1], B, H, W)
            gbuf = _wide(gy, 1, 5)
            gv = _v(gbuf, 1, cout, B, H, W)
            w, eps = _dev(d["w"], d["eps"])
            ss = None if d["ss"] is None else _dev(d["ss"][0].reshape(-1), d["ss"][1].reshape(-1))
            ends = None if feat is None else th._Ends(xbuf[:, 3:3 + feat], int(xbuf.shape[1]), eps, sa, s1, feat)

            def run():
                dx, dw, db = th.conv_backward(inp, a_mode, ss, w, gv, True, dxc, ends=ends)
                assert dx.t.shape == (M, dxc) and dw.shape == w.shape and db.shape == (cout,)
                return dx.t, dw, db

            dx, dw, db = _twice(run)
            assert torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
            # (the wrapper zero-fills dw and hands the kernels only the live taps, so this guards the wrapper's tap list)
            dead = ~_live_mask(k, H, W)
            assert (dw.cpu()[:, :, dead] == 0).all(), "weight gradient of a tap that never hits the image"
            r64, r32 = ref(torch.float64), ref(torch.float32)
            _check("conv_nt<plain,store> dx", what, dx, r64[0], r32[0], failures, depth=k * k * cout)
            _check("conv_tn<%s> dw" % a_name, what, dw, r64[1], r32[1], failures)
            _check("colsum db", what, db, r64[2], r32[2], failures, depth=M)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# ConvTranspose2d(3, 2, 1, 1) of relu(x * scale + shift): four output-parity launches, and its backward
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ci,co", [(8, 8), (17, 33), (64, 32)])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 1, 5), (1, 3, 2), (2, 7, 5)])
def test_conv_transpose(B, H, W, ci, co):
    e_mode = THERMAL_E_DIFFUSE if (B, H, W, ci, co) == (2, 7, 5, 17, 33) else THERMAL_E_STORE
    g = _gen(4, B, H, W, ci, co)
    M, Mo = B * H * W, B * 4 * H * W
    x = torch.randn(M, ci, generator=g)
    w = torch.randn(ci, co, 3, 3, generator=g) / math.sqrt(ci * 9 / 4)
    b = 0.1 * torch.randn(co, generator=g)
    sc, sh = _affine(g, B, ci)
    gy = torch.randn(Mo, co, generator=g)
    eps, xc = torch.randn(Mo, co, generator=g), torch.randn(Mo, co, generator=g)
    sa, s1 = to.coefficients(500)

    def ref(dt):
        xv, wv, bv, scv, shv, gv, ev, cv = _cast(dt, x, w, b, sc, sh, gy, eps, xc)
        a = to.affine_relu_rows(xv, scv, shv, B).detach().requires_grad_()
        wv.requires_grad_()
        bv.requires_grad_()
        y = to.conv_transpose_rows(a, wv, bv, B, H, W)
        y.backward(gv)
        out = to.rows_finalize(cv, ev, y.detach(), sa, s1) if e_mode == THERMAL_E_DIFFUSE else y.detach()
        return out, a.grad, wv.grad, bv.grad

    xbuf = _wide(x, 2, 1)
    inp = _v(xbuf, 2, ci, B, H, W)
    wd, bd, epsd = _dev(w, b, eps)
    ss = _dev(sc.reshape(-1), sh.reshape(-1))
    ends = None
    if e_mode == THERMAL_E_DIFFUSE:
        cbuf = _wide(xc, 2, 3)
        ends = th._Ends(cbuf[:, 2:2 + co], int(cbuf.shape[1]), epsd, sa, s1, co)

    def forward():
        obuf = _blank(Mo, co, 0, 7)  # the leading channel slice of a cat buffer
        th.conv_transpose(inp, ss, wd, bd, obuf.data_ptr(), int(obuf.shape[1]), ends=ends, e_mode=e_mode)
        return (_extent(obuf, 0, co),)  # NaN left in the extent = a pixel that none of the four parities wrote

    (out,) = _twice(forward)
    gbuf = _wide(gy, 4, 1)

    def backward():
        dx, dw, db = th.conv_transpose_backward(inp, ss, wd, _v(gbuf, 4, co, B, 2 * H, 2 * W))
        assert dx.t.shape == (M, ci) and dw.shape == wd.shape and db.shape == (co,)
        return dx.t, dw, db

    dx, dw, db = _twice(backward)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    what = "%dx%dx%d %d->%d" % (B, H, W, ci, co)
    failures = []
    _check("conv_nt<gn_relu,%s> transpose" % ("diffuse" if e_mode == THERMAL_E_DIFFUSE else "store"), what, out, r64[0], r32[0], failures)
    _check("conv_nt<plain,store> transpose dx", what, dx, r64[1], r32[1], failures)
    _check("conv_tn<gn_relu> transpose dw", what, dw, r64[2], r32[2], failures)
    _check("colsum db", what, db, r64[3], r32[3], failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_colsum(rows):
    failures = []
    for cols in (1, 63, 64, 65, 300):
        x = torch.randn(rows, cols, generator=_gen(5, rows, cols))
        buf = _wide(x, 3, 2)

        def run():
            out = torch.full((cols,), NAN, dtype=torch.float32, device=DEV)
            th.colsum(_v(buf, 3, cols, 1, rows, 1), out)
            return (out,)

        (got,) = _twice(run)
        assert torch.isfinite(got).all()
        _check("colsum", "%dx%d" % (rows, cols), got, to.colsum_rows(x.double()), to.colsum_rows(x), failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics and backward
# ---------------------------------------------------------------------------------------------------------------------
# (B, hw, C, G): one element per group (variance exactly 0); hw around the 256-pixel slab; groups of 1, 4, 9, 16, 128 channels
GN_CASES = [(1, 1, 8, 8), (2, 1, 64, 8), (1, 255, 32, 8), (1, 256, 32, 8), (3, 257, 64, 8), (2, 515, 128, 8), (1, 40, 3, 3),
            (1, 9, 1024, 8), (2, 70, 72, 8)]
# seeds of test_group_norm_backward, chosen on the CPU so that no float64 pre-activation has |z| < 1e-5
GN_SEEDS = {case: {(3, 257, 64, 8): 2, (2, 515, 128, 8): 3}.get(case, 0) for case in GN_CASES}


def _gn_inputs(case, offset, seed=0):
    B, hw, C, G = case
    g = _gen(6, B, hw, C, G, seed)
    x = torch.randn(B * hw, C, generator=g) + offset
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma = sign * (0.5 + torch.rand(C, generator=g))
    beta = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B * hw, C, generator=g)
    return x, gamma, beta, dy


def _gn_module(G, C, gamma, beta):
    gn = nn.GroupNorm(G, C, eps=1e-5).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    return gn


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_group_norm_forward(case, offset):
    """offset 1e3: mean 1e3, standard deviation 1 - the cancellation the Welford / Chan form exists for."""
    B, hw, C, G = case
    x, gamma, beta, _ = _gn_inputs(case, offset)
    gn = _gn_module(G, C, gamma, beta)
    buf = _wide(x, 5, 0)  # a trailing channel slice

    def run():
        st, (sc, sh) = th.group_norm(_v(buf, 5, C, B, hw, 1), gn)
        assert st.shape == (B * G * 2,) and sc.shape == (B * C,) and sh.shape == (B * C,)
        return st, sc, sh

    st, sc, sh = _twice(run)
    assert torch.isfinite(st).all() and torch.isfinite(sc).all() and torch.isfinite(sh).all()
    st = st.reshape(B, G, 2)
    if hw * (C // G) == 1:  # one element per group: the mean is a copy of x, M2 = 0 exactly, rstd = 1 / sqrt(eps)
        assert torch.equal(st[..., 0].cpu().reshape(-1), x.reshape(-1))
        want = 1.0 / np.sqrt(np.float64(np.float32(1e-5)))  # to one float32 rounding
        assert ((st[..., 1].cpu().double() - want).abs() <= float(np.spacing(np.float32(want)))).all()
    r64 = to.group_norm_stats(x.double(), gamma.double(), beta.double(), B, G)
    r32 = to.group_norm_stats(x, gamma, beta, B, G)
    what = "%dx%dx%d/%d offset %g" % (B, hw, C, G, offset)
    failures = []
    for name, got, a, b in zip(("mean", "rstd", "scale", "shift"), (st[..., 0], st[..., 1], sc, sh), r64, r32):
        _check("gn_stats %s" % name, what, got, a, b, failures)
    assert not failures, failures


def _gn_margin(case, seed):
    B, hw, C, G = case
    x, gamma, beta, _ = _gn_inputs(case, 0.0, seed)
    return to.group_norm_rows(x.double(), gamma.double(), beta.double(), B, G).abs().min().item()


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_group_norm_backward(case):
    B, hw, C, G = case
    seed = GN_SEEDS[case]
    margin = _gn_margin(case, seed)
    print("thermal[gn_bwd] %s: smallest |pre-activation| of the float64 reference %.3e" % (case, margin))
    assert margin >= 1e-5, "the seed leaves a pre-activation on the ReLU mask's edge"
    x, gamma, beta, dy = _gn_inputs(case, 0.0, seed)
    gn = _gn_module(G, C, gamma, beta)
    xbuf, dbuf = _wide(x, 5, 0), _wide(dy, 2, 3)
    xv = _v(xbuf, 5, C, B, hw, 1)
    st, ss = th.group_norm(xv, gn)

    def run():
        dx, dgamma, dbeta = th.group_norm_backward(xv, gn, st, ss, _v(dbuf, 2, C, B, hw, 1))
        assert dx.t.shape == (B * hw, C) and dgamma.shape == (C,) and dbeta.shape == (C,)
        return dx.t, dgamma, dbeta

    got = _twice(run)

    def ref(dt):
        xv_, gv, bv, dv = _cast(dt, x, gamma, beta, dy)
        for v in (xv_, gv, bv):
            v.requires_grad_()
        to.gn_relu_rows(xv_, gv, bv, B, G).backward(dv)
        return xv_.grad, gv.grad, bv.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    failures = []
    for name, o, a, b in zip(("dx", "dgamma", "dbeta"), got, r64, r32):
        assert torch.isfinite(o).all()
        _check("gn_bwd %s" % name, "%dx%dx%d/%d" % case, o, a, b, failures)
    assert not failures, failures


def test_group_norm_backward_mask_at_zero():
    """A channel with gamma = beta = 0 has the pre-activation x * 0 + 0 = 0 exactly, in the kernel as in the reference, and
    ReLU passes no gradient at 0: that channel's dgamma and dbeta are exactly 0.  (Every other pre-activation of the case keeps
    the 1e-5 margin.)"""
    case = (2, 70, 16, 4)
    B, hw, C, G = case
    x, gamma, beta, dy = _gn_inputs(case, 0.0)
    gamma[5] = 0.0
    beta[5] = 0.0
    z = to.group_norm_rows(x.double(), gamma.double(), beta.double(), B, G)
    keep = torch.arange(C) != 5
    assert (z[:, 5] == 0).all() and z[:, keep].abs().min().item() >= 1e-5
    gn = _gn_module(G, C, gamma, beta)
    xbuf, dbuf = _wide(x, 5, 0), _wide(dy, 2, 3)
    xv = _v(xbuf, 5, C, B, hw, 1)
    st, ss = th.group_norm(xv, gn)

    def run():
        dx, dgamma, dbeta = th.group_norm_backward(xv, gn, st, ss, _v(dbuf, 2, C, B, hw, 1))
        return dx.t, dgamma, dbeta

    dx, dgamma, dbeta = _twice(run)

    def ref(dt):
        xv_, gv, bv, dv = _cast(dt, x, gamma, beta, dy)
        for v in (xv_, gv, bv):
            v.requires_grad_()
        to.gn_relu_rows(xv_, gv, bv, B, G).backward(dv)
        return xv_.grad, gv.grad, bv.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert r64[1][5] == 0 and r64[2][5] == 0
    assert dgamma[5].item() == 0 and dbeta[5].item() == 0
    failures = []
    for name, o, a, b in zip(("dx", "dgamma", "dbeta"), (dx, dgamma, dbeta), r64, r32):
        _check("gn_bwd %s" % name, "2x70x16/4, a channel at exactly 0", o, a, b, failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# MaxPool2d(3, 2, 1) of relu(x * scale + shift), with indices, and its backward
# ---------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1, 3), (2, 1, 6, 5), (1, 5, 5, 64), (2, 7, 4, 70), (1, 12, 13, 32)]
POOL_IDS = ["x".join(map(str, c)) for c in POOL_CASES]
# seeds of test_max_pool_general, chosen on the CPU so that at most 1 % of a case's windows are near-ties in float64
POOL_SEEDS = {case: 0 for case in POOL_CASES}


def _pooled(n):
    return (n - 1) // 2 + 1


def _pool_gpu(x, sc, sh, B, H, W, C, allow_nan=False):
    """-> (pooled rows, indices), both from a run into a NaN-filled cat-buffer slice, run twice."""
    Mo = B * _pooled(H) * _pooled(W)
    xbuf = _wide(x, 1, 2)
    ss = _dev(sc.reshape(-1), sh.reshape(-1))

    def run():
        obuf = _blank(Mo, C, 6, 1)
        idx = th.max_pool(_v(xbuf, 1, C, B, H, W), ss, _v(obuf, 6, C, B, _pooled(H), _pooled(W)))
        assert idx.shape == (Mo, C) and idx.dtype == torch.int32
        return _extent(obuf, 6, C, allow_nan), idx

    return _twice(run)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _exact_pool_input(case):
    B, H, W, C = case
    return torch.randn(B * H * W, C, generator=_gen(7, *case))


def _distinct_nonzero(x, B, H, W):
    """Within every (sample, channel) image - so within every window - the nonzero values of relu(x) are distinct."""
    v = torch.relu(x).reshape(B, H * W, -1).sort(dim=1).values
    return bool(((v[:, 1:] != v[:, :-1]) | (v[:, 1:] == 0)).all())


@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_max_pool_exact_and_backward(case):
    """scale 1, shift 0: the kernel's fmaf is exact, so output and indices are torch's bit for bit - the all-zero windows the
    ReLU leaves included, where the first element in row-major order wins."""
    B, H, W, C = case
    x = _exact_pool_input(case)
    assert _distinct_nonzero(x, B, H, W)
    ref, ridx = to.max_pool_rows(torch.relu(x), B, H, W)
    out, idx = _pool_gpu(x, torch.ones(B, C), torch.zeros(B, C), B, H, W, C)
    assert _same_bits(out.cpu(), ref)
    assert torch.equal(idx.cpu().long(), ridx)
    # backward with these indices: every pixel sums at most four terms in window order, so float32 index_add is the bits
    Mo = ref.shape[0]
    g = _gen(8, *case)
    g1, g2 = torch.randn(Mo, C, generator=g), torch.randn(Mo, C, generator=g)
    b_of = torch.arange(Mo).div(Mo // B, rounding_mode="floor")[:, None]
    lin = ((b_of * H * W + ridx) * C + torch.arange(C)[None, :]).reshape(-1)
    xv = _v(_wide(x, 1, 2), 1, C, B, H, W)
    b1, b2 = _wide(g1, 2, 2), _wide(g2, 9, 0)
    for second in (False, True):
        want = torch.zeros(B * H * W * C).index_add_(0, lin, (g1 + g2 if second else g1).reshape(-1)).reshape(B * H * W, C)

        def run():
            g2v = _v(b2, 9, C, B, _pooled(H), _pooled(W)) if second else None
            dx = th.max_pool_backward(xv, idx, _v(b1, 2, C, B, _pooled(H), _pooled(W)), g2v)
            assert dx.t.shape == (B * H * W, C)
            return (dx.t,)

        (dx,) = _twice(run)
        assert _same_bits(dx.cpu(), want), "g2 %s" % second


@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_max_pool_plateau_and_nan(case):
    B, H, W, C = case
    ones, zeros = torch.ones(B, C), torch.zeros(B, C)
    base = torch.randn(B * H * W, C, generator=_gen(9, *case))
    nan_img = base.clone()
    nan_img[(B * H * W) // 2, C // 2] = NAN
    for name, x in (("constant", torch.full((B * H * W, C), 1.5)), ("negative", -base.abs() - 0.1), ("nan", nan_img)):
        ref, ridx = to.max_pool_rows(torch.relu(x), B, H, W)
        out, idx = _pool_gpu(x, ones, zeros, B, H, W, C, allow_nan=True)
        assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)), name
        assert bool(torch.isnan(ref).any()) == (name == "nan")
        assert _same_bits(torch.nan_to_num(out.cpu(), nan=7.0), torch.nan_to_num(ref, nan=7.0)), name
        assert torch.equal(idx.cpu().long(), ridx), name


def _general_pool_inputs(case, seed):
    B, H, W, C = case
    g = _gen(10, *case, seed)
    x = torch.randn(B * H * W, C, generator=g)
    sign = torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
    sc = sign * (0.5 + torch.rand(B, C, generator=g))
    sh = 2.0 + torch.rand(B, C, generator=g)  # most pre-activations positive: few all-zero windows
    return x, sc, sh


def _pool_near_ties(case, seed):
    """Mask [pooled rows, C] of the windows whose float64 top two values are within 1e-5 of the maximum of each other."""
    B, H, W, C = case
    x, sc, sh = _general_pool_inputs(case, seed)
    z = to.to_image(to.affine_relu_rows(x.double(), sc.double(), sh.double(), B), B, H, W)
    pad = F.pad(z, (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(pad, 3, stride=2).reshape(B, C, 9, -1)
    top = win.topk(2, dim=2).values
    near = (top[:, :, 0] - top[:, :, 1]) <= 1e-5 * z.abs().max()
    return near.permute(0, 2, 1).reshape(-1, C)


@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_max_pool_general(case):
    B, H, W, C = case
    seed = POOL_SEEDS[case]
    near = _pool_near_ties(case, seed)
    share = near.double().mean().item()
    print("thermal[maxpool] %s: %.3f %% of the windows are near-ties in float64" % (case, 100 * share))
    assert share <= 0.01
    x, sc, sh = _general_pool_inputs(case, seed)
    out, idx = _pool_gpu(x, sc, sh, B, H, W, C)
    r64, i64 = to.max_pool_rows(to.affine_relu_rows(x.double(), sc.double(), sh.double(), B), B, H, W)
    r32, _ = to.max_pool_rows(to.affine_relu_rows(x, sc, sh, B), B, H, W)
    _check("maxpool_fwd", "%dx%dx%dx%d" % case, out, r64, r32)
    assert torch.equal(idx.cpu().long()[~near], i64[~near])


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize (align_corners=False) and its backward
# ---------------------------------------------------------------------------------------------------------------------
# the UNet's own 2k -> 2k - 1 steps, then the identity, an enlargement and a reduction by more than two
RESIZE_CASES = [((2, 2), (1, 1)), ((4, 6), (3, 5)), ((14, 10), (13, 9)), ((2, 346), (1, 345)), ((5, 5), (5, 5)), ((3, 4), (7, 9)),
                ((9, 8), (4, 3))]


def _resize_gpu(x, gy, B, hi, wi, ho, wo, C):
    xbuf, gbuf = _wide(x, 2, 3), _wide(gy, 1, 1)
    xv = _v(xbuf, 2, C, B, hi, wi)

    def run():
        obuf = _blank(B * ho * wo, C, 0, 5)
        th.resize(xv, _v(obuf, 0, C, B, ho, wo))
        dx = th.resize_backward(xv, _v(gbuf, 1, C, B, ho, wo))
        assert dx.t.shape == (B * hi * wi, C)
        return _extent(obuf, 0, C), dx.t

    return _twice(run)


@pytest.mark.parametrize("C", [1, 70])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("sizes", RESIZE_CASES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_resize(sizes, B, C):
    (hi, wi), (ho, wo) = sizes
    g = _gen(11, hi, wi, ho, wo, B, C)
    x, gy = torch.randn(B * hi * wi, C, generator=g), torch.randn(B * ho * wo, C, generator=g)

    def ref(dt, xs, gs):
        xv, gv = _cast(dt, xs, gs)
        xv.requires_grad_()
        y = to.resize_rows(xv, B, hi, wi, ho, wo)
        y.backward(gv)
        return y.detach(), xv.grad

    y, dx = _resize_gpu(x, gy, B, hi, wi, ho, wo, C)
    assert torch.isfinite(dx).all()
    r64, r32 = ref(torch.float64, x, gy), ref(torch.float32, x, gy)
    what = "%dx%d->%dx%d B%d C%d" % (hi, wi, ho, wo, B, C)
    failures = []
    _check("resize_fwd", what, y, r64[0], r32[0], failures)
    _check("resize_bwd", what, dx, r64[1], r32[1], failures)
    # <resize(x), g> = <x, resize_backward(g)> on the kernels' own outputs, in float64.  Positive operands, so that the inner
    # product is a sum of like-signed terms and the floor (1e-6 of it) is not at the mercy of a cancellation; the yardstick is
    # the same residual of float32 CPU torch.
    xp, gp = x.abs() + 0.5, gy.abs() + 0.5
    yk, dxk = _resize_gpu(xp, gp, B, hi, wi, ho, wo, C)
    yt, dxt = ref(torch.float32, xp, gp)
    lhs = (yk.cpu().double() * gp.double()).sum().item()
    res = abs(lhs - (xp.double() * dxk.cpu().double()).sum().item())
    yard = abs((yt.double() * gp.double()).sum().item() - (xp.double() * dxt.double()).sum().item())
    bar = max(4 * yard, 1e-6 * abs(lhs))
    print("thermal[resize adjoint] %s: error %.3e, yardstick %.3e, bar %.3e (maximum %.3e), ratio %.2f"
          % (what, res, yard, bar, abs(lhs), res / max(yard, 0.25e-6 * abs(lhs))))
    if not res <= bar:
        failures.append(("resize adjoint", what, res, bar))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# rows_kernel
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["finalize", "scale", "axpy"])
def test_rows_op(mode):
    failures = []
    for rows in (1, 257):
        for Fe in (1, 3, 300):
            for t in TIMES:
                g = _gen(12, rows, Fe, t)
                p, q, r = (torch.randn(rows, Fe, generator=g) for _ in range(3))
                sa, s1 = to.coefficients(t)
                pb, qb, rb = _wide(p, 1, 2), _wide(q, 3, 0), _wide(r, 0, 4)
                ptr = lambda buf, off: buf.data_ptr() + 4 * off
                if mode == "finalize":  # as _unet_forward calls it
                    args = (THERMAL_ROWS_FINALIZE, rows, Fe, sa, s1, ptr(pb, 1), pb.shape[1], ptr(qb, 3), qb.shape[1], ptr(rb, 0), rb.shape[1])
                    ref = lambda dt: to.rows_finalize(p.to(dt), q.to(dt), r.to(dt), sa, s1)
                elif mode == "scale":  # as _ScoreFunction.backward calls it: d pred / d eps_hat
                    c = float(-s1 / sa)
                    args = (THERMAL_ROWS_SCALE, rows, Fe, c, 0.0, ptr(pb, 1), pb.shape[1], None, 0, None, 0)
                    ref = lambda dt: to.rows_scale(p.to(dt), c)
                else:
                    args = (THERMAL_ROWS_AXPY, rows, Fe, float(sa), 0.0, ptr(pb, 1), pb.shape[1], ptr(qb, 3), qb.shape[1], None, 0)
                    ref = lambda dt: to.rows_axpy(p.to(dt), q.to(dt), float(sa))

                def run():
                    obuf = _blank(rows, Fe, 2, 2)
                    th.rows_op(*args, ptr(obuf, 2), int(obuf.shape[1]), obuf)
                    return (_extent(obuf, 2, Fe),)

                (got,) = _twice(run)
                _check("rows_kernel %s" % mode, "%dx%d t%d" % (rows, Fe, t), got, ref(torch.float64), ref(torch.float32), failures)
    assert not failures, failures


def test_residual_pass_through_is_a_copy():
    """FINALIZE with s1 = 0 and sa = 1 (no noise, no correction) returns the clean rows bit for bit, and so does the E_DIFFUSE
    epilogue of a convolution."""
    g = _gen(13)
    rows, Fe = 70, 5
    p, q, r = (torch.randn(rows, Fe, generator=g) for _ in range(3))
    pb, qb, rb = _wide(p, 1, 2), _wide(q, 3, 0), _wide(r, 0, 4)
    obuf = _blank(rows, Fe, 2, 2)
    th.rows_op(THERMAL_ROWS_FINALIZE, rows, Fe, 1.0, 0.0, pb.data_ptr() + 4, pb.shape[1], qb.data_ptr() + 12, qb.shape[1], rb.data_ptr(),
               rb.shape[1], obuf.data_ptr() + 8, int(obuf.shape[1]), obuf)
    assert _same_bits(_extent(obuf, 2, Fe).cpu(), p)
    w, b, eps = _dev(torch.randn(Fe, Fe, 3, 3, generator=g), torch.randn(Fe, generator=g), q)
    obuf = _blank(rows, Fe, 2, 2)
    ends = th._Ends(pb[:, 1:1 + Fe], int(pb.shape[1]), eps, 1.0, 0.0, Fe)
    th.conv(_v(rb, 0, Fe, 2, 5, 7), THERMAL_A_PLAIN, None, w, b, _v(obuf, 2, Fe, 2, 5, 7), ends=ends, e_mode=THERMAL_E_DIFFUSE)
    assert _same_bits(_extent(obuf, 2, Fe).cpu(), p)


# ---------------------------------------------------------------------------------------------------------------------
# rejections: refused in host code, before any launch
# ---------------------------------------------------------------------------------------------------------------------


def test_rejections():
    L = _lib.lib()
    B, H, W, C, G = 2, 3, 4, 8, 4
    M = B * H * W
    g = _gen(14)
    xbuf = _wide(torch.randn(M, C, generator=g), 1, 1)
    xv = _v(xbuf, 1, C, B, H, W)
    w, b, eps = _dev(torch.randn(C, C, 3, 3, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g))
    ss = _dev(torch.ones(B * C), torch.zeros(B * C))
    gamma, beta = _dev(torch.ones(C), torch.zeros(C))
    obuf = _blank(M, C, 1, 1)
    ov = _v(obuf, 1, C, B, H, W)
    small = torch.full((B * G * 2 + 2 * B * C + C,), NAN, dtype=torch.float32, device=DEV)  # stats, scale, shift, column sums
    stats, scale, shift, sums = small[:B * G * 2], small[B * G * 2:B * G * 2 + B * C], small[B * G * 2 + B * C:-C], small[-C:]
    idx = torch.full((M, C), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    s = th._stream(xbuf)
    ends = th._Ends(xbuf[:, 1:1 + C], int(xbuf.shape[1]), eps, 0.9, 0.4, C)

    def conv_args(**change):
        a = th._conv_args(xv, change.pop("a_mode", THERMAL_A_PLAIN), ss, w, b, ov, ends, change.pop("e_mode", THERMAL_E_STORE),
                          packed=th._tap_major(w, 1, 0))
        for k, v in change.items():
            setattr(a, k, v)
        return a

    good = conv_args()
    nb_w = L.gw_thermal_conv_wgrad_workspace_bytes(good)
    nb_c = L.gw_thermal_colsum_workspace_bytes(M, C)
    nb_g = L.gw_thermal_groupnorm_workspace_bytes(B, H * W, C, G)
    assert 0 < nb_w <= ws.numel() and 0 < nb_c <= ws.numel() and 0 < nb_g <= ws.numel()
    p = lambda t: t.data_ptr()
    gn_f = lambda C_, G_, ld, nb: L.gw_thermal_groupnorm_forward(B, H * W, C_, G_, xv.ptr, ld, p(gamma), p(beta), 1e-5, p(ws), nb, p(stats),
                                                                 p(scale), p(shift), s)
    gn_b = lambda C_, G_, ld, nb: L.gw_thermal_groupnorm_backward(B, H * W, C_, G_, xv.ptr, ld, p(ss[0]), p(ss[1]), p(stats), p(gamma), xv.ptr,
                                                                  xv.ld, p(ws), nb, ov.ptr, p(sums), p(sums), s)
    rows = lambda mode, sa, ld: L.gw_thermal_rows(mode, M, C, sa, 0.4, xv.ptr, ld, p(eps), C, xv.ptr, xv.ld, ov.ptr, ov.ld, s)
    refused = [
        ("gw_thermal_conv", "ld_a < cin", lambda: L.gw_thermal_conv_forward(conv_args(ld_a=C - 1), s)),
        ("gw_thermal_conv", "ld_out < cout", lambda: L.gw_thermal_conv_forward(conv_args(ld_out=C - 1), s)),
        ("gw_thermal_conv", "a_mode 3", lambda: L.gw_thermal_conv_forward(conv_args(a_mode=3), s)),
        ("gw_thermal_conv", "a_mode -1", lambda: L.gw_thermal_conv_forward(conv_args(a_mode=-1), s)),
        ("gw_thermal_conv", "e_mode 2", lambda: L.gw_thermal_conv_forward(conv_args(e_mode=2), s)),
        ("gw_thermal_conv", "e_mode 2 (wgrad)", lambda: L.gw_thermal_conv_wgrad(conv_args(e_mode=2), p(ws), nb_w, ov.ptr, s)),
        ("gw_thermal_conv", "features != cout",
         lambda: L.gw_thermal_conv_forward(conv_args(e_mode=THERMAL_E_DIFFUSE, features=C - 1), s)),
        ("gw_thermal_conv", "sa = 0", lambda: L.gw_thermal_conv_forward(conv_args(e_mode=THERMAL_E_DIFFUSE, sa=0.0), s)),
        ("gw_thermal_conv_wgrad", "workspace one byte short", lambda: L.gw_thermal_conv_wgrad(good, p(ws), nb_w - 1, ov.ptr, s)),
        ("gw_thermal_colsum", "ld < cols", lambda: L.gw_thermal_colsum(M, C, xv.ptr, C - 1, p(ws), nb_c, p(sums), s)),
        ("gw_thermal_colsum", "workspace one byte short", lambda: L.gw_thermal_colsum(M, C, xv.ptr, xv.ld, p(ws), nb_c - 1, p(sums), s)),
        ("gw_thermal_groupnorm_forward", "ld < C", lambda: gn_f(C, G, C - 1, nb_g)),
        ("gw_thermal_groupnorm_forward", "C % groups", lambda: gn_f(C, 3, xv.ld, nb_g)),
        ("gw_thermal_groupnorm_forward", "workspace one byte short", lambda: gn_f(C, G, xv.ld, nb_g - 1)),
        ("gw_thermal_groupnorm_backward", "ld < C", lambda: gn_b(C, G, C - 1, nb_g)),
        ("gw_thermal_groupnorm_backward", "C % groups", lambda: gn_b(C, 3, xv.ld, nb_g)),
        ("gw_thermal_groupnorm_backward", "workspace one byte short", lambda: gn_b(C, G, xv.ld, nb_g - 1)),
        ("gw_thermal_maxpool_forward", "ld_x < C",
         lambda: L.gw_thermal_maxpool_forward(B, H, W, C, xv.ptr, C - 1, p(ss[0]), p(ss[1]), ov.ptr, ov.ld, p(idx), s)),
        ("gw_thermal_maxpool_forward", "ld_out < C",
         lambda: L.gw_thermal_maxpool_forward(B, H, W, C, xv.ptr, xv.ld, p(ss[0]), p(ss[1]), ov.ptr, C - 1, p(idx), s)),
        ("gw_thermal_maxpool_backward", "ld_g1 < C", lambda: L.gw_thermal_maxpool_backward(B, H, W, C, p(idx), xv.ptr, C - 1, None, 0, ov.ptr, s)),
        ("gw_thermal_maxpool_backward", "ld_g2 < C",
         lambda: L.gw_thermal_maxpool_backward(B, H, W, C, p(idx), xv.ptr, xv.ld, xv.ptr, C - 1, ov.ptr, s)),
        ("gw_thermal_resize_forward", "ld_x < C", lambda: L.gw_thermal_resize_forward(B, H, W, H, W, C, xv.ptr, C - 1, ov.ptr, ov.ld, s)),
        ("gw_thermal_resize_forward", "ld_out < C", lambda: L.gw_thermal_resize_forward(B, H, W, H, W, C, xv.ptr, xv.ld, ov.ptr, C - 1, s)),
        ("gw_thermal_resize_backward", "ld_g < C", lambda: L.gw_thermal_resize_backward(B, H, W, H, W, C, xv.ptr, C - 1, ov.ptr, s)),
        ("gw_thermal_rows", "ld_p < F", lambda: rows(THERMAL_ROWS_FINALIZE, 0.9, C - 1)),
        ("gw_thermal_rows", "mode 3", lambda: rows(3, 0.9, xv.ld)),
        ("gw_thermal_rows", "sa = 0", lambda: rows(THERMAL_ROWS_FINALIZE, 0.0, xv.ld)),
    ]
    for entry, what, call in refused:
        rc = call()
        msg = L.gw_last_error().decode(errors="replace")
        print("thermal[rejection] %s, %s: %d, %r" % (entry, what, rc, msg))
        assert rc in (-1, -2), (entry, what, rc)  # GW_E_BADARG / GW_E_UNSUPPORTED, never GW_OK or GW_E_LAUNCH
        assert msg.startswith(entry), (entry, what, msg)
    torch.cuda.synchronize()
    assert torch.isnan(obuf).all() and torch.isnan(small).all() and (idx == -7).all(), "a refused call wrote to its output"
    # the same arguments unchanged are accepted
    assert L.gw_thermal_conv_forward(good, s) == 0
    assert torch.isfinite(_extent(obuf, 1, C)).all()
