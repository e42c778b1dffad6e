"""WeatherMesh's convolution towers, encoder, decoder and model on the GPU: the kernels of csrc/gw_convnd.hip one by one against
``torch.nn.functional`` in float64, the blocks and the model against the float64 restatements of tests/weathermesh_model_oracle.py
and against the outputs recorded from the reference's own classes (tests/golden/weathermesh_model_*.npz), three optimizer steps,
and a closed form that needs no oracle.

Bar, the project's standing one (``_bar`` of tests/test_gpu_weathermesh.py): the yardstick is the float32 CPU restatement's own
error against float64 on the same case (for the recorded cases: the recorded float32 output's); ours may err at most 4 x that,
with a floor of 1e-6 of the tensor's maximum; the yardstick itself must be within 1e-3 of that maximum.  Every figure is printed
before it is asserted.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from graph_weather_amd import weathermesh_model as wm

from . import weathermesh_model_oracle as mo
from .cafa_oracle import params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {"ratio": 0.0, "what": ""}


def _bar(what, got, ref64, yard32):
    """got: ours; ref64: the oracle's; yard32: the float32 CPU restatement's."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), what
    scale = ref64.abs().max().item()
    yard = (yard32.double().reshape(ref64.shape) - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    bar = max(4.0 * yard, 1e-6 * scale)
    ratio = err / yard if yard > 0 else 0.0
    print("%s: error %.3e, yardstick %.3e, bar %.3e (maximum %.3e), ratio %.2f" % (what, err, yard, bar, scale, ratio))
    if err > 1e-6 * scale and ratio > WORST["ratio"]:
        WORST.update(ratio=ratio, what=what)
    assert yard <= 1e-3 * scale, (what, yard, scale)
    assert err <= bar, (what, err, yard, bar)


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for s, t in zip(a, b):
        assert (s is None and t is None) or torch.equal(s, t)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# the convolution primitive
# ---------------------------------------------------------------------------------------------------------------------
# name: (kernel, stride, cin, cout, input shape, bias, output layout, BN_GELU load mode)
CONV_CASES = {
    "2d k3 s2 3->8": (3, 2, 3, 8, (2, 3, 13, 18), False, "plain", False),
    "2d k1 s2 3->8": (1, 2, 3, 8, (2, 3, 13, 18), False, "plain", False),
    "3d k3 s(1,2,2) 4->8": (3, (1, 2, 2), 4, 8, (2, 4, 3, 13, 18), False, "plain", False),
    "3d k3 s1 8->70": (3, 1, 8, 70, (1, 8, 2, 9, 10), False, "plain", False),
    "3d k1 s1 16->8 bias channels-last": (1, 1, 16, 8, (2, 16, 4, 4, 5), True, "channels_last", False),
    "2d k3 s2 5->6 short axes": (3, 2, 5, 6, (1, 5, 1, 2), False, "plain", False),
    "3d k3 s(1,2,2) 4->8 depth slice": (3, (1, 2, 2), 4, 8, (2, 4, 3, 13, 18), False, "depth_slice", False),
    "3d k3 s(1,2,2) 4->8 bn_gelu": (3, (1, 2, 2), 4, 8, (2, 4, 3, 13, 18), False, "plain", True),
    "2d k3 s1 8->70 bn_gelu": (3, 1, 8, 70, (1, 8, 9, 10), False, "plain", True),
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_convolution_against_float64(name):
    """Forward, data gradient and weight gradient, each launched twice and bitwise equal."""
    k, stride, cin, cout, shape, with_bias, layout, bn_gelu = CONV_CASES[name]
    rank = len(shape) - 2
    rs = np.random.RandomState(len(name) + cin * cout)
    x = _randn(rs, *shape)
    w = _randn(rs, cout, cin, *([k] * rank)) / math.sqrt(cin * k ** rank)
    bias = 0.5 * _randn(rs, cout) if with_bias else None
    table = torch.stack([1.0 + 0.3 * _randn(rs, cin), 0.2 * _randn(rs, cin), torch.zeros(cin), torch.ones(cin)]) if bn_gelu else None
    out_shape = wm._out_shape(shape, cout, wm._triple(stride, rank, "stride"))
    assert out_shape[2:] == tuple((n - 1) // s + 1 for n, s in zip(shape[2:], wm._triple(stride, rank, "stride")[3 - rank:]))
    dout = _randn(rs, *out_shape)

    def oracle(dtype):
        xa = x.to(dtype)
        if bn_gelu:
            view = [1, -1] + [1] * rank
            xa = F.gelu(xa * table[0].to(dtype).view(view) + table[1].to(dtype).view(view))
        xa = xa.detach().requires_grad_(True)
        ps = [w.to(dtype).requires_grad_(True)] + ([bias.to(dtype).requires_grad_(True)] if with_bias else [])
        out = mo.conv(xa, ps[0], stride, k // 2, ps[1] if with_bias else None)
        assert tuple(out.shape) == out_shape
        return [out.detach()] + list(torch.autograd.grad((out * dout.to(dtype)).sum(), [xa] + ps))

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    xd, wd, dd = x.to(DEV), w.to(DEV), dout.to(DEV)
    bd = bias.to(DEV) if with_bias else None
    td = table.to(DEV) if bn_gelu else None

    def forward():
        if layout == "channels_last":  # [B, D, H, W, C] rows, written through the strides of the permuted view
            rows = torch.full((out_shape[0],) + out_shape[2:] + (cout,), float("nan"), device=DEV)
            return [wm.convnd_forward(xd, wd, stride, bias=bd, bn=td, out=rows.permute(0, 4, 1, 2, 3)).contiguous()]
        if layout == "depth_slice":  # planes 1 .. D of a buffer with D + 2 planes; the others stay untouched
            buf = torch.full(out_shape[:2] + (out_shape[2] + 2,) + out_shape[3:], 7.0, device=DEV)
            got = wm.convnd_forward(xd, wd, stride, bias=bd, bn=td, out=buf[:, :, 1:-1])
            assert not got.is_contiguous() and (buf[:, :, 0] == 7.0).all() and (buf[:, :, -1] == 7.0).all()
            return [got.contiguous()]
        return [wm.convnd_forward(xd, wd, stride, bias=bd, bn=td)]

    got = _twice(forward) + _twice(lambda: [wm.convnd_dgrad(dd, wd, stride, shape)]) + _twice(
        lambda: list(wm.convnd_wgrad(xd, dd, w.shape, stride, bn=td, need_bias=with_bias)))
    for nm, g_, r_, y_ in zip(("out", "dx", "dw", "db"), got, ref, yard):
        _bar("%s %s" % (name, nm), g_, r_, y_)
    # dx accumulates into a given tensor: twice the gradient (exactly, in floating point: g + g)
    acc = wm.convnd_dgrad(dd, wd, stride, shape, dx=got[1].clone(), accumulate=True)
    assert torch.equal(acc, got[1] + got[1])


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_batchnorm_statistics_against_float64(offset):
    """Mean, rstd, scale, shift and both running updates; at offset 50 with unit spread E[x^2] - E[x]^2 in float32 loses the
    variance (shown: its error exceeds the bar) and the two-pass kernel does not."""
    rs = np.random.RandomState(3)
    x = offset + _randn(rs, 2, 5, 3, 7, 9)
    gamma, beta, rm, rv = 1.0 + 0.3 * _randn(rs, 5), 0.2 * _randn(rs, 5), 0.1 * _randn(rs, 5), 0.5 + _randn(rs, 5).abs()
    n = x.numel() // 5

    def oracle(dtype):
        xx = x.to(dtype)
        mean, var = xx.mean((0, 2, 3, 4)), xx.var((0, 2, 3, 4), unbiased=False)
        rstd = 1 / torch.sqrt(var + 1e-5)
        scale = gamma.to(dtype) * rstd
        return [scale, beta.to(dtype) - mean * scale, mean, rstd, 0.9 * rm.to(dtype) + 0.1 * mean, 0.9 * rv.to(dtype) + 0.1 * var * n / (n - 1)]

    def ours():
        m, v = rm.to(DEV), rv.to(DEV)
        st = wm.bn_stats(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, True, m, v)
        return [st[0], st[1], st[2], st[3], m, v]

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    got = _twice(ours)
    for nm, g_, r_, y_ in zip(("scale", "shift", "mean", "rstd", "running_mean", "running_var"), got, ref, yard):
        _bar("statistics offset %g %s" % (offset, nm), g_, r_, y_)
    if offset:
        naive = (x * x).mean((0, 2, 3, 4)) - x.mean((0, 2, 3, 4)) ** 2
        true = x.double().var((0, 2, 3, 4), unbiased=False)
        ours_var = 1 / got[3].cpu().double() ** 2 - 1e-5
        print("variance at offset 50: naive float32 error %.3e, ours %.3e" % ((naive - true).abs().max(), (ours_var - true).abs().max()))
        assert (naive - true).abs().max() > 20 * (ours_var - true).abs().max()
    # eval mode reads the running buffers and leaves them alone; x is not read
    m, v = rm.to(DEV), rv.to(DEV)
    st = wm.bn_stats(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, False, m, v).cpu().double()
    rstd = 1 / torch.sqrt(rv.double() + 1e-5)
    want = torch.stack([gamma.double() * rstd, beta.double() - rm.double() * gamma.double() * rstd, rm.double(), rstd])
    assert torch.equal(m.cpu(), rm) and torch.equal(v.cpu(), rv)
    assert (st - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def test_num_batches_tracked_and_the_one_value_per_channel_error():
    block = wm.ConvDownBlock(3, 8).to(DEV)
    x = _randn(np.random.RandomState(0), 2, 3, 6, 6).to(DEV)
    block.train()(x)
    assert [int(b.num_batches_tracked) for b in (block.bn1, block.bn2, block.bn_down)] == [1, 1, 1]
    block.eval()(x)
    assert [int(b.num_batches_tracked) for b in (block.bn1, block.bn2, block.bn_down)] == [1, 1, 1]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        block.train()(x[:1, :, :2, :2])  # conv2's output is [1, 8, 1, 1]
    assert block.eval()(x[:1, :, :2, :2]).shape == (1, 8, 1, 1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        wm.bn_stats(x[:1, :, :1, :1], block.bn1.weight[:3], block.bn1.bias[:3], 1e-5, 0.1, True, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# upsampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 2, 3, 1, 2), (1, 1, 1, 1)])
def test_upsampling_against_interpolate_in_float64(shape):
    rs = np.random.RandomState(sum(shape))
    x = _randn(rs, *shape)
    dout = _randn(rs, *shape[:-2], 2 * shape[-2], 2 * shape[-1])

    def oracle(dtype):
        xx = x.to(dtype).requires_grad_(True)
        out = mo.upsample(xx)
        return [out.detach(), torch.autograd.grad((out * dout.to(dtype)).sum(), xx)[0]]

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    got = _twice(lambda: [wm.upsample2x_forward(x.to(DEV)), wm.upsample2x_backward(dout.to(DEV))])
    for nm, g_, r_, y_ in zip(("out", "dx"), got, ref, yard):
        _bar("upsample %s %s" % (shape, nm), g_, r_, y_)


# ---------------------------------------------------------------------------------------------------------------------
# the blocks
# ---------------------------------------------------------------------------------------------------------------------
# name: (class, arguments, keywords, input shape, input offset)
BLOCK_CASES = {
    "down 2d 3->8": ("ConvDownBlock", (3, 8), {}, (2, 3, 13, 18), 0.0),
    "down 2d 3->8 offset 50": ("ConvDownBlock", (3, 8), {}, (2, 3, 13, 18), 50.0),
    "down 3d 4->8": ("ConvDownBlock", (4, 8), dict(stride=(1, 2, 2), is_3d=True), (2, 4, 3, 13, 18), 0.0),
    "down 3d 8->70": ("ConvDownBlock", (8, 70), dict(stride=(1, 2, 2), is_3d=True), (1, 8, 2, 9, 10), 0.0),
    "up 2d 8->3": ("ConvUpBlock", (8, 3), {}, (2, 8, 4, 5), 0.0),
    "up 3d 16->5": ("ConvUpBlock", (16, 5), dict(is_3d=True), (2, 16, 3, 4, 5), 0.0),
}


def block_oracle(name, dtype, training):
    """(out, dx, parameter gradients, buffer updates) of the restatement on the CPU in ``dtype``."""
    cls, args, kw, shape, offset = BLOCK_CASES[name]
    rs = np.random.RandomState(len(name))
    x = (offset + _randn(rs, *shape)).to(dtype).requires_grad_(True)
    module = mo.fill_model_(getattr(wm, cls)(*args, **kw), 40 + len(name))
    p = {k: v.to(dtype) if v.is_floating_point() else v for k, v in params(module, torch.float32).items()}
    learn = {k: v.requires_grad_(True) for k, v in p.items() if k in dict(module.named_parameters())}
    updates = {}
    if cls == "ConvDownBlock":
        out = mo.down_block(p, "", x, kw.get("stride", 2), training, updates)
    else:
        out = mo.up_block(p, "", x, training, updates)
    dout = _randn(rs, *out.shape)
    grads = torch.autograd.grad((out * dout.to(dtype)).sum(), [x] + list(learn.values()))
    return out.detach(), grads[0], dict(zip(learn, grads[1:])), updates, module, x.detach().float(), dout


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_blocks_against_float64(name, training):
    ref = block_oracle(name, torch.float64, training)
    yard = block_oracle(name, torch.float32, training)
    module, x, dout = ref[4].to(DEV).train(training), ref[5].to(DEV).requires_grad_(True), ref[6].to(DEV)
    before = {k: v.clone() for k, v in module.state_dict().items() if "running_" in k}
    out = module(x)
    out.backward(dout)
    what = "%s %s" % (name, "train" if training else "eval")
    _bar(what + " out", out, ref[0], yard[0])
    _bar(what + " dx", x.grad, ref[1], yard[1])
    for k, prm in module.named_parameters():
        assert prm.grad is not None and ref[2][k].abs().max().item() > 0, k
        _bar("%s d %s" % (what, k), prm.grad, ref[2][k], yard[2][k])
    for k, v in before.items():
        if training:
            _bar("%s %s" % (what, k), module.state_dict()[k], ref[3][k], yard[3][k])
        else:
            assert torch.equal(module.state_dict()[k], v), k
    assert set(ref[3]) == (set(before) if training else set())


@pytest.mark.parametrize("cls,args,kw,shape", [("ConvDownBlock", (3, 8), {}, (2, 3, 5, 6)),
                                               ("ConvUpBlock", (8, 3), dict(is_3d=True), (1, 8, 2, 3, 2))])
def test_closed_form_zero_convolutions_give_gelu_of_twice_the_bias(cls, args, kw, shape):
    """Every convolution weight zero, gamma = 1, beta = b: each BatchNorm sees zeros (mean 0, variance 0) and returns b, so
    the block's output is the constant gelu(2 b) in both modes - no oracle involved."""
    b = 0.3
    block = getattr(wm, cls)(*args, **kw)
    with torch.no_grad():
        for k, v in block.named_parameters():
            v.fill_(0.0 if v.dim() > 1 else (1.0 if k.endswith("weight") else b))
        for k, v in block.named_buffers():
            if k.endswith("running_mean"):
                v.zero_()
    block = block.to(DEV)
    want = 0.5 * (2 * b) * (1 + math.erf(2 * b / math.sqrt(2)))
    x = _randn(np.random.RandomState(1), *shape).to(DEV)
    for training in (True, False):
        out = block.train(training)(x)
        err = (out.double() - want).abs().max().item()
        print("closed form %s %s: gelu(2 b) = %.9f, largest error %.3e" % (cls, "train" if training else "eval", want, err))
        assert err <= 1e-6 * want


# ---------------------------------------------------------------------------------------------------------------------
# encoder, decoder, model
# ---------------------------------------------------------------------------------------------------------------------
def _tables(model, dtype):
    conv = lambda m: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params(m, torch.float32).items()}  # noqa: E731
    return conv(model), [conv(q) for q in model.processors]


def _to_device(model):
    model.to(DEV)
    for q in model.processors:  # a plain list: .to() does not reach them
        q.to(DEV)
    return model


@functools.lru_cache(maxsize=None)
def model_oracle(name, training):
    """Float64 outputs and buffer updates of the restatement with the case's weights."""
    model = mo.build_model(wm.WeatherMesh, name)
    p, procs = _tables(model, torch.float64)
    surface, pressure = mo.case_inputs(name)
    updates = {}
    with torch.no_grad():
        out = mo.model_forward(p, procs, surface.double(), pressure.double(), mo.FORECAST_STEPS, mo.MODEL_KW, training, updates)
    return out, updates


@pytest.mark.parametrize("name", list(mo.CASES))
def test_model_against_the_recorded_outputs_of_the_reference_classes(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert int(g["seed"]) == mo.CASES[name][2]
    model = _to_device(mo.build_model(wm.WeatherMesh, name))
    surface, pressure = (t.to(DEV) for t in mo.case_inputs(name))
    for training, pre in ((False, ""), (True, "train_")):
        ref, updates = model_oracle(name, training)
        with torch.no_grad():
            out = model.train(training)(surface, pressure, mo.FORECAST_STEPS)
        assert isinstance(out, wm.WeatherMeshOutput) and out.surface.is_contiguous() and out.pressure.is_contiguous()
        assert tuple(out.surface.shape) == g[pre + "surface"].shape and tuple(out.pressure.shape) == g[pre + "pressure"].shape
        _bar("%s %ssurface" % (name, pre), out.surface, ref[0], torch.from_numpy(g[pre + "surface"]))
        _bar("%s %spressure" % (name, pre), out.pressure, ref[1], torch.from_numpy(g[pre + "pressure"]))
    sd = model.state_dict()
    assert set(updates) == {k for k in sd if "running_" in k}
    for k, v in updates.items():
        _bar("%s %s" % (name, k), sd[k], v, torch.from_numpy(g["buffer/" + k]))
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    if name.endswith("13x18"):  # 13 -> 7 -> 4 and 18 -> 9 -> 5, then 2^2 x: larger than the input
        assert tuple(out.surface.shape) == (2, 3, 16, 20) and tuple(out.pressure.shape) == (2, 4, 3, 16, 20)


def _halves_oracle(dtype):
    """Encoder output from the case inputs and decoder outputs from a random latent, eval mode."""
    name = "weathermesh_model_13x18"
    model = mo.build_model(wm.WeatherMesh, name)
    p, _ = _tables(model, dtype)
    surface, pressure = mo.case_inputs(name)
    latent_in = _randn(np.random.RandomState(77), 2, 4, 4, 5, 8)
    kw = mo.MODEL_KW
    with torch.no_grad():
        latent = mo.encoder_forward(p, "encoder.", surface.to(dtype), pressure.to(dtype), 2, 1, kw["kernel"], kw["num_heads"], False, {})
        s, q = mo.decoder_forward(p, "decoder.", latent_in.to(dtype), 2, 1, kw["kernel"], kw["num_heads"], False, {})
    return model, (surface, pressure, latent_in), (latent, s, q)


def test_encoder_and_decoder_alone_against_float64():
    model, (surface, pressure, latent_in), ref = _halves_oracle(torch.float64)
    yard = _halves_oracle(torch.float32)[2]
    model = _to_device(model).eval()
    with torch.no_grad():
        latent = model.encoder(surface.to(DEV), pressure.to(DEV))
        s, q = model.decoder(latent_in.to(DEV))
    assert tuple(latent.shape) == (2, 4, 4, 5, 8) and latent.is_contiguous()  # channels-last rows, the surface plane last
    for nm, g_, r_, y_ in zip(("encoder latent", "decoder surface", "decoder pressure"), (latent, s, q), ref, yard):
        _bar(nm, g_, r_, y_)


def _train_oracle(dtype):
    """Outputs and every gradient (the model's parameters, then the processors') of one training-mode step at (24, 32)."""
    name = "weathermesh_model_24x32"
    model = mo.build_model(wm.WeatherMesh, name)
    p, procs = _tables(model, dtype)
    names = [k for k, _ in model.named_parameters()]
    leaves = [p[k].requires_grad_(True) for k in names] + [q[k].requires_grad_(True) for q in procs for k in q]
    surface, pressure = mo.case_inputs(name)
    rs = np.random.RandomState(5)
    ws, wp = _randn(rs, 2, 3, 24, 32), _randn(rs, 2, 4, 3, 24, 32)
    s, q = mo.model_forward(p, procs, surface.to(dtype), pressure.to(dtype), mo.FORECAST_STEPS, mo.MODEL_KW, True, {})
    grads = torch.autograd.grad((s * ws.to(dtype)).sum() + (q * wp.to(dtype)).sum(), leaves)
    return model, (surface, pressure, ws, wp), [s.detach(), q.detach()] + list(grads), names


def test_training_mode_gradients_of_the_whole_model_against_float64():
    model, (surface, pressure, ws, wp), ref, names = _train_oracle(torch.float64)
    yard = _train_oracle(torch.float32)[2]
    model = _to_device(model).train()
    out = model(surface.to(DEV), pressure.to(DEV), mo.FORECAST_STEPS)
    ((out.surface * ws.to(DEV)).sum() + (out.pressure * wp.to(DEV)).sum()).backward()
    ours = [dict(model.named_parameters())[k] for k in names] + [v for q in model.processors for v in q.state_dict(keep_vars=True).values()]
    labels = names + ["processors[%d].%s" % (i, k) for i, q in enumerate(model.processors) for k in q.state_dict()]
    _bar("training surface", out.surface, ref[0], yard[0])
    _bar("training pressure", out.pressure, ref[1], yard[1])
    assert len(ours) == len(ref) - 2
    for label, prm, r_, y_ in zip(labels, ours, ref[2:], yard[2:]):
        assert prm.grad is not None and r_.abs().max().item() > 0, label
        _bar("training d " + label, prm.grad, r_, y_)


def _three_steps():
    name = "weathermesh_model_13x18"
    model = _to_device(mo.build_model(wm.WeatherMesh, name)).train()
    leaves = list(model.parameters()) + [v for q in model.processors for v in q.parameters()]
    opt = torch.optim.AdamW(leaves, lr=3e-3)
    surface, pressure = (t.to(DEV) for t in mo.case_inputs(name))
    rs = np.random.RandomState(9)
    ts, tp = _randn(rs, 2, 3, 16, 20).to(DEV), _randn(rs, 2, 4, 3, 16, 20).to(DEV)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = model(surface, pressure, mo.FORECAST_STEPS)
        loss = (out.surface - ts).square().mean() + (out.pressure - tp).square().mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return losses + [v.detach().clone() for v in leaves] + [v.clone() for k, v in model.state_dict().items() if "running_" in k]


def test_three_adamw_steps_reduce_the_loss_and_are_bitwise_repeatable():
    a, b = _three_steps(), _three_steps()
    torch.cuda.synchronize()
    print("losses of three AdamW steps: %.6f %.6f %.6f" % tuple(t.item() for t in a[:3]))
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and all(torch.isfinite(t).all() for t in a)
    assert a[2].item() < a[1].item() < a[0].item()


def test_zz_worst_ratio():
    print("worst ratio to the float32 CPU yardstick: %.2f (%s)" % (WORST["ratio"], WORST["what"]))
    assert WORST["ratio"] <= 4.0
