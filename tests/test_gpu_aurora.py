"""The Aurora kernels (csrc/gw_aurora.hip, csrc/gw_conv3d.hip, the MASKED attention of csrc/gw_fengwu.hip) and models on the GPU
against float64 restatements (tests/aurora_oracle.py and the torch compositions below).

Bars, those of tests/test_gpu_fengwu.py and tests/test_gpu_cafa.py for gradients, applied to every result here: the yardstick is
the float32 CPU restatement's own error against float64 on the same case, computed here; the kernels may err at most 4 x that,
with a floor of 1e-6 of the result's maximum.  Every figure is printed before it is asserted.  Nothing compares the kernels
with themselves, except where bitwise equality is the claim (repeat runs, the all-zero bias, checkpointing, graph replay).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_weather_amd as gw
from graph_weather_amd import aurora
from graph_weather_amd import fengwu_ghr as fg

from . import aurora_oracle as ao

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")


def _check(what, got, ref64, yard32):
    """got: ours; ref64: the oracle's; yard32: the float32 CPU restatement's."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), what
    scale = ref64.abs().max().item()
    yard = (yard32.double().reshape(ref64.shape) - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    bar = max(4.0 * yard, 1e-6 * scale)
    print("%s: error %.3e, yardstick %.3e, bar %.3e (maximum %.3e)" % (what, err, yard, bar, scale))
    assert err <= bar, (what, err, yard, bar)


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# masked attention
# ---------------------------------------------------------------------------------------------------------------------
def _keep(pattern, B, n):
    """Boolean [B, n], True = the key is kept; the samples of a case differ."""
    keep = torch.ones(B, n, dtype=torch.bool)
    if pattern == "none":
        pass
    elif pattern == "tail":      # sample 0 loses its tail, sample 1 its head
        keep[0, n // 2 + 1:] = False
        keep[-1, : n // 3] = False
    elif pattern == "single":    # one kept key in sample 0; sample 1 keeps all but one
        keep[0] = False
        keep[0, min(5, n - 1)] = True
        keep[-1, 0] = B == 1
    elif pattern == "inside":    # the boundary inside the first key block; sample 1: the whole leading block of 64 (32) keys dropped
        keep[0, 40:] = False
        keep[-1, :64] = False
    else:
        raise KeyError(pattern)
    assert keep.any(dim=1).all()
    return keep


# (B, n, heads, dim_head, mask pattern, mode): n = 1; the packed form (n <= 16) at 9 and 16; 17; 70 = one block of 64 and a ragged
# second one.  mode "big": q scaled so that the scores reach +-120.
MASKED_CASES = [
    (1, 1, 1, 12, "none", ""), (2, 9, 2, 12, "tail", ""), (2, 16, 1, 32, "single", ""), (2, 17, 2, 32, "single", ""),
    (2, 17, 1, 12, "tail", "big"), (2, 70, 2, 12, "inside", ""), (2, 70, 1, 32, "inside", "big"), (2, 70, 2, 32, "tail", ""),
]


def _scores(qkv, B, n, heads, d):
    inner = heads * d
    t = qkv.double().reshape(B, n, 3 * inner)
    q, k = (t[..., lo:lo + inner].reshape(B, n, heads, d) for lo in (0, inner))
    return torch.einsum("bihd,bjhd->bhij", q, k) * d ** -0.5


@functools.lru_cache(maxsize=None)
def _masked_case(B, n, heads, d, pattern, mode):
    inner = heads * d
    rs = np.random.RandomState(100 * n + d + B)
    qkv, dout = _randn(rs, B * n, 3 * inner), _randn(rs, B * n, inner)
    if mode == "big":
        qkv[:, :inner] *= 120.0 / _scores(qkv, B, n, heads, d).abs().max().item()
    keep = _keep(pattern, B, n)
    bias = torch.zeros(B, n).masked_fill(~keep, -INF)
    return qkv, dout, keep, bias


@functools.lru_cache(maxsize=None)
def _masked_oracle(B, n, heads, d, pattern, mode, dtype):
    qkv, dout, _, bias = _masked_case(B, n, heads, d, pattern, mode)
    inner = heads * d
    t = qkv.to(dtype).clone().requires_grad_(True)
    q, k, v = (c.reshape(B, n, heads, d).permute(0, 2, 1, 3) for c in t.reshape(B, n, 3 * inner).split(inner, dim=-1))
    sim = (q @ k.transpose(-1, -2)) * d ** -0.5 + bias.to(dtype)[:, None, None, :]
    out = (sim.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * n, inner)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), t.grad


@pytest.mark.parametrize("B,n,heads,d,pattern,mode", MASKED_CASES)
def test_masked_attention_forward_and_backward(B, n, heads, d, pattern, mode):
    inner, scale = heads * d, d ** -0.5
    qkv, dout, keep, bias = _masked_case(B, n, heads, d, pattern, mode)
    ref, dref = _masked_oracle(B, n, heads, d, pattern, mode, torch.float64)
    yard, dyard = _masked_oracle(B, n, heads, d, pattern, mode, torch.float32)
    if mode == "big":
        dots = _scores(qkv, B, n, heads, d)
        print("scores in [%.1f, %.1f]" % (dots.min().item(), dots.max().item()))
        assert dots.max() > 100 and dots.min() < -100
    what = "masked attention B%d n%d h%d d%d %s %s" % (B, n, heads, d, pattern, mode)
    q_dev, g_dev, b_dev = qkv.to(DEV), dout.to(DEV), bias.to(DEV)
    out, lse = aurora.attention_masked_forward(q_dev, b_dev, B, heads, n, d, scale)
    dqkv = aurora.attention_masked_backward(q_dev, b_dev, out, lse, g_dev, B, heads, n, d, scale)
    out2, lse2 = aurora.attention_masked_forward(q_dev, b_dev, B, heads, n, d, scale)
    dqkv2 = aurora.attention_masked_backward(q_dev, b_dev, out2, lse2, g_dev, B, heads, n, d, scale)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse).all()
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2) and torch.equal(lse, lse2)
    _check(what + " out", out, ref, yard)
    _check(what + " dqkv", dqkv, dref, dyard)
    dropped = (~keep).reshape(B * n).to(DEV)
    if dropped.any():  # dk and dv of a dropped key are exactly zero
        assert (dqkv[dropped][:, inner:] == 0).all()
        assert (dref[dropped.cpu()][:, inner:] == 0).all()


@pytest.mark.parametrize("B,n,heads,d", [(2, 9, 2, 12), (3, 16, 1, 32), (2, 17, 2, 12), (2, 70, 2, 32)])
def test_zero_bias_reproduces_the_unmasked_kernels_bitwise(B, n, heads, d):
    inner, scale = heads * d, d ** -0.5
    rs = np.random.RandomState(n + d)
    qkv, dout = _randn(rs, B * n, 3 * inner).to(DEV), _randn(rs, B * n, inner).to(DEV)
    zero = torch.zeros(B, n, device=DEV)
    out, lse = aurora.attention_masked_forward(qkv, zero, B, heads, n, d, scale)
    dqkv = aurora.attention_masked_backward(qkv, zero, out, lse, dout, B, heads, n, d, scale)
    out0, lse0 = fg.attention_forward(qkv, B, heads, n, d, scale)
    dqkv0 = fg.attention_backward(qkv, out0, lse0, dout, B, heads, n, d, scale)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(lse, lse0) and torch.equal(dqkv, dqkv0)


# ---------------------------------------------------------------------------------------------------------------------
# EarthSystemLoss
# ---------------------------------------------------------------------------------------------------------------------
def _points(kind, n):
    if kind == "lattice":
        return {108: lambda: ao.lattice(31), 300: lambda: ao.lattice(32, n_lon=20, n_lat=15)}[n]()
    rs = np.random.RandomState(n)
    if kind == "far":     # a row of points 10 degrees apart: no pair but (i, i) inside the radius
        return np.stack([10.0 * np.arange(n) - 5.0 * n, rs.uniform(-1, 1, n)], axis=-1).astype(np.float32)
    if kind == "near":    # everything inside a 2 degree box
        return rs.uniform(-1, 1, (n, 2)).astype(np.float32)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _loss_case(kind, n, c):
    rs = np.random.RandomState(7 * n + c)
    pred = 250.0 + 200.0 * rs.standard_normal((1, n, c))
    target = pred + 5.0 * rs.standard_normal((1, n, c))
    return (torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(target.astype(np.float32)),
            torch.from_numpy(_points(kind, n)[None]))


@functools.lru_cache(maxsize=None)
def _loss_oracle(kind, n, c, dtype):
    """(the four values, d value_k / d pred and d value_k / d target for each k, G) of the restatement."""
    pred, target, pts = (t.to(dtype) for t in _loss_case(kind, n, c))
    pred.requires_grad_(True)
    target.requires_grad_(True)
    out = ao.earth_loss(pred, target, pts, 0.5, 0.3, 0.2)
    vals = torch.stack([out[k] for k in ao.LOSS_KEYS])
    grads = []
    for k in range(4):
        gp, gt = torch.autograd.grad(vals[k], (pred, target), retain_graph=True, allow_unused=True)
        grads.append((torch.zeros_like(pred) if gp is None else gp, torch.zeros_like(pred) if gt is None else gt))
    e = (pred - target).detach()[0]
    near = (((pts[0][:, None] - pts[0][None]) ** 2).sum(-1) < 25.0).to(dtype)
    G = (near[:, :, None] * (e[:, None, :] - e[None, :, :])).sum(1)
    return vals.detach(), grads, G


LOSS_CASES = [("near", 1, 3), ("lattice", 108, 1), ("lattice", 108, 3), ("lattice", 300, 5), ("near", 70, 5), ("far", 40, 3)]


@pytest.mark.parametrize("kind,n,c", LOSS_CASES)
def test_earth_system_loss_values_pair_rows_and_gradients(kind, n, c):
    pred, target, pts = _loss_case(kind, n, c)
    vals, grads, G = _loss_oracle(kind, n, c, torch.float64)
    yvals, ygrads, yG = _loss_oracle(kind, n, c, torch.float32)
    what = "earth loss %s n%d c%d" % (kind, n, c)
    p, t, q = pred.to(DEV).requires_grad_(True), target.to(DEV).requires_grad_(True), pts.to(DEV)
    out, Gd, _ = aurora.earth_loss_forward(p.detach(), t.detach(), q, True, 0.5, 0.3, 0.2)
    out2, Gd2, _ = aurora.earth_loss_forward(p.detach(), t.detach(), q, True, 0.5, 0.3, 0.2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(Gd, Gd2)  # two runs are bitwise equal
    for k, key in enumerate(ao.LOSS_KEYS):
        _check("%s %s" % (what, key), out[k], vals[k], yvals[k])
    _check(what + " pair rows G", Gd, G, yG)
    if kind == "far":
        assert float(out[2]) == 0.0 and (Gd == 0).all()  # exactly
    if kind == "near" and n > 1:
        assert float(vals[2]) > 0 and (G != 0).any()
    res = gw.EarthSystemLoss(0.5, 0.3, 0.2)(p, t, q)
    assert list(res) == list(ao.LOSS_KEYS) and all(v.dim() == 0 for v in res.values())
    for k, key in enumerate(ao.LOSS_KEYS):  # the gradient of each of the four outputs taken separately
        gp, gt = torch.autograd.grad(res[key], (p, t), retain_graph=True)
        _check("%s d %s / d pred" % (what, key), gp, grads[k][0], ygrads[k][0])
        _check("%s d %s / d target" % (what, key), gt, grads[k][1], ygrads[k][1])
        if kind == "far" and key == "spatial_correlation_loss":
            assert (gp == 0).all() and (gt == 0).all()
    sp = gw.EarthSystemLoss().spatial_correlation_loss(p, t, q)
    assert torch.equal(sp.detach(), out[2])


def test_mse_and_physical_terms_batch_2():
    rs = np.random.RandomState(11)
    B, n, c = 2, 301, 4
    pred64 = torch.from_numpy(250.0 + 200.0 * rs.standard_normal((B, n, c)))
    target64 = pred64 + torch.from_numpy(5.0 * rs.standard_normal((B, n, c)))
    pts64 = torch.from_numpy(np.stack([rs.uniform(-180, 180, (B, n)), rs.uniform(-90, 90, (B, n))], axis=-1))

    def oracle(dtype):
        p, t = pred64.to(dtype).requires_grad_(True), target64.to(dtype).requires_grad_(True)
        mse, phys = ((p - t) ** 2).mean(), ao.physical_loss(p, pts64.to(dtype))
        vals = [0.5 * mse + 0.2 * phys, mse, phys]
        grads = [torch.autograd.grad(v, (p, t), retain_graph=True, allow_unused=True) for v in vals]
        return [v.detach() for v in vals], [(gp, torch.zeros_like(p) if gt is None else gt) for gp, gt in grads]

    vals, grads = oracle(torch.float64)
    yvals, ygrads = oracle(torch.float32)
    p, t, q = pred64.float().to(DEV).requires_grad_(True), target64.float().to(DEV).requires_grad_(True), pts64.float().to(DEV)
    out = aurora._EarthLoss.apply(p, t, q, False, 0.5, 0.3, 0.2)
    assert float(out[2].detach()) == 0.0
    for k, (idx, key) in enumerate([(0, "total"), (1, "mse"), (3, "physical")]):
        _check("batch 2 " + key, out[idx], vals[k], yvals[k])
        gp, gt = torch.autograd.grad(out[idx], (p, t), retain_graph=True)
        _check("batch 2 d %s / d pred" % key, gp, grads[k][0], ygrads[k][0])
        _check("batch 2 d %s / d target" % key, gt, grads[k][1], ygrads[k][1])
    phys = gw.EarthSystemLoss().physical_loss(p, q)
    _check("batch 2 physical_loss()", phys, vals[2], yvals[2])
    (gp,) = torch.autograd.grad(phys, (p,))
    _check("batch 2 d physical_loss() / d pred", gp, grads[2][0], ygrads[2][0])
    with pytest.raises(RuntimeError, match="one sample"):
        gw.EarthSystemLoss()(p, t, q)


# ---------------------------------------------------------------------------------------------------------------------
# 3 x 3 x 3 convolutions
# ---------------------------------------------------------------------------------------------------------------------
# (transposed, (d, h, w), cin, cout): one voxel; a small odd volume; 1224 voxels per sample = 2448 in all, two slabs and a partial
# third, and 39 row tiles the last of which is ragged
CONV_CASES = [(False, (1, 1, 1), 1, 8), (False, (3, 4, 5), 3, 8), (False, (8, 9, 17), 3, 96), (False, (8, 9, 17), 1, 8),
              (True, (1, 1, 1), 3, 2), (True, (3, 4, 5), 8, 1), (True, (8, 9, 17), 96, 2)]


@functools.lru_cache(maxsize=None)
def _conv_case(transposed, dhw, cin, cout):
    rs = np.random.RandomState(dhw[2] + 10 * cin + cout)
    x = _randn(rs, 2, cin, *dhw)
    w = _randn(rs, *((cin, cout) if transposed else (cout, cin)), 3, 3, 3) / np.sqrt(27.0 * cin)
    b = 0.1 * _randn(rs, cout)
    g = _randn(rs, 2, cout, *dhw)
    return x, w, b, g


@functools.lru_cache(maxsize=None)
def _conv_oracle(transposed, dhw, cin, cout, dtype):
    x, w, b, g = (t.to(dtype).clone().requires_grad_(True) for t in _conv_case(transposed, dhw, cin, cout))
    out = (F.conv_transpose3d if transposed else F.conv3d)(x, w, b, padding=1)
    (out * g.detach()).sum().backward()
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("transposed,dhw,cin,cout", CONV_CASES)
def test_conv3d_forward_data_and_weight_gradients(transposed, dhw, cin, cout):
    x, w, b, g = _conv_case(transposed, dhw, cin, cout)
    ref = _conv_oracle(transposed, dhw, cin, cout, torch.float64)
    yard = _conv_oracle(transposed, dhw, cin, cout, torch.float32)
    what = "%s %s cin %d cout %d" % ("ConvTranspose3d" if transposed else "Conv3d", dhw, cin, cout)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    if transposed:
        out = aurora._ConvTranspose3d.apply(xd, wd, bd)
        out.backward(g.to(DEV))
        got = out
    else:
        rows = aurora._Conv3dRows.apply(xd, wd, bd)  # [(b, d, h, w), cout]
        assert tuple(rows.shape) == (2 * dhw[0] * dhw[1] * dhw[2], cout)
        rows.backward(g.permute(0, 2, 3, 4, 1).reshape(-1, cout).to(DEV))
        got = rows.reshape(2, *dhw, cout).permute(0, 4, 1, 2, 3)
    torch.cuda.synchronize()
    _check(what + " out", got, ref[0], yard[0])
    _check(what + " dx", xd.grad, ref[1], yard[1])
    _check(what + " dweight", wd.grad, ref[2], yard[2])
    _check(what + " dbias", bd.grad, ref[3], yard[3])


# ---------------------------------------------------------------------------------------------------------------------
# weight gradients in one fixed order
# ---------------------------------------------------------------------------------------------------------------------
# (rows, m, n): one row; one slab; 2500 rows = two slabs of 1024 and a partial third; tiles with ragged edges (m, n not multiples of 64)
@pytest.mark.parametrize("rows,m,n", [(1, 3, 2), (108, 64, 5), (2500, 70, 130)])
def test_gemm_tn_ordered(rows, m, n):
    rs = np.random.RandomState(rows + m)
    a, b = _randn(rs, rows, m), _randn(rs, rows, n)
    ref, ref_sum = a.double().T @ b.double(), a.double().sum(0)
    c, colsum = aurora.gemm_tn_ordered(a.to(DEV), b.to(DEV), True)
    c2, colsum2 = aurora.gemm_tn_ordered(a.to(DEV), b.to(DEV), True)
    assert torch.equal(c, c2) and torch.equal(colsum, colsum2)
    _check("a^T b rows %d m %d n %d" % (rows, m, n), c, ref, a.T @ b)
    _check("column sums rows %d m %d" % (rows, m), colsum, ref_sum, a.sum(0))
    assert aurora.gemm_tn_ordered(a.to(DEV), b.to(DEV), False)[1] is None


# (rows, width): one row; a width that is no multiple of 64; 300 rows = one slab of 256 and a partial second
@pytest.mark.parametrize("rows,width", [(1, 32), (108, 70), (300, 96), (5, 300)])
def test_layernorm_backward_ordered(rows, width):
    rs = np.random.RandomState(rows + width)
    y, dn, gamma, beta = 3.0 * _randn(rs, rows, width) + 1.0, _randn(rs, rows, width), 1.0 + 0.25 * _randn(rs, width), _randn(rs, width)

    def oracle(dtype):
        t = [v.to(dtype).clone().requires_grad_(True) for v in (y, gamma, beta)]
        F.layer_norm(t[0], (width,), t[1], t[2], 1e-5).backward(dn.to(dtype))
        return [v.grad for v in t]

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    got = aurora.layernorm_backward_ordered(dn.to(DEV), y.to(DEV), gamma.to(DEV))
    got2 = aurora.layernorm_backward_ordered(dn.to(DEV), y.to(DEV), gamma.to(DEV))
    for k, key in enumerate(("dy", "dgamma", "dbeta")):
        assert torch.equal(got[k], got2[k])
        _check("LayerNorm backward rows %d width %d %s" % (rows, width, key), got[k], ref[k], yard[k])


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def _call(module, kind, t):
    if kind == "model":
        return module(t["points"], t["features"], t.get("mask"))
    if kind == "perceiver":
        return module(t["x"], t.get("attention_mask"))
    return module(t["x"])


def _oracle_gradients(name, module, inputs, g, dtype):
    sd = ao.params(module, dtype, requires_grad=True)
    t = {k: (v if v.dtype == torch.bool else v.to(dtype).clone().requires_grad_(k != "points")) for k, v in inputs.items()}
    out = ao.run(name, sd, t, dtype)
    (out * g.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads.update({"input:" + k: v.grad for k, v in t.items() if v.dtype != torch.bool and v.requires_grad})
    return out.detach(), grads


@pytest.mark.parametrize("name", [n for n, c in ao.CASES.items() if c[0] != "loss"])
def test_model_parity_and_gradients(golden_dir, name):
    kind = ao.CASES[name][0]
    module, inputs = ao.build(aurora, name), ao.case_inputs(name)
    golden = torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["out"])
    g = _randn(np.random.RandomState(5), *golden.shape)
    ref, gref = _oracle_gradients(name, module, inputs, g, torch.float64)
    yard, gyard = _oracle_gradients(name, module, inputs, g, torch.float32)
    module = module.to(DEV)  # eval(): dropout, where a class has it, is the identity; forward and backward both run
    t = {k: (v.to(DEV) if v.dtype == torch.bool else v.to(DEV).requires_grad_(k != "points")) for k, v in inputs.items()}
    out = _call(module, kind, t)
    assert tuple(out.shape) == tuple(golden.shape)
    _check(name + " against the restatement", out, ref, yard)  # tests/test_aurora_host.py ties the restatement to the reference
    out.backward(g.to(DEV))
    params = dict(module.named_parameters())
    assert set(params) | {k for k in gref if k.startswith("input:")} == set(gref)
    used = 0
    for key in sorted(gref):
        got = t[key[6:]].grad if key.startswith("input:") else params[key].grad
        if gref[key] is None:  # the decoder half of Swin3DEncoder's nn.Transformer: parameters only
            assert got is None and "swin_transformer.decoder" in key, key
            continue
        assert got is not None, key
        _check(name + " " + key, got, gref[key], gyard[key])
        used += 1
    print("%s: %d gradients checked" % (name, used))


def test_golden_loss_case(golden_dir):
    name = "aurora_loss_n108"
    golden = torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["out"])
    inputs = ao.case_inputs(name)
    ref, yard = ao.run(name, None, inputs), ao.run(name, None, inputs, torch.float32)
    res = ao.build(aurora, name)(*(inputs[k].to(DEV) for k in ("pred", "target", "points")))
    got = torch.stack([res[k] for k in ao.LOSS_KEYS])
    assert tuple(got.shape) == tuple(golden.shape)
    _check(name + " against the restatement", got, ref, yard)  # tests/test_aurora_host.py ties the restatement to the reference


def _training_case():
    rs = np.random.RandomState(3)
    pts = torch.from_numpy(ao.lattice(41)[None]).to(DEV)
    feats = _randn(rs, 1, 108, 5).to(DEV)
    target = (280.0 + 10.0 * _randn(rs, 1, 108, 3)).to(DEV)
    return pts, feats, target


def test_training_steps_reduce_the_loss():
    torch.manual_seed(0)
    model = gw.AuroraModel(5, 3, latent_dim=64, num_layers=2).to(DEV).train()  # no dropout anywhere: trains as it is
    loss_fn = gw.EarthSystemLoss()
    pts, feats, target = _training_case()
    opt = gw.AdamW(model.parameters(), lr=1e-2)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = loss_fn(model(pts, feats), target, pts)["total_loss"]
        losses.append(float(loss))
        if len(losses) < 4:
            loss.backward()
            opt.step()
    torch.cuda.synchronize()
    print("aurora training losses", losses)
    assert all(np.isfinite(v) for v in losses)
    assert losses[3] < losses[2] < losses[1] < losses[0]
    for k, v in model.named_parameters():
        assert torch.isfinite(v).all(), k
        assert not torch.equal(v, before[k]), k


def test_checkpointing_gives_the_same_gradients_bitwise():
    pts, feats, target = _training_case()
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(0)
        model = gw.AuroraModel(5, 3, latent_dim=64, num_layers=2, use_checkpointing=ckpt).to(DEV).train()
        loss = gw.EarthSystemLoss()(model(pts, feats), target, pts)["total_loss"]
        loss.backward()
        grads.append((float(loss), {k: v.grad.clone() for k, v in model.named_parameters()}))
    assert grads[0][0] == grads[1][0] and len(grads[0][1]) == 42
    for k in grads[0][1]:
        assert torch.equal(grads[0][1][k], grads[1][1][k]), k


def test_captured_inference_replays_on_a_changed_input():
    name = "aurora_model_b2_mask"
    model, inputs = ao.build(aurora, name).to(DEV), {k: v.to(DEV) for k, v in ao.case_inputs(name).items()}
    pts, feats, mask = inputs["points"], inputs["features"], inputs["mask"]
    with torch.no_grad():
        eager = model(pts, feats, mask).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        model(pts, feats, mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = model(pts, feats, mask)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    feats.copy_(feats.flip(0))  # new input in place: the replay follows it
    with torch.no_grad():
        eager2 = model(pts, feats, mask).clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2) and not torch.equal(eager, eager2)


def test_truncation_and_mask_errors_on_the_device():
    model = gw.AuroraModel(5, 3, latent_dim=64, num_layers=1, max_seq_len=50).to(DEV).eval()
    rs = np.random.RandomState(9)
    pts, feats = torch.from_numpy(ao.lattice(51)[None]).to(DEV), _randn(rs, 1, 108, 5).to(DEV)
    with torch.no_grad():
        out = model(pts, feats)
        assert tuple(out.shape) == (1, 50, 3)  # more than max_seq_len points are truncated
        assert torch.equal(out, model(pts[:, :50], feats[:, :50]))
        with pytest.raises(RuntimeError):  # ... and with a mask the reference's broadcast fails: so does ours
            model(pts, feats, torch.ones(1, 108, dtype=torch.bool, device=DEV))
