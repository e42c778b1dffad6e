"""The FengWu-GHR kernels (csrc/gw_fengwu.hip) and models on the GPU against the float64 restatement (tests/fengwu_oracle.py).

Bars.  Forward: 1e-5 of the output's maximum - what tests/test_gpu_wide.py holds the fp32-MFMA paths to.  Gradients: the
yardstick is the float32 CPU restatement's own error against float64 on the same case, computed here; the kernels may err at
most 4 x that (a different summation order of the tiles, and the probabilities are recomputed), with a floor of 1e-6 of the
gradient's maximum.  Every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

import graph_weather_amd as gw
from graph_weather_amd import fengwu_ghr as fg

from . import fengwu_oracle as fo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FWD_BAR = 1e-5


def _check_forward(what, got, ref64):
    scale = ref64.abs().max().item()
    err = (got.detach().cpu().double() - ref64).abs().max().item() / scale
    print("%s: forward error %.3e of the maximum (bar %.0e)" % (what, err, FWD_BAR))
    assert err <= FWD_BAR, (what, err)


def _check_gradient(what, got, ref64, yard32):
    """got: ours; ref64: the oracle's; yard32: the float32 CPU restatement's."""
    scale = ref64.abs().max().item()
    yard = (yard32.double() - ref64).abs().max().item()
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    bar = max(4.0 * yard, 1e-6 * scale)
    print("%s: gradient error %.3e, yardstick %.3e, bar %.3e (maximum %.3e)" % (what, err, yard, bar, scale))
    assert err <= bar, (what, err, yard, bar)
    return (err / scale, yard / scale) if scale > 0 else (0.0, 0.0)  # (a single key: dq = dk = 0 exactly)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
# (batch, heads, N, dim_head, mode): pairs = batch * heads in {1, 3, 40}; N over the packed form (<= 16), the tile edges (63, 64, 65),
# several tiles with a ragged tail (130, 300); every dim_head padding (8 -> 16, 32, 64, 128).  mode "big": q scaled so that
# the scores reach +-120; "offset": the buffer view starts one float off 16-byte alignment (the scalar load / store path).
# dim_head 6 and 20 (not multiples of 4; beyond the issue's list): the feature tail inside a group of four and head columns
# that are not 16-byte aligned.
ATTENTION_CASES = [
    (1, 1, 1, 8, ""), (1, 3, 1, 64, ""), (1, 3, 9, 64, ""), (10, 4, 9, 32, ""), (1, 1, 9, 128, ""), (10, 4, 16, 128, ""),
    (1, 3, 17, 64, ""), (10, 4, 17, 128, ""), (1, 1, 63, 32, ""), (1, 3, 64, 64, ""), (10, 4, 65, 8, ""), (1, 1, 130, 128, ""),
    (1, 3, 130, 64, ""), (1, 1, 300, 64, ""), (3, 1, 300, 32, ""), (1, 3, 65, 64, "big"), (1, 3, 9, 32, "big"),
    (1, 3, 65, 64, "offset"), (2, 2, 9, 8, "offset"), (2, 2, 9, 6, ""), (1, 3, 65, 20, ""),
]


def _attention_case(batch, heads, n, d, mode):
    inner = heads * d
    rs = np.random.RandomState(1000 * n + 10 * d + batch)
    qkv = torch.from_numpy(rs.standard_normal((batch * n, 3 * inner)).astype(np.float32))
    dout = torch.from_numpy(rs.standard_normal((batch * n, inner)).astype(np.float32))
    scale = d ** -0.5
    if mode == "big":
        q, k = qkv[:, :inner].reshape(batch, n, heads, d), qkv[:, inner:2 * inner].reshape(batch, n, heads, d)
        s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()).abs().max().item() * scale
        qkv[:, :inner] *= 120.0 / s
    return qkv, dout, scale


def _attention_oracle(qkv, dout, batch, heads, n, d, scale, dtype):
    inner = heads * d
    t = qkv.to(dtype).clone().requires_grad_(True)
    q, k, v = (c.reshape(batch, n, heads, d).permute(0, 2, 1, 3) for c in t.split(inner, dim=-1))
    out = fo.attention_core(q, k, v, scale).permute(0, 2, 1, 3).reshape(batch * n, inner)
    (out * dout.to(dtype)).sum().backward()
    dots = torch.matmul(q, k.transpose(-1, -2)) * scale
    return out.detach(), t.grad, torch.logsumexp(dots.detach(), dim=-1).reshape(batch * heads, n)


@pytest.mark.parametrize("batch,heads,n,d,mode", ATTENTION_CASES)
def test_attention_forward_and_backward(batch, heads, n, d, mode):
    inner = heads * d
    qkv, dout, scale = _attention_case(batch, heads, n, d, mode)
    ref, dref, lse_ref = _attention_oracle(qkv, dout, batch, heads, n, d, scale, torch.float64)
    _, dyard, _ = _attention_oracle(qkv, dout, batch, heads, n, d, scale, torch.float32)
    if mode == "big":
        dots = torch.einsum("bihd,bjhd->bhij", qkv[:, :inner].reshape(batch, n, heads, d).double(),
                            qkv[:, inner:2 * inner].reshape(batch, n, heads, d).double()) * scale
        assert dots.max() > 100 and dots.min() < -100 and not torch.isfinite(torch.exp(dots.float())).all()
    # the operands are strided views of a wider buffer (row stride != 3 inner); "offset" breaks the 16-byte alignment
    off = 1 if mode == "offset" else 0
    buf = torch.full((batch * n, 3 * inner + 8), float("nan"), device=DEV)
    view = buf[:, off:off + 3 * inner]
    view.copy_(qkv)
    gbuf = torch.full((batch * n, inner + 4), float("nan"), device=DEV)
    gview = gbuf[:, off:off + inner]
    gview.copy_(dout)
    what = "attention b%d h%d n%d d%d %s" % (batch, heads, n, d, mode)
    out, lse = fg.attention_forward(view, batch, heads, n, d, scale)
    dqkv = fg.attention_backward(view, out, lse, gview, batch, heads, n, d, scale)
    out2, lse2 = fg.attention_forward(view, batch, heads, n, d, scale)
    dqkv2 = fg.attention_backward(view, out2, lse2, gview, batch, heads, n, d, scale)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "forward is not bitwise reproducible"
    assert torch.equal(dqkv, dqkv2), "backward is not bitwise reproducible"
    _check_forward(what, out, ref)
    assert (lse.cpu().double().sum(0) - lse_ref).abs().max().item() <= 1e-5 * max(1.0, lse_ref.abs().max().item())  # maximum + log sum
    for name, lo in (("dq", 0), ("dk", inner), ("dv", 2 * inner)):
        _check_gradient(what + " " + name, dqkv[:, lo:lo + inner], dref[:, lo:lo + inner], dyard[:, lo:lo + inner])


def test_attention_autograd_node_and_dim_head_limit():
    batch, heads, n, d = 2, 2, 20, 16
    qkv, dout, scale = _attention_case(batch, heads, n, d, "")
    _, dref, _ = _attention_oracle(qkv, dout, batch, heads, n, d, scale, torch.float64)
    _, dyard, _ = _attention_oracle(qkv, dout, batch, heads, n, d, scale, torch.float32)
    t = qkv.to(DEV).requires_grad_(True)
    out = fg._Attention.apply(t, batch, heads, n, d, scale)
    (out * dout.to(DEV)).sum().backward()
    _check_gradient("attention autograd node", t.grad, dref, dyard)
    with pytest.raises(NotImplementedError, match="dim_head"):
        fg.attention_forward(torch.zeros(4, 3 * 160, device=DEV), 1, 1, 4, 160, 160 ** -0.5)
    with pytest.raises(NotImplementedError, match="dim_head"):
        gw.ImageMetaModel(image_size=8, patch_size=4, depth=1, heads=1, mlp_dim=5, channels=2, dim_head=160)


# ---------------------------------------------------------------------------------------------------------------------
# knn_interpolate, GELU
# ---------------------------------------------------------------------------------------------------------------------
def _knn_positions(name):
    grid5 = torch.tensor(fo.lat_lons_5deg()).to(torch.long)
    if name == "grid5_to_image20":
        return grid5, fo.image_positions(20, 20), (20, 20)
    return fo.image_positions(20, 20), grid5, None  # image -> rows


@pytest.mark.parametrize("name", ["grid5_to_image20", "image20_to_grid5"])
def test_knn_interpolate_forward_and_backward(name):
    pos_x, pos_y, image = _knn_positions(name)
    table = fg.KnnTable(pos_x, pos_y)
    assign = fo.knn_assign(pos_x, pos_y)
    weights = fo.knn_weights(pos_x, pos_y, assign)
    batch, c = 3, 5
    rs = np.random.RandomState(7)
    n_src, n_tgt = pos_x.shape[0], pos_y.shape[0]
    flat = torch.from_numpy(rs.standard_normal((n_src, batch * c)).astype(np.float32))  # the reference's "n (b c)" layout
    g = torch.from_numpy(rs.standard_normal((n_tgt, batch * c)).astype(np.float32))

    def oracle(dtype):
        t = flat.to(dtype).clone().requires_grad_(True)
        y = fo.knn_interpolate(t, assign, weights)
        (y * g.to(dtype)).sum().backward()
        return y.detach(), t.grad

    ref, dref = oracle(torch.float64)
    _, dyard = oracle(torch.float32)
    rows = lambda t, n: t.reshape(n, batch, c).permute(1, 0, 2).contiguous()  # noqa: E731  n (b c) -> b n c
    if image is not None:  # [B, n, c] rows -> [B, c, h, w] image
        x = rows(flat, n_src).to(DEV).requires_grad_(True)
        y = fg._Knn.apply(x, table, False, (batch, c) + image)
        got = y.permute(2, 3, 0, 1).reshape(n_tgt, batch * c)
        y.backward(g.reshape(image + (batch, c)).permute(2, 3, 0, 1).contiguous().to(DEV))
        dgot = x.grad.permute(1, 0, 2).reshape(n_src, batch * c)
    else:  # image -> rows
        x = flat.reshape(20, 20, batch, c).permute(2, 3, 0, 1).contiguous().to(DEV).requires_grad_(True)
        y = fg._Knn.apply(x, table, True, (batch, n_tgt, c))
        got = y.permute(1, 0, 2).reshape(n_tgt, batch * c)
        y.backward(rows(g, n_tgt).to(DEV))
        dgot = x.grad.permute(2, 3, 0, 1).reshape(n_src, batch * c)
    _check_forward("knn_interpolate " + name, got, ref)
    _check_gradient("knn_interpolate " + name, dgot, dref, dyard)
    # targets on top of exactly one source (weight 1e16): the source row comes through
    hit = (weights[:, 0] == 1e16) & (weights[:, 1] < 1e16)
    assert hit.sum() > 10
    src = flat[assign[hit, 0]].double()
    rel = ((got.detach().cpu().double()[hit] - src).abs() / src.abs().clamp_min(1e-30)).max().item()
    print("knn_interpolate %s: %d coincident targets, relative error %.3e" % (name, int(hit.sum()), rel))
    assert rel <= 1e-6


@pytest.mark.parametrize("rows,mlp_dim", [(1, 5), (777, 7), (20000, 5)])
def test_gelu_forward_and_backward(rows, mlp_dim):
    rs = np.random.RandomState(rows)
    x = torch.from_numpy(rs.uniform(-6.0, 6.0, (rows, mlp_dim)).astype(np.float32))
    x.view(-1)[:3] = torch.tensor([-6.0, 6.0, 0.0])[:min(3, x.numel())]
    g = torch.from_numpy(rs.standard_normal((rows, mlp_dim)).astype(np.float32))

    def oracle(dtype):
        t = x.to(dtype).clone().requires_grad_(True)
        y = fo.gelu(t)
        (y * g.to(dtype)).sum().backward()
        return y.detach(), t.grad

    ref, dref = oracle(torch.float64)
    _, dyard = oracle(torch.float32)
    t = x.to(DEV).requires_grad_(True)
    y = fg._Gelu.apply(t)
    y.backward(g.to(DEV))
    _check_forward("gelu %dx%d" % (rows, mlp_dim), y, ref)
    _check_gradient("gelu %dx%d" % (rows, mlp_dim), t.grad, dref, dyard)


# ---------------------------------------------------------------------------------------------------------------------
# the models: golden parity and gradients of every parameter and of the input
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_gradients(model, x, fn, g, dtype):
    sd = fo.params(model, dtype, requires_grad=True)
    t = x.to(dtype).clone().requires_grad_(True)
    out = fn(sd, t)
    (out * g.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["input"] = t.grad
    return out.detach(), grads


@pytest.mark.parametrize("name", fo.ALL_CASES)
def test_model_parity_and_gradients(golden_dir, name):
    model, x, fn = fo.build(gw, name)
    golden = torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["out"])
    g = torch.from_numpy(np.random.RandomState(5).standard_normal(tuple(golden.shape)).astype(np.float32))
    ref, gref = _oracle_gradients(model, x, fn, g, torch.float64)
    _, gyard = _oracle_gradients(model, x, fn, g, torch.float32)
    model = model.to(DEV)
    if hasattr(model, "knn_provider"):
        assert model.knn_provider == "builtin"
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd)
    assert tuple(out.shape) == tuple(golden.shape)
    _check_forward(name + " against the restatement", out, ref)
    _check_forward(name + " against the reference's output", out, golden.double())
    out.backward(g.to(DEV))
    worst = (0.0, 0.0)
    names = dict(model.named_parameters())
    assert set(names) | {"input"} == set(gref)
    for key in sorted(gref):
        got = xd.grad if key == "input" else names[key].grad
        assert got is not None, key
        worst = max(worst, _check_gradient(name + " " + key, got, gref[key], gyard[key]))
    print("%s: worst gradient error %.3e of its maximum (yardstick there %.3e)" % ((name,) + worst))


def test_training_step_lowers_the_loss():
    """train/era5.py's step: MetaModel -> NormalizedMSELoss -> backward -> AdamW, six times on one batch."""
    lat_lons = fo.lat_lons_5deg()
    cfg, batch, seed = fo.META_CASES["fengwu_meta_5deg"]
    model = fo.fill_(gw.MetaModel(lat_lons, **cfg), seed).to(DEV)
    x = fo.rows_input(cfg, batch, seed, len(lat_lons)).to(DEV)
    target = fo.rows_input(cfg, batch, seed + 1, len(lat_lons)).to(DEV)
    criterion = gw.NormalizedMSELoss(lat_lons=lat_lons, feature_variance=[1.0] * cfg["channels"], device=DEV)
    opt = gw.AdamW(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = criterion(model(x), target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("fengwu training losses:", " ".join("%.5f" % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_captured_forward_replays_bitwise():
    model, x, _ = fo.build(gw, "fengwu_wrapper_meta_5deg")
    model = model.to(DEV).eval()
    x = x.to(DEV)
    with torch.no_grad():
        eager = model(x).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        model(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = model(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(x.flip(0))  # new input in place: the replay follows it
    with torch.no_grad():
        eager2 = model(x).clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2) and not torch.equal(eager, eager2)
