"""The CaFA kernels (axial addressing of csrc/gw_fengwu.hip, csrc/gw_cafa.hip) and models on the GPU against the float64
restatement (tests/cafa_oracle.py).

Bars, those of tests/test_gpu_fengwu.py.  Forward: 1e-5 of the output's maximum.  Gradients: the yardstick is the float32 CPU
restatement's own error against float64 on the same case, computed here; the kernels may err at most 4 x that, with a floor of
1e-6 of the gradient's maximum.  Every figure is printed before it is asserted.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_weather_amd as gw
from graph_weather_amd import _lib, cafa
from graph_weather_amd import fengwu_ghr as fg

from . import cafa_oracle as co

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FWD_BAR = 1e-5
NAN = float("nan")


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
    return (err / scale, yard / scale) if scale > 0 else (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# axial attention
# ---------------------------------------------------------------------------------------------------------------------
# (B, H, W, heads, dim_head, mode).  Along the height the sequences are (b, w) with n = H, along the width (b, h) with n = W:
# n over 1, the packed form (<= 16: (2, 3, 9) packs four sequences per workgroup across the batch boundary, 6 and 18 of them),
# the tile edge (64, 65) and several tiles with a ragged tail (90, 130); every dim_head padding (8 -> 16, 32, 64, 128) and 20
# (not a multiple of 4).  mode "big": q scaled so that the scores along the tested axis reach +-120; "offset": the buffer view starts
# one float off 16-byte alignment (the scalar load / store path).
AXIAL_CASES = [
    (1, 1, 1, 1, 8, ""), (2, 3, 9, 1, 8, ""), (2, 5, 16, 2, 32, "big"), (1, 17, 3, 3, 64, "offset"), (2, 3, 65, 3, 64, ""),
    (1, 64, 5, 1, 128, ""), (3, 90, 7, 2, 20, ""), (1, 130, 2, 1, 64, ""),
]


def _sequences(t, B, H, W, axis):
    """[(b h w), c] rows -> [sequences, n, c] along ``axis`` (a copy for the height)."""
    g = t.reshape(B, H, W, -1)
    return g.permute(0, 2, 1, 3).reshape(B * W, H, -1) if axis == 1 else g.reshape(B * H, W, -1)


def _rows_back(t, B, H, W, axis):
    """[sequences, n, c] -> [(b h w), c]"""
    c = t.shape[-1]
    return t.reshape(B, W, H, c).permute(0, 2, 1, 3).reshape(B * H * W, c) if axis == 1 else t.reshape(B * H * W, c)


def _scores(qkv, B, H, W, axis, heads, d):
    inner = heads * d
    s = _sequences(qkv.double(), B, H, W, axis)
    q, k = (s[..., lo:lo + inner].reshape(s.shape[0], s.shape[1], heads, d) for lo in (0, inner))
    return torch.einsum("bihd,bjhd->bhij", q, k) * d ** -0.5


@functools.lru_cache(maxsize=None)
def _axial_case(B, H, W, heads, d, mode, axis):
    inner = heads * d
    rs = np.random.RandomState(1000 * H + 10 * W + d + B)
    qkv = torch.from_numpy(rs.standard_normal((B * H * W, 3 * inner)).astype(np.float32))
    dout = torch.from_numpy(rs.standard_normal((B * H * W, inner)).astype(np.float32))
    if mode == "big":
        qkv[:, :inner] *= 120.0 / _scores(qkv, B, H, W, axis, heads, d).abs().max().item()
    return qkv, dout


@functools.lru_cache(maxsize=None)
def _axial_oracle(B, H, W, heads, d, mode, axis, dtype):
    """(out, dqkv, log-sum-exp [pairs, n]) of the restatement's attention core along ``axis``; computed once per case."""
    qkv, dout = _axial_case(B, H, W, heads, d, mode, axis)
    inner = heads * d
    t = qkv.to(dtype).clone().requires_grad_(True)
    s = _sequences(t, B, H, W, axis)
    q, k, v = (c.reshape(c.shape[0], c.shape[1], heads, d).permute(0, 2, 1, 3) for c in s.split(inner, dim=-1))
    sim = (q @ k.transpose(-1, -2)) * d ** -0.5
    o = (sim.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(s.shape[0], s.shape[1], inner)
    out = _rows_back(o, B, H, W, axis)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), t.grad, torch.logsumexp(sim.detach(), dim=-1).reshape(-1, s.shape[1])


def _buffers(B, H, W, heads, d, mode, axis):
    """qkv and dout as strided views of wider NaN-filled buffers."""
    qkv, dout = _axial_case(B, H, W, heads, d, mode, axis)
    inner, rows = heads * d, B * H * W
    off = 1 if mode == "offset" else 0
    buf = torch.full((rows, 3 * inner + 8), NAN, device=DEV)
    view = buf[:, off:off + 3 * inner]
    view.copy_(qkv)
    gbuf = torch.full((rows, inner + 4), NAN, device=DEV)
    gview = gbuf[:, off:off + inner]
    gview.copy_(dout)
    return buf, view, gbuf, gview, off


def _padding_is_nan(buf, off, width):
    return bool(torch.isnan(buf[:, :off]).all() and torch.isnan(buf[:, off + width:]).all())


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("B,H,W,heads,d,mode", AXIAL_CASES)
def test_axial_attention_forward_and_backward(B, H, W, heads, d, mode, axis):
    inner, rows, scale = heads * d, B * H * W, d ** -0.5
    ref, dref, lse_ref = _axial_oracle(B, H, W, heads, d, mode, axis, torch.float64)
    _, dyard, _ = _axial_oracle(B, H, W, heads, d, mode, axis, torch.float32)
    if mode == "big":
        dots = _scores(_axial_case(B, H, W, heads, d, mode, axis)[0], B, H, W, axis, heads, d)
        print("axis %d: scores in [%.1f, %.1f]" % (axis, dots.min().item(), dots.max().item()))
        assert dots.max() > 100 and dots.min() < -100 and not torch.isfinite(torch.exp(dots.float())).all()
    buf, view, gbuf, gview, off = _buffers(B, H, W, heads, d, mode, axis)
    what = "axial attention B%d H%d W%d h%d d%d axis %d %s" % (B, H, W, heads, d, axis, mode)
    out, lse = cafa.attention_axial_forward(view, B, H, W, axis, heads, d, scale)
    dqkv = cafa.attention_axial_backward(view, out, lse, gview, B, H, W, axis, heads, d, scale)
    out2, lse2 = cafa.attention_axial_forward(view, B, H, W, axis, heads, d, scale)
    dqkv2 = cafa.attention_axial_backward(view, out2, lse2, gview, B, H, W, axis, heads, d, scale)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (rows, inner) and tuple(dqkv.shape) == (rows, 3 * inner)
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse).all()
    assert _padding_is_nan(buf, off, 3 * inner) and _padding_is_nan(gbuf, off, inner)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "forward is not bitwise reproducible"
    assert torch.equal(dqkv, dqkv2), "backward is not bitwise reproducible"
    _check_forward(what, out, ref)
    assert (lse.cpu().double().sum(0) - lse_ref).abs().max().item() <= 1e-5 * max(1.0, lse_ref.abs().max().item())
    for name, lo in (("dq", 0), ("dk", inner), ("dv", 2 * inner)):
        _check_gradient(what + " " + name, dqkv[:, lo:lo + inner], dref[:, lo:lo + inner], dyard[:, lo:lo + inner])

    # the outputs through strides of their own: out and dqkv as views of wider NaN-filled buffers, by the C entry points
    L = _lib.lib()
    outer, inner_seq, n, sq = cafa._axial(B, H, W, axis, int(view.stride(0)))
    obuf = torch.full((rows, inner + 4), NAN, device=DEV)
    oview = obuf[:, off:off + inner]
    dbuf = torch.full((rows, 3 * inner + 8), NAN, device=DEV)
    dview = dbuf[:, off:off + 3 * inner]
    lse3 = torch.empty_like(lse)
    delta = torch.empty((outer * inner_seq * heads, n), device=DEV)
    so = cafa._axial(B, H, W, axis, inner + 4)[3]
    sd = cafa._axial(B, H, W, axis, 3 * inner + 8)[3]
    st = torch.cuda.current_stream().cuda_stream
    p, g = view.data_ptr(), dview.data_ptr()
    _lib.check(L.gw_attention_axial_forward(outer, inner_seq, heads, n, d, p, p + 4 * inner, p + 8 * inner, cafa._i3(sq), scale,
                                            oview.data_ptr(), cafa._i3(so), lse3.data_ptr(), st), "gw_attention_axial_forward")
    _lib.check(L.gw_attention_axial_backward(outer, inner_seq, heads, n, d, p, p + 4 * inner, p + 8 * inner, cafa._i3(sq), scale,
                                             oview.data_ptr(), cafa._i3(so), gview.data_ptr(), cafa._i3(so), lse3.data_ptr(),
                                             delta.data_ptr(), g, g + 4 * inner, g + 8 * inner, cafa._i3(sd), st),
               "gw_attention_axial_backward")
    torch.cuda.synchronize()
    assert torch.equal(oview, out) and torch.equal(lse3, lse) and torch.equal(dview, dqkv)
    assert _padding_is_nan(obuf, off, inner) and _padding_is_nan(dbuf, off, 3 * inner)


@pytest.mark.parametrize("B,H,W,heads,d,mode", AXIAL_CASES)
def test_axial_attention_is_the_existing_attention_bit_for_bit(B, H, W, heads, d, mode):
    """Same arithmetic, new addressing: the width axis against attention_forward on the same buffer (its rows are the sequences
    already), the height axis against attention_forward on a transposed contiguous copy, transposed back."""
    inner, scale = heads * d, d ** -0.5
    _, view, _, gview, _ = _buffers(B, H, W, heads, d, mode, 2)
    out, lse = cafa.attention_axial_forward(view, B, H, W, 2, heads, d, scale)
    dqkv = cafa.attention_axial_backward(view, out, lse, gview, B, H, W, 2, heads, d, scale)
    out0, lse0 = fg.attention_forward(view, B * H, heads, W, d, scale)
    dqkv0 = fg.attention_backward(view, out0, lse0, gview, B * H, heads, W, d, scale)
    assert torch.equal(out, out0) and torch.equal(lse, lse0) and torch.equal(dqkv, dqkv0)

    _, view, _, gview, _ = _buffers(B, H, W, heads, d, mode, 1)
    out, lse = cafa.attention_axial_forward(view, B, H, W, 1, heads, d, scale)
    dqkv = cafa.attention_axial_backward(view, out, lse, gview, B, H, W, 1, heads, d, scale)
    copy = _sequences(view, B, H, W, 1).reshape(B * W * H, 3 * inner).contiguous()
    gcopy = _sequences(gview, B, H, W, 1).reshape(B * W * H, inner).contiguous()
    out0, lse0 = fg.attention_forward(copy, B * W, heads, H, d, scale)
    dqkv0 = fg.attention_backward(copy, out0, lse0, gcopy, B * W, heads, H, d, scale)
    assert torch.equal(out, _rows_back(out0.reshape(B * W, H, inner), B, H, W, 1))
    assert torch.equal(lse, lse0)
    assert torch.equal(dqkv, _rows_back(dqkv0.reshape(B * W, H, 3 * inner), B, H, W, 1))


def test_axial_autograd_node():
    B, H, W, heads, d = 2, 5, 16, 2, 32
    for axis in (1, 2):
        qkv, dout = _axial_case(B, H, W, heads, d, "", axis)
        _, dref, _ = _axial_oracle(B, H, W, heads, d, "", axis, torch.float64)
        _, dyard, _ = _axial_oracle(B, H, W, heads, d, "", axis, torch.float32)
        t = qkv.to(DEV).requires_grad_(True)
        out = cafa._AxialAttention.apply(t, B, H, W, axis, heads, d, d ** -0.5)
        (out * dout.to(DEV)).sum().backward()
        _check_gradient("axial autograd node axis %d" % axis, t.grad, dref, dyard)
    with pytest.raises(NotImplementedError, match="dim_head"):
        cafa.attention_axial_forward(torch.zeros(4, 3 * 160, device=DEV), 1, 2, 2, 1, 1, 160, 160 ** -0.5)
    with pytest.raises(ValueError, match="Axis must be 1"):
        cafa.attention_axial_forward(torch.zeros(4, 24, device=DEV), 1, 2, 2, 3, 1, 8, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# patch embed / expand
# ---------------------------------------------------------------------------------------------------------------------
# (B, C, H, W, f, D): the model cases' shapes (even, padded, f = 3 with odd sizes, f = 1) and one whose padded ring is wider
# than the image remainder (5 = 4 + 1: rows and columns of patches with a single live pixel).  Patches: 1 024 (one full slab
# of the weight gradient), 1 122 (two slabs), 182, 153, 4; K = C f f = 12, 45, 4, 112 (two K steps of 64, ragged).
PATCH_CASES = [(2, 3, 32, 64, 2, 128), (2, 3, 33, 65, 2, 128), (2, 5, 20, 37, 3, 48), (1, 4, 9, 17, 1, 32), (1, 7, 5, 5, 4, 16)]
GUARD = 64


def _guarded(shape):
    """A NaN-filled tensor of ``shape`` inside a NaN-filled allocation with GUARD floats on either side."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    return big, big[GUARD:GUARD + n].view(shape)


def _guards_untouched(big):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[-GUARD:]).all())


@functools.lru_cache(maxsize=None)
def _patch_case(B, C, H, W, f, D):
    rs = np.random.RandomState(100 * H + W + f)
    oh, ow = -(-H // f), -(-W // f)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))  # noqa: E731
    k = C * f * f
    return dict(x=t(B, C, H, W), w_e=t(D, C, f, f) / k ** 0.5, b_e=0.1 * t(D), g_rows=t(B * oh * ow, D),
                rows=t(B * oh * ow, D), w_x=t(D, C, f, f) / D ** 0.5, b_x=0.1 * t(C), g_img=t(B, C, H, W))


@functools.lru_cache(maxsize=None)
def _patch_oracle(B, C, H, W, f, D, dtype):
    c = {k: v.to(dtype).clone().requires_grad_(True) for k, v in _patch_case(B, C, H, W, f, D).items()}
    oh, ow = -(-H // f), -(-W // f)
    xp = F.pad(c["x"], (0, ow * f - W, 0, oh * f - H))
    rows = F.conv2d(xp, c["w_e"], c["b_e"], stride=f).permute(0, 2, 3, 1).reshape(B * oh * ow, D)
    (rows * c["g_rows"]).sum().backward()
    img = F.conv_transpose2d(c["rows"].reshape(B, oh, ow, D).permute(0, 3, 1, 2), c["w_x"], c["b_x"], stride=f)[:, :, :H, :W]
    (img * c["g_img"]).sum().backward()
    return rows.detach(), img.detach(), {k: v.grad for k, v in c.items() if k not in ("g_rows", "g_img")}


@pytest.mark.parametrize("B,C,H,W,f,D", PATCH_CASES)
def test_patch_embed_and_expand(B, C, H, W, f, D):
    c = {k: v.to(DEV) for k, v in _patch_case(B, C, H, W, f, D).items()}
    rows_ref, img_ref, gref = _patch_oracle(B, C, H, W, f, D, torch.float64)
    _, _, gyard = _patch_oracle(B, C, H, W, f, D, torch.float32)
    what = "patch B%d C%d %dx%d f%d D%d" % (B, C, H, W, f, D)
    oh, ow = -(-H // f), -(-W // f)
    M = B * oh * ow

    def run():
        rows = cafa.patch_embed_forward(c["x"], c["w_e"], c["b_e"], f)
        dx, dwe, dbe = cafa.patch_embed_backward(c["x"], c["w_e"], c["g_rows"], f)
        img = cafa.patch_expand_forward(c["rows"], c["w_x"], c["b_x"], B, H, W, f)
        drows, dwx, dbx = cafa.patch_expand_backward(c["rows"], c["w_x"], c["g_img"], f)
        return rows, dx, dwe, dbe, img, drows, dwx, dbx

    first, second = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "not bitwise reproducible"
    rows, dx, dwe, dbe, img, drows, dwx, dbx = first
    assert tuple(rows.shape) == (M, D) and tuple(img.shape) == (B, C, H, W) and tuple(dx.shape) == (B, C, H, W)
    _check_forward(what + " embed", rows, rows_ref)
    _check_forward(what + " expand", img, img_ref)
    for key, got in (("x", dx), ("w_e", dwe), ("b_e", dbe), ("rows", drows), ("w_x", dwx), ("b_x", dbx)):
        assert got.shape == gref[key].shape
        _check_gradient(what + " d" + key, got, gref[key], gyard[key])

    # every output inside a NaN-filled allocation: its whole extent is written, nothing around it is
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = int(L.gw_patch_workspace_bytes(B, C, H, W, f, D))
    ws = torch.empty((ws_bytes // 4,), device=DEV)
    ld = D + 3  # rows with padding columns
    big_r, r_out = _guarded((M, ld))
    big_dx, dx_out = _guarded((B, C, H, W))
    big_dw, dw_out = _guarded((D, C, f, f))
    big_db, db_out = _guarded((D,))
    _lib.check(L.gw_patch_embed_forward(B, C, H, W, f, D, c["x"].data_ptr(), c["w_e"].data_ptr(), c["b_e"].data_ptr(), r_out.data_ptr(),
                                        ld, st), "gw_patch_embed_forward")
    _lib.check(L.gw_patch_embed_backward(B, C, H, W, f, D, c["x"].data_ptr(), c["w_e"].data_ptr(), c["g_rows"].data_ptr(), D,
                                         ws.data_ptr(), ws_bytes, dx_out.data_ptr(), dw_out.data_ptr(), db_out.data_ptr(), st),
               "gw_patch_embed_backward")
    torch.cuda.synchronize()
    assert torch.equal(r_out[:, :D], rows) and torch.isnan(r_out[:, D:]).all() and _guards_untouched(big_r)
    assert torch.equal(dx_out, dx) and torch.equal(dw_out, dwe) and torch.equal(db_out, dbe)
    assert _guards_untouched(big_dx) and _guards_untouched(big_dw) and _guards_untouched(big_db)
    big_i, i_out = _guarded((B, C, H, W))
    big_dr, dr_out = _guarded((M, ld))
    big_dw, dw_out = _guarded((D, C, f, f))
    big_db, db_out = _guarded((C,))
    _lib.check(L.gw_patch_expand_forward(B, C, H, W, f, D, c["rows"].data_ptr(), D, c["w_x"].data_ptr(), c["b_x"].data_ptr(),
                                         i_out.data_ptr(), st), "gw_patch_expand_forward")
    _lib.check(L.gw_patch_expand_backward(B, C, H, W, f, D, c["rows"].data_ptr(), D, c["w_x"].data_ptr(), c["g_img"].data_ptr(),
                                          ws.data_ptr(), ws_bytes, dr_out.data_ptr(), ld, dw_out.data_ptr(), db_out.data_ptr(), st),
               "gw_patch_expand_backward")
    torch.cuda.synchronize()
    assert torch.equal(i_out, img) and _guards_untouched(big_i)
    assert torch.equal(dr_out[:, :D], drows) and torch.isnan(dr_out[:, D:]).all() and _guards_untouched(big_dr)
    assert torch.equal(dw_out, dwx) and torch.equal(db_out, dbx) and _guards_untouched(big_dw) and _guards_untouched(big_db)


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_gradients(model, x, cfg, g, dtype):
    sd = co.params(model, dtype, requires_grad=True)
    t = x.to(dtype).clone().requires_grad_(True)
    out = co.forecaster(sd, t, cfg)
    (out * g.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["input"] = t.grad
    return out.detach(), grads


@pytest.mark.parametrize("name", list(co.CASES))
def test_model_parity_and_gradients(golden_dir, name):
    cfg, (b, h, w), _ = co.CASES[name]
    model, x = co.build(gw, name)
    golden = torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["out"])
    g = torch.from_numpy(np.random.RandomState(5).standard_normal(tuple(golden.shape)).astype(np.float32))
    ref, gref = _oracle_gradients(model, x, cfg, g, torch.float64)
    _, gyard = _oracle_gradients(model, x, cfg, g, torch.float32)
    model = model.to(DEV).train()  # dropout = 0: train() runs
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd)
    assert tuple(out.shape) == tuple(golden.shape) == (b, cfg["output_channels"], h, w)  # the input's spatial size, odd or not
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


def test_training_step_changes_every_parameter():
    model, x = co.build(gw, "cafa_f3_20x37")
    model = model.to(DEV).train()
    x = x.to(DEV)
    target = torch.from_numpy(np.random.RandomState(3).standard_normal((2, 4, 20, 37)).astype(np.float32)).to(DEV)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = gw.AdamW(model.parameters(), lr=1e-2)
    opt.zero_grad()
    loss = ((model(x) - target) ** 2).mean()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    print("cafa training loss %.5f" % float(loss))
    assert np.isfinite(float(loss))
    for k, v in model.named_parameters():
        assert torch.isfinite(v).all(), k
        assert not torch.equal(v, before[k]), k


def test_captured_forward_replays_bitwise():
    model, x = co.build(gw, "cafa_ref_33x65")
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


def test_standalone_classes_equal_the_row_path_bitwise():
    """CaFAEncoder / CaFAProcessor / CaFADecoder on NCHW against the forecaster's internal rows, same weights."""
    cfg, (b, h, w), _ = co.CASES["cafa_ref_32x64"]
    model, x = co.build(gw, "cafa_ref_32x64")
    model = model.to(DEV).eval()
    x = x.to(DEV)
    f = cfg["downsampling_factor"]
    oh, ow = h // f, w // f
    with torch.no_grad():
        rows = model.encoder.rows(x)
        image = model.encoder(x)  # [b, dim, oh, ow]
        assert tuple(image.shape) == (b, cfg["model_dim"], oh, ow)
        assert torch.equal(image.permute(0, 2, 3, 1).reshape(b * oh * ow, -1), rows)
        rows2 = model.processor.rows(rows, b, oh, ow)
        image2 = model.processor(image)
        assert torch.equal(image2.permute(0, 2, 3, 1).reshape(b * oh * ow, -1), rows2)
        out = model.decoder(image2)
        assert torch.equal(out, model(x))
        # the attention classes on b h w d
        grid = rows.reshape(b, oh, ow, -1)
        blk = model.processor.blocks[0]
        assert torch.equal(blk(grid).reshape(b * oh * ow, -1), blk.rows(rows, b, oh, ow))
        assert torch.equal(blk.attn(grid).reshape(b * oh * ow, -1), blk.attn.rows(rows, b, oh, ow))
        for axis in (1, 2):
            assert torch.equal(blk.attn.attn_height(grid, axis).reshape(b * oh * ow, -1),
                               blk.attn.attn_height.rows(rows, b, oh, ow, axis, None))
        # Conv2d drops a ragged edge where the forecaster pads: the stand-alone encoder on 33 x 65 is the encoder on 32 x 64
        xr = torch.cat([x, x[:, :, :1]], dim=2)
        xr = torch.cat([xr, xr[:, :, :, :1]], dim=3)
        assert torch.equal(model.encoder(xr), image)
