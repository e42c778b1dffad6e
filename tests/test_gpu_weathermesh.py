"""WeatherMesh's processor on the GPU: the neighbourhood attention kernels of csrc/gw_na3d.hip, ``NeighborhoodAttention3D`` and
``WeatherMeshProcessor`` against float64 restatements (tests/weathermesh_oracle.py), a closed form that needs no oracle, and the
outputs recorded from the reference's own class (tests/golden/weathermesh_processor_*.npz).

Bar, the project's standing one: the yardstick is the float32 CPU restatement's own error against float64 on the same case,
computed here (for the recorded cases: the recorded float32 output's); the kernels may err at most 4 x that, with a floor of 1e-6
of the result's maximum; the yardstick itself must be within 1e-3 of that maximum, so the bar cannot hide a failure.  Every figure
is printed before it is asserted, and the worst ratio to the yardstick is printed by the last test.
"""
import os

import numpy as np
import pytest
import torch

from graph_weather_amd import weathermesh

from . import weathermesh_oracle as wo
from .cafa_oracle import fill_, params

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


# ---------------------------------------------------------------------------------------------------------------------
# the attention kernels
# ---------------------------------------------------------------------------------------------------------------------
def _na_case(what, shape, kernel, nh, dh, seed, strided=False, dense=False):
    """out, dq, dk, dv of the kernels from a random dout against the float64 restatement; every launch twice, bitwise equal."""
    B, D, H, W = shape
    rows, C, scale = B * D * H * W, nh * dh, dh ** -0.5
    rs = np.random.RandomState(seed)
    q, k, v, dout = (_randn(rs, rows, C) for _ in range(4))

    def oracle(dtype, fn=wo.na3d):
        ts = [t.to(dtype).requires_grad_(True) for t in (q, k, v)]
        vol = [t.view(B, D, H, W, nh, dh) for t in ts]
        out = (fn(*vol, kernel, scale) if fn is wo.na3d else fn(*vol, scale)).reshape(rows, C)
        return [out.detach()] + list(torch.autograd.grad((out * dout.to(dtype)).sum(), ts))

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    if dense:  # every window is the whole volume: plain softmax attention over all tokens
        for a, b in zip(ref, oracle(torch.float64, wo.dense_attention)):
            assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())
    if strided is True:  # q, k, v as column blocks of a wider table, dout as a column block of another: leading dimensions above the width
        table = torch.cat([q, k, v, torch.zeros(rows, 4)], dim=1).to(DEV)
        qd, kd, vd = table[:, :C], table[:, C:2 * C], table[:, 2 * C:3 * C]
        dd = torch.cat([torch.zeros(rows, C), dout], dim=1).to(DEV)[:, C:]
        assert qd.stride(0) == 3 * C + 4 and dd.stride(0) == 2 * C and not dd.is_contiguous()
    elif strided == "odd":  # [rows, 3 C + 1]: no leading dimension a multiple of 4, no table 16-byte aligned
        table = torch.cat([torch.zeros(rows, 1), q, k, v], dim=1).to(DEV)
        qd, kd, vd, dd = table[:, 1:1 + C], table[:, 1 + C:1 + 2 * C], table[:, 1 + 2 * C:], dout.to(DEV)
        assert qd.stride(0) == 3 * C + 1 and qd.data_ptr() % 16 == 4
    else:
        qd, kd, vd, dd = q.to(DEV), k.to(DEV), v.to(DEV), dout.to(DEV)

    def ours():
        out, lse = weathermesh.na3d_forward(qd, kd, vd, shape, kernel, nh, scale)
        return [out, lse] + list(weathermesh.na3d_backward(qd, kd, vd, shape, kernel, nh, scale, out, lse, dd))

    a, b = ours(), ours()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), what
    stacked = weathermesh.na3d_backward(qd, kd, vd, shape, kernel, nh, scale, a[0], a[1], dd, stacked=True)
    assert stacked[3].shape == (rows, 3 * C) and all(torch.equal(x, y) for x, y in zip(stacked[:3], a[2:5]))
    for nm, g_, r_, y_ in zip(("out", "dq", "dk", "dv"), [a[0]] + a[2:5], ref, yard):
        _bar("%s %s" % (what, nm), g_, r_, y_)
    return ref


# (B, D, H, W), kernel, heads, head_dim
NA_CASES = [
    ((2, 4, 5, 6), (3, 3, 5), 2, 8),      # axis lengths k + 1, k + 2, k + 1: the long inverse ranges
    ((1, 7, 9, 11), (5, 7, 7), 8, 4),     # the default kernel at length k + 2 on every axis
    ((1, 6, 17, 33), (3, 5, 5), 1, 4),    # two and four tiles plus one row / column
    ((1, 3, 9, 9), (3, 5, 7), 2, 8),      # H and W the tile size plus one
    ((1, 2, 3, 40), (1, 3, 7), 3, 6),     # heads do not divide 64, head_dim no multiple of 4, a kernel of 1: the general path
    ((1, 5, 8, 8), (5, 7, 7), 2, 64),     # the widest head of the tiled path
    ((1, 5, 8, 8), (5, 7, 7), 1, 128),    # above it: the general path
    ((1, 3, 20, 12), (3, 7, 7), 2, 32),   # a last-but-one tile whose keys are seen from the far border: the longest key-side halo
]


@pytest.mark.parametrize("shape,kernel,nh,dh", NA_CASES)
def test_kernels_against_float64(shape, kernel, nh, dh):
    _na_case("%s kernel %s heads %d x %d" % (shape, kernel, nh, dh), shape, kernel, nh, dh, 100 + nh * dh + sum(shape))


def test_whole_volume_window_is_dense_attention():
    _na_case("(1, 3, 3, 3) kernel (3, 3, 3) heads 1 x 4", (1, 3, 3, 3), (3, 3, 3), 1, 4, 7, dense=True)


@pytest.mark.parametrize("shape,kernel,nh,dh", [((2, 4, 9, 10), (3, 5, 5), 2, 8), ((1, 3, 4, 9), (3, 3, 5), 3, 6)])
def test_strided_tables_and_a_non_contiguous_dout(shape, kernel, nh, dh):
    _na_case("strided %s kernel %s heads %d x %d" % (shape, kernel, nh, dh), shape, kernel, nh, dh, 55, strided=True)


def test_unaligned_rows_take_the_general_path():
    """A leading dimension that is no multiple of 4 and tables that start 4 bytes past a 16-byte boundary."""
    _na_case("unaligned (1, 3, 5, 6) kernel (3, 3, 5) heads 2 x 8", (1, 3, 5, 6), (3, 3, 5), 2, 8, 56, strided="odd")


def test_closed_form_uniform_softmax_returns_the_window_centre():
    """q = 0 makes the softmax uniform; v carries the token's own (d, h, w), so the output is the mean coordinate of the window:
    start + (k - 1) / 2 per axis - what inward-shifted windows give, and neither zero padding nor truncation does."""
    B, D, H, W = shape = (1, 6, 9, 10)
    kernel = (3, 5, 7)
    grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"), dim=-1).float()
    v = torch.cat([grid, torch.zeros(D, H, W, 1)], dim=-1).reshape(-1, 4)
    rs = np.random.RandomState(5)
    k = _randn(rs, D * H * W, 4)
    out, _ = weathermesh.na3d_forward(torch.zeros(D * H * W, 4, device=DEV), k.to(DEV), v.to(DEV), shape, kernel, 1, 0.5)
    want = torch.zeros(D, H, W, 4)
    for axis, (L, kk) in enumerate(zip((D, H, W), kernel)):
        centre = torch.tensor([min(max(i - kk // 2, 0), L - kk) + (kk - 1) / 2 for i in range(L)])
        want[..., axis] = centre.view([-1 if a == axis else 1 for a in range(3)])
    err = (out.cpu().view(D, H, W, 4) - want).abs().max().item()
    print("closed form: largest error %.3e" % err)
    assert want[0, 0, 0].tolist() == [1.0, 2.0, 3.0, 0.0] and want[-1, -1, -1].tolist() == [4.0, 6.0, 6.0, 0.0]
    assert err <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wo.CASES))
def test_recorded_outputs_of_the_reference_class(name):
    kw, shape, seed = wo.CASES[name]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert int(g["seed"]) == seed
    module = fill_(weathermesh.WeatherMeshProcessor(**kw), seed).to(DEV)
    x = wo.case_input(name)
    full = dict(n_layers=10, kernel=(5, 7, 7), num_heads=8)
    full.update({k: v for k, v in kw.items() if k != "latent_dim"})
    ref = wo.processor_forward(params(module), x.double(), full["n_layers"], full["kernel"], full["num_heads"])
    for mode, key in (("eval", "out"), ("train", "train_out")):
        getattr(module, mode)()
        with torch.no_grad():
            out = module(x.to(DEV))
        assert tuple(out.shape) == tuple(shape)
        _bar("%s %s" % (name, mode), out, ref, torch.from_numpy(g[key]))


def _train_setup():
    shape, kw = (1, 4, 6, 7, 16), dict(latent_dim=16, n_layers=2, kernel=(3, 3, 5), num_heads=2)
    rs = np.random.RandomState(21)
    return shape, kw, _randn(rs, *shape), _randn(rs, *shape) / 16


def _train_oracle(dtype, steps):
    """(outputs per step, gradients of step 1) of the restatement trained on the CPU in ``dtype``."""
    shape, kw, x, w = _train_setup()
    p = {k: v.to(dtype).requires_grad_(True) for k, v in params(fill_(weathermesh.WeatherMeshProcessor(**kw), 9)).items()}
    opt = torch.optim.AdamW(list(p.values()), lr=1e-3, eps=1e-3)
    outs, grads = [], None
    for _ in range(steps):
        opt.zero_grad()
        out = wo.processor_forward(p, x.to(dtype), kw["n_layers"], kw["kernel"], kw["num_heads"])
        (out * w.to(dtype)).sum().backward()
        if grads is None:
            grads = {k: v.grad.detach().clone() for k, v in p.items()}
        opt.step()
        outs.append(out.detach())
    return outs, grads


def test_three_adamw_steps_against_float64():
    """eps = 1e-3 keeps AdamW's update a smooth function of gradients that are zero in exact arithmetic (the key bias's: a shift of
    every key moves no softmax), so rounding noise in them is not amplified to steps of the size of the learning rate."""
    shape, kw, x, w = _train_setup()
    (ref, gref), (yard, gyard) = _train_oracle(torch.float64, 3), _train_oracle(torch.float32, 3)
    module = fill_(weathermesh.WeatherMeshProcessor(**kw), 9).to(DEV).train()
    opt = torch.optim.AdamW(module.parameters(), lr=1e-3, eps=1e-3)
    xd, wd = x.to(DEV), w.to(DEV)
    for step in range(3):
        opt.zero_grad()
        out = module(xd)
        (out * wd).sum().backward()
        if step == 0:
            for k, prm in module.named_parameters():
                assert prm.grad is not None, k
                _bar("training step 1 d %s" % k, prm.grad, gref[k], gyard[k])
        opt.step()
        _bar("training step %d output" % (step + 1), out, ref[step], yard[step])
    assert (ref[2] - ref[0]).abs().max().item() > 1e-3  # the steps moved the output by far more than the bar


def test_forward_and_backward_twice_are_bitwise_equal():
    module = fill_(weathermesh.WeatherMeshProcessor(latent_dim=32, n_layers=2, kernel=(3, 5, 5), num_heads=4), 4).to(DEV)
    x = _randn(np.random.RandomState(8), 2, 4, 9, 10, 32).to(DEV)

    def run():
        module.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        out = module(xi)
        out.square().sum().backward()
        return [out.detach(), xi.grad] + [p.grad.clone() for p in module.parameters()]

    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and all(torch.isfinite(t).all() for t in a)
    assert a[1].abs().max().item() > 0


def test_nothing_of_size_tokens_x_window_is_allocated():
    """Forward and backward of the attention allocate out [rows, C], the two planes [2, rows heads], the stacked gradient
    [rows, 3 C] and delta [rows heads] - the bound below, plus 512 bytes of allocator rounding per tensor - and nothing that grows
    with the window: one score per (token, key, head) would be 245 x the planes."""
    shape, kernel, nh, dh = (1, 6, 16, 16), (5, 7, 7), 4, 8
    rows, C = 6 * 16 * 16, nh * dh
    rs = np.random.RandomState(2)
    qkv, dout = _randn(rs, rows, 3 * C).to(DEV), _randn(rs, rows, C).to(DEV)
    views = (qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:])
    out, lse = weathermesh.na3d_forward(*views, shape, kernel, nh, dh ** -0.5)  # warm: the library is loaded
    del out, lse
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, lse = weathermesh.na3d_forward(*views, shape, kernel, nh, dh ** -0.5)
    grads = weathermesh.na3d_backward(*views, shape, kernel, nh, dh ** -0.5, out, lse, dout, stacked=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = 4 * (rows * C + 2 * rows * nh + 3 * rows * C + rows * nh) + 4 * 512
    scores = 4 * rows * 245 * nh
    print("attention forward + backward: peak %d bytes, bound %d, one score per (token, key, head) %d" % (peak, bound, scores))
    assert grads[3].shape == (rows, 3 * C)
    assert peak <= bound < scores / 4


def test_zz_worst_ratio():
    print("worst ratio to the float32 CPU yardstick: %.2f (%s)" % (WORST["ratio"], WORST["what"]))
    assert WORST["ratio"] <= 4.0
