"""The GenCast kernels (csrc/gw_gencast.hip) and layers on the GPU against float64 restatements (tests/gencast_oracle.py).

Bar, the one of tests/test_gpu_aurora.py, applied to every output and every gradient here: the yardstick is the float32 CPU
restatement's own error against float64 on the same case, computed here; the kernels may err at most 4 x that, with a floor of
1e-6 of the result's maximum.  Every figure is printed before it is asserted.  Nothing compares the kernels with themselves,
except where bitwise equality is the claim (repeat runs, the training step, graph replay).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_weather_amd as gw
from graph_weather_amd import gencast

from . import gencast_oracle as go

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


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
# graph attention
# ---------------------------------------------------------------------------------------------------------------------
def _graph(rs, n_src, n_dst, deg):
    """Shuffled COO [2, E]: destination i has deg[i] incoming edges from sources drawn with replacement."""
    dst = np.repeat(np.arange(n_dst), deg)
    src = rs.randint(0, n_src, dst.size)
    order = rs.permutation(dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64)


def _graph37(rs):
    deg = np.arange(37) % 10  # in-degrees 0 ... 9
    deg[0], deg[1], deg[36] = 0, 1, 36  # forced
    return _graph(rs, 37, 37, deg)


def _graph_hub(rs):
    """70 nodes: destination 5 has 280 more in-edges (duplicates among them), source 9 has 280 more out-edges."""
    base = _graph(rs, 70, 70, np.arange(70) % 6)
    hub_in = np.stack([rs.randint(0, 70, 280), np.full(280, 5)])
    hub_out = np.stack([np.full(280, 9), rs.randint(0, 70, 280)])
    ei = np.concatenate([base, hub_in, hub_out], axis=1)
    return ei[:, rs.permutation(ei.shape[1])].astype(np.int64)


def _attention_case(what, ei, n_src, n_dst, H, C, with_e, mean, seed, q_scale=1.0, stacked=False):
    rs = np.random.RandomState(seed)
    hc, E = H * C, ei.shape[1]
    q, k, v = _randn(rs, n_dst, hc) * q_scale, _randn(rs, n_src, hc), _randn(rs, n_src, hc)
    e = _randn(rs, E, hc) if with_e else None
    dout = _randn(rs, n_dst, C if mean else hc)
    eit = torch.from_numpy(ei)

    def oracle(dtype):
        ts = [t.to(dtype).requires_grad_(True) for t in (q, k, v) + ((e,) if with_e else ())]
        out = go.graph_attention(ts[0], ts[1], ts[2], ts[3] if with_e else None, eit[0], eit[1], n_dst, H, mean)
        grads = torch.autograd.grad((out * dout.to(dtype)).sum(), ts)
        return [out.detach()] + list(grads)

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    if stacked:  # q, k, v as column blocks of one table: leading dimension 3 hc > width
        table = torch.cat([q, k, v], dim=1).to(DEV)
        qd, kd, vd = table[:, :hc], table[:, hc:2 * hc], table[:, 2 * hc:]
        assert qd.stride(0) == 3 * hc
    else:
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ed, dd = (e.to(DEV) if with_e else None), dout.to(DEV)
    plan = gencast.edge_plan(eit.to(DEV), n_src, n_dst).plan

    def ours():
        out, out_heads, lse = gencast.graph_attention_forward(qd, kd, vd, ed, plan, H, mean)
        return [out, lse] + list(gencast.graph_attention_backward(qd, kd, vd, ed, plan, H, mean, out_heads, lse, dd))

    a, b = ours(), ours()
    torch.cuda.synchronize()
    for x, y in zip(a, b):  # both launches of the backward, and the forward, run twice: bitwise equal
        assert (x is None and y is None) or torch.equal(x, y), what
    names = ["out", "dq", "dk", "dv"] + (["de"] if with_e else [])
    got = [a[0]] + a[2:5] + ([a[5]] if with_e else [])
    for nm, g_, r_, y_ in zip(names, got, ref, yard):
        _check("%s %s" % (what, nm), g_, r_, y_)
    return ref, eit


def test_attention_n37_h4_c128_edges():
    ei = _graph37(np.random.RandomState(1))
    ref, eit = _attention_case("N 37 H 4 C 128 with e", ei, 37, 37, 4, 128, True, False, 101)
    deg = torch.bincount(eit[1], minlength=37)
    assert int(deg[0]) == 0 and int(deg[1]) == 1 and int(deg[36]) == 36
    assert (ref[0][0] == 0).all() and (ref[1][0] == 0).all()  # the row without incoming edges: output and dq are zero


def test_attention_n37_h4_c128_plain_head_mean():
    _attention_case("N 37 H 4 C 128 head-mean", _graph37(np.random.RandomState(1)), 37, 37, 4, 128, False, True, 102)


def test_attention_n37_h4_c128_edges_head_mean():
    _attention_case("N 37 H 4 C 128 with e, head-mean", _graph37(np.random.RandomState(1)), 37, 37, 4, 128, True, True, 112)


def test_attention_hubs_and_duplicate_edges():
    ei = _graph_hub(np.random.RandomState(2))
    pairs = set()
    assert any((p in pairs) or pairs.add(p) for p in zip(ei[0].tolist(), ei[1].tolist()))  # duplicates are separate edges
    assert np.bincount(ei[1], minlength=70)[5] >= 280 and np.bincount(ei[0], minlength=70)[9] >= 280
    _attention_case("N 70 H 2 C 24 hubs", ei, 70, 70, 2, 24, True, False, 103)


def test_attention_scalar_path_stacked_table():
    _attention_case("N 23 H 3 C 7 scalar, stacked", _graph(np.random.RandomState(3), 23, 23, np.arange(23) % 8), 23, 23, 3, 7, True, False, 104,
                    stacked=True)
    _attention_case("N 23 H 3 C 7 scalar, stacked, head-mean", _graph(np.random.RandomState(3), 23, 23, np.arange(23) % 8), 23, 23, 3, 7,
                    False, True, 114, stacked=True)


@pytest.mark.parametrize("H,C,mean", [(2, 160, False), (2, 512, False), (2, 512, True), (1, 640, False), (1, 1028, False), (1, 2052, False), (2, 129, True),
                                      (1, 515, False)])
def test_attention_wide_heads(H, C, mean):
    """dim_head above 128, the last block's shape (head-mean of 512-wide heads), every fragment width and the long-row kernels
    (a dim_head above 2048; a scalar one above 512)."""
    ei = _graph(np.random.RandomState(4), 9, 9, np.array([0, 1, 2, 3, 4, 5, 6, 7, 9]))
    _attention_case("N 9 H %d C %d%s" % (H, C, " head-mean" if mean else ""), ei, 9, 9, H, C, C <= 512, mean, 105 + C)


def test_attention_bipartite():
    ei = _graph(np.random.RandomState(5), 11, 29, np.arange(29) % 5)
    _attention_case("n_src 11 n_dst 29", ei, 11, 29, 2, 8, True, False, 106)


def test_attention_scores_of_100():
    ei = _graph37(np.random.RandomState(7))
    rs = np.random.RandomState(107)  # (the first two draws of the case below)
    q, k = _randn(rs, 37, 16) * 50.0, _randn(rs, 37, 16)
    s = (q[ei[1]] * k[ei[0]]).sum(-1) / 4.0
    assert s.max() >= 100 and s.min() <= -100
    _attention_case("N 37 H 1 C 16 scores of 100", ei, 37, 37, 1, 16, False, False, 107, q_scale=50.0)


def test_attention_single_self_loop():
    _attention_case("N 1 self-loop", np.zeros((2, 1), dtype=np.int64), 1, 1, 2, 4, True, False, 108)


def test_attention_no_edges():
    plan = gencast.edge_plan(torch.zeros((2, 0), dtype=torch.int64, device=DEV), 5, 5).plan
    rs = np.random.RandomState(109)
    q, k, v, dout = (_randn(rs, 5, 8).to(DEV) for _ in range(4))
    e = torch.zeros((0, 8), device=DEV)
    out, out_heads, lse = gencast.graph_attention_forward(q, k, v, e, plan, 2, False)
    dq, dk, dv, de = gencast.graph_attention_backward(q, k, v, e, plan, 2, False, out_heads, lse, dout)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (5, 8) and tuple(de.shape) == (0, 8)
    assert (out == 0).all() and (dq == 0).all() and (dk == 0).all() and (dv == 0).all()


def test_attention_refuses_oversized_rows():
    plan = gencast.edge_plan(torch.zeros((2, 1), dtype=torch.int64, device=DEV), 1, 1).plan
    x = torch.zeros((1, 4100), device=DEV)
    with pytest.raises(NotImplementedError, match="heads \\* dim_head <= 4096"):
        gencast.graph_attention_forward(x, x, x, None, plan, 1, False)


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
def _act64(name):
    return {None: (lambda z: z), "relu": F.relu, "silu": F.silu}[name]


def _cond_ln_case(what, x, scale, bias, dout, act):
    def oracle(dtype):
        ts = [t.to(dtype).requires_grad_(True) for t in (x, scale, bias)]
        out = _act64(act)(ts[1] * F.layer_norm(ts[0], (x.shape[1],), None, None, 1e-5) + ts[2])
        return [out.detach()] + list(torch.autograd.grad((out * dout.to(dtype)).sum(), ts))

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    xd, sd, bd, dd = x.to(DEV), scale.to(DEV), bias.to(DEV), dout.to(DEV)
    got = [gencast.cond_layernorm_forward(xd, sd, bd, act)] + list(gencast.cond_layernorm_backward(xd, sd, bd, act, dd))
    for nm, g_, r_, y_ in zip(("out", "dx", "dscale", "dbias"), got, ref, yard):
        _check("%s %s" % (what, nm), g_, r_, y_)


@pytest.mark.parametrize("width", [512, 24, 7, 2048])
@pytest.mark.parametrize("rows", [1, 37, 300])
def test_cond_layernorm(width, rows):
    rs = np.random.RandomState(width + rows)
    x, scale, bias, dout = _randn(rs, rows, width) * 2.0 + 0.5, 1.0 + 0.5 * _randn(rs, rows, width), _randn(rs, rows, width), _randn(rs, rows, width)
    for act in (None, "relu", "silu"):
        _cond_ln_case("cond-LN %d x %d %s" % (rows, width, act), x, scale, bias, dout, act)


@pytest.mark.parametrize("width", [24, 512])
def test_cond_layernorm_constant_row(width):
    """A row of equal values: variance 0, the normalised row is exactly 0 and the output is act(bias)."""
    rs = np.random.RandomState(width)
    x = torch.full((2, width), 3.0)
    scale, bias, dout = 1.0 + 0.5 * _randn(rs, 2, width), _randn(rs, 2, width), _randn(rs, 2, width)
    _cond_ln_case("cond-LN constant rows, width %d" % width, x, scale, bias, dout, "silu")
    out = gencast.cond_layernorm_forward(x.to(DEV), scale.to(DEV), bias.to(DEV), None)
    assert torch.equal(out.cpu(), bias)


@pytest.mark.parametrize("width", [512, 24, 7, 2048])
@pytest.mark.parametrize("rows", [1, 37, 300])
def test_beta_gate(width, rows):
    rs = np.random.RandomState(1000 + width + rows)
    o, xr, dy = _randn(rs, rows, width), _randn(rs, rows, width), _randn(rs, rows, width)
    w = _randn(rs, 1, 3 * width) / np.sqrt(3.0 * width)

    def oracle(dtype):
        ts = [t.to(dtype).requires_grad_(True) for t in (o, xr, w)]
        g = (torch.cat([ts[0], ts[1], ts[0] - ts[1]], dim=-1) @ ts[2].T).sigmoid()
        y = g * ts[1] + (1 - g) * ts[0]
        return [y.detach()] + list(torch.autograd.grad((y * dy.to(dtype)).sum(), ts))

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    od, xd, wd, dd = o.to(DEV), xr.to(DEV), w.to(DEV), dy.to(DEV)
    y, gate = gencast.beta_gate_forward(od, xd, wd)
    a, b = gencast.beta_gate_backward(od, xd, wd, gate, dd), gencast.beta_gate_backward(od, xd, wd, gate, dd)
    assert all(torch.equal(p_, q_) for p_, q_ in zip(a, b))
    assert tuple(a[2].shape) == (1, 3 * width)
    for nm, g_, r_, y_ in zip(("y", "d_out", "d_x_r", "dw"), [y] + list(a), ref, yard):
        _check("gate %d x %d %s" % (rows, width, nm), g_, r_, y_)


@pytest.mark.parametrize("n", [1, 1027])
def test_silu(n):
    rs = np.random.RandomState(n)
    x = torch.from_numpy(rs.uniform(-30.0, 30.0, n).astype(np.float32))
    x[0] = 30.0
    if n > 1:
        x[1] = -30.0
    dy = _randn(rs, n)

    def oracle(dtype):
        t = x.to(dtype).requires_grad_(True)
        y = F.silu(t)
        return y.detach(), torch.autograd.grad((y * dy.to(dtype)).sum(), t)[0]

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    xd = x.to(DEV)
    _check("silu n %d y" % n, gencast.silu_forward(xd), ref[0], yard[0])
    _check("silu n %d dx" % n, gencast.silu_backward(xd, dy.to(DEV)), ref[1], yard[1])


def test_fourier_features():
    rs = np.random.RandomState(32)
    rows, nf = 41, 32
    t = torch.from_numpy(rs.uniform(-2.0, 2.0, (rows, 1)).astype(np.float32))
    t[0, 0], t[1, 0] = -2.0, 2.0
    dout = _randn(rs, rows, 2 * nf)

    def oracle(dtype):
        tt = t.to(dtype).requires_grad_(True)
        out = go.fourier_features(tt, nf, 16)
        return out.detach(), torch.autograd.grad((out * dout.to(dtype)).sum(), tt)[0]

    ref, yard = oracle(torch.float64), oracle(torch.float32)
    td = t.to(DEV)
    _check("fourier F 32 out", gencast.fourier_forward(td, nf, 16), ref[0], yard[0])
    _check("fourier F 32 dt", gencast.fourier_backward(td, dout.to(DEV), nf, 16), ref[1], yard[1])


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def _module_case(what, kind, cfg, inp, seed):
    """Outputs and the gradient of every parameter and every float input against the float64 restatement."""
    module = go.build_kind(gencast, kind, cfg, seed)
    rs = np.random.RandomState(seed + 500)
    keys = [k for k, _ in module.named_parameters()]
    float_in = [k for k, v in inp.items() if v.dtype != torch.int64]
    weights = None

    def oracle(dtype):
        nonlocal weights
        p = go.params(module, dtype, requires_grad=True)
        ci = go.cast(inp, dtype, True)
        outs = go.run_kind(kind, cfg, p, ci)
        if weights is None:
            weights = [_randn(rs, *o.shape) for o in outs]
        loss = sum((o * w.to(dtype)).sum() for o, w in zip(outs, weights))
        wrt = [p[k] for k in keys] + [ci[k] for k in float_in]
        grads = torch.autograd.grad(loss, wrt, allow_unused=True)
        return [o.detach() for o in outs], [torch.zeros_like(t) if g is None else g for g, t in zip(grads, wrt)]

    (ref, gref), (yard, gyard) = oracle(torch.float64), oracle(torch.float32)
    module = module.to(DEV)
    di = {k: (v.to(DEV) if v.dtype == torch.int64 else v.to(DEV).requires_grad_(True)) for k, v in inp.items()}
    outs = go.call_kind(module, kind, di)
    torch.autograd.backward(outs, [w.to(DEV) for w in weights])
    for i, (o, r_, y_) in enumerate(zip(outs, ref, yard)):
        _check("%s output %d" % (what, i), o, r_, y_)
    got = [dict(module.named_parameters())[k].grad for k in keys] + [di[k].grad for k in float_in]
    for nm, g_, r_, y_ in zip(keys + float_in, got, gref, gyard):
        assert g_ is not None, nm
        if nm.endswith("transformer_conv.lin_key.bias"):
            _check_key_bias("%s d %s" % (what, nm), g_, r_, y_, gref[keys.index(nm[:-4] + "weight")])
        else:
            _check("%s d %s" % (what, nm), g_, r_, y_)
    return module


def _check_key_bias(what, got, ref64, yard32, weight_grad64):
    """The key bias adds the same q_i . b to every score of destination i, which the softmax ignores: its true gradient is zero
    and the float64, float32 and kernel values are all rounding residue of sum_j dk_j, whose terms cancel.  "1e-6 of the result's
    maximum" would be 1e-6 of that residue, and 4 x the float32 residue is one noise draw against another; the floor is
    therefore taken from the maximum of the same product's other output, d lin_key.weight (= dk^T x, with bias gradient = dk^T 1)."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), what
    yard = (yard32.double().reshape(ref64.shape) - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    bar = max(4.0 * yard, 1e-6 * weight_grad64.abs().max().item())
    print("%s: error %.3e, yardstick %.3e, bar %.3e (true value 0; maximum of d weight %.3e)" % (what, err, yard, bar, weight_grad64.abs().max().item()))
    assert err <= bar, (what, err, yard, bar)


@pytest.mark.parametrize("name", list(go.CASES))
def test_golden_cases_against_float64(name):
    kind, cfg, _, seed = go.CASES[name]
    _module_case(name, kind, cfg, go.case_inputs(name), seed)


def test_encoder_without_layer_norm_relu_and_a_receiver_without_edges():
    cfg = dict(grid_dim=7, mesh_dim=3, edge_dim=4, hidden_dims=[40, 24], use_layer_norm=False)
    inp = go.case_inputs("gencast_encoder")
    inp["edge_index"][1] %= 9  # mesh rows 9, 10, 11 receive nothing
    assert int(torch.bincount(inp["edge_index"][1], minlength=12)[9:].sum()) == 0
    module = _module_case("encoder no LN, ReLU", "encoder", cfg, inp, 31)
    assert module.grid_mlp.norm_layer is None and isinstance(module.grid_mlp.activation, torch.nn.ReLU)


def test_interaction_network_receiver_without_edges_gets_zeros():
    net = go.fill_(gencast.InteractionNetwork(5, 6, 3, [9, 8], use_layer_norm=True, scale_factor=0.5), 32).to(DEV)
    rs = np.random.RandomState(33)
    xs, xr, ea = _randn(rs, 7, 5), _randn(rs, 4, 6), _randn(rs, 10, 3)
    ei = torch.from_numpy(np.stack([rs.randint(0, 7, 10), rs.randint(0, 3, 10)]).astype(np.int64))  # receiver 3 has no edge

    def oracle(dtype):
        p = {"n." + k: v for k, v in go.params(net, dtype).items()}
        return go.interaction(p, "n", xs.to(dtype), xr.to(dtype), ei, ea.to(dtype), "ReLU", 0.5)

    out = net((xs.to(DEV), xr.to(DEV)), ei.to(DEV), ea.to(DEV))
    _check("interaction network", out, oracle(torch.float64), oracle(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _train_step():
    torch.manual_seed(0)
    enc = go.build(gencast, "gencast_encoder").to(DEV)
    proc = go.build_kind(gencast, "processor", dict(latent_dim=24, hidden_dims=[40, 24], num_blocks=2, num_heads=4, num_frequencies=8,
                                                    base_period=16, noise_emb_dim=12, edges_dim=4), 41).to(DEV)
    dec = go.build_kind(gencast, "decoder", dict(edges_dim=4, output_dim=5, hidden_dims=[40, 24], activation_layer="SiLU"), 42).to(DEV)
    inp = {k: v.to(DEV) for k, v in go.case_inputs("gencast_encoder").items()}
    rs = np.random.RandomState(43)
    mesh_ei = torch.from_numpy(go.random_graph(rs, 12, 5)).to(DEV)
    mesh_ea = _randn(rs, mesh_ei.shape[1], 4).to(DEV)
    noise = torch.full((12, 1), 0.7, device=DEV)
    m2g = torch.stack([inp["edge_index"][1], inp["edge_index"][0]])
    params = [p for m in (enc, proc, dec) for p in m.parameters()]
    opt = gw.AdamW(params, lr=1e-3)
    grid, mesh = enc(inp["grid"], inp["mesh"], inp["edge_attr"], inp["edge_index"])
    mesh = proc(mesh, mesh_ei, noise, mesh_ea)
    out = dec(mesh, grid, inp["edge_attr"], m2g)
    torch.autograd.backward(out, torch.ones_like(out) / out.numel())
    opt.step()
    torch.cuda.synchronize()
    return [out.detach().clone()] + [p.detach().clone() for p in params] + [p.grad.detach().clone() for p in params]


def test_training_step_is_bitwise_reproducible():
    a, b = _train_step(), _train_step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.isfinite(x).all() for x in a)


def test_processor_forward_replays_in_a_hip_graph():
    name = "gencast_processor_edges"
    proc = go.build(gencast, name).to(DEV).eval()
    inp = {k: v.to(DEV) for k, v in go.case_inputs(name).items()}
    x, noise = inp["x"].clone(), inp["noise_levels"].clone()
    with torch.no_grad():
        proc(x, inp["edge_index"], noise, inp["edge_attr"])  # eager: sorts the edges once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = proc(x, inp["edge_index"], noise, inp["edge_attr"])
    rs = np.random.RandomState(51)
    x2, noise2 = _randn(rs, *x.shape).to(DEV), (noise + 0.25)
    x.copy_(x2)
    noise.copy_(noise2)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = proc(x2, inp["edge_index"], noise2, inp["edge_attr"])
    assert torch.equal(y, eager) and torch.isfinite(y).all()
    assert not torch.equal(eager, proc(inp["x"], inp["edge_index"], inp["noise_levels"], inp["edge_attr"]).detach())
