"""The ensemble-shared kernels (fan-out ConditionalLayerNorm, grouped gather, grouped segment sum) and the FGN model on the GPU.

Where the claim is "the same arithmetic" the test asks for bitwise equality: the fan-out forward against the grouped kernel on x
repeated per member, the grouped gather against the existing call on explicitly repeated tables, the grouped segment sum against
the existing entry at share = 1 and share = batch, default noise draws against the same vectors passed in, repeated training
steps, graph replay.  Everything else is measured against float64 restatements (tests/fgn_oracle.py) under the project's bar: the
yardstick is the float32 CPU restatement's own error against float64 on the same case, the kernels may err at most 4 x that, with
a floor of 1e-6 of the result's maximum.  The recorded outputs of the reference (tests/golden) are held to the same bar.  Every
figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from graph_weather_amd import fgn, gencast, wide
from graph_weather_amd.fgn import FunctionalGenerativeNetwork, _forward_member_loop

from . import fgn_oracle as fo
from . import gencast_model_oracle as mo
from .cafa_oracle import fill_, params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bar(what, got, ref64, yard32, factor=4.0):
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), what
    scale = ref64.abs().max().item()
    yard = (yard32.double().reshape(ref64.shape) - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    bar = max(factor * yard, 1e-6 * scale)
    print("%s: error %.3e, yardstick %.3e, bar %.3e (maximum %.3e), ratio %.2f" % (what, err, yard, bar, scale, err / max(yard, 1e-300)))
    assert err <= bar, (what, err, yard, bar)


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _strided(t, pad=3):
    """The same values on the device behind a row stride of width + pad."""
    wide_ = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    wide_[:, :t.shape[1]] = t.to(DEV)
    return wide_[:, :t.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# fan-out ConditionalLayerNorm
# ---------------------------------------------------------------------------------------------------------------------
_ACTS = {None: lambda t: t, "relu": F.relu, "silu": F.silu}


@pytest.mark.parametrize("act", [None, "relu", "silu"])
@pytest.mark.parametrize("width", [5, 16, 20, 130])  # 5 and 130 are no multiples of 4; 130 takes three columns per lane
def test_fanout_cond_layernorm(width, act):
    for B in (1, 3):
        for N in (1, 2, 3):
            for M in (1, 5, 300):  # 300 rows exceed one 256-row slab
                rs = np.random.RandomState(1000 * B + 100 * N + M + width)
                x, dout = _randn(rs, B * M, width), _randn(rs, B * N * M, width)
                scale, bias = 1.0 + 0.5 * _randn(rs, B * N, width), _randn(rs, B * N, width)

                def oracle(dtype):
                    xs, sc, bi = (t.to(dtype).clone().requires_grad_(True) for t in (x, scale, bias))
                    xh = F.layer_norm(xs, (width,), None, None, 1e-5).view(B, 1, M, width)
                    y = _ACTS[act](sc.view(B, N, 1, width) * xh + bi.view(B, N, 1, width)).reshape(B * N * M, width)
                    return [y.detach()] + list(torch.autograd.grad((y * dout.to(dtype)).sum(), (xs, sc, bi)))

                ref, yard = oracle(torch.float64), oracle(torch.float32)
                strided = (B + N + M) % 2 == 1  # half of the shapes read and write nothing but views with a row stride
                put = _strided if strided else (lambda t: t.to(DEV))
                xd, sd, bd, dd = put(x), put(scale), put(bias), put(dout)
                y = fgn.cond_layernorm_fanout_forward(xd, sd, bd, M, N, act)
                dx, dscale, dbias = fgn.cond_layernorm_fanout_backward(xd, sd, bd, M, N, act, dd)
                again = fgn.cond_layernorm_fanout_backward(xd, sd, bd, M, N, act, dd)
                x_rep = xd.reshape(B, 1, M, width).expand(B, N, M, width).reshape(B * N * M, width)
                y_grouped = gencast.cond_layernorm_grouped_forward(x_rep, sd, bd, M, act)
                torch.cuda.synchronize()
                what = "fan-out cln B %d N %d M %d width %d %s%s" % (B, N, M, width, act, " strided" if strided else "")
                assert y.shape == (B * N * M, width) and torch.equal(y, y_grouped), what  # bitwise the grouped kernel on repeated x
                assert all(torch.equal(a, b) for a, b in zip((dx, dscale, dbias), again)), what
                for name, got, r_, y_ in zip(("out", "dx", "dscale", "dbias"), (y, dx, dscale, dbias), ref, yard):
                    _bar("%s %s" % (what, name), got, r_, y_)


def test_fanout_cond_layernorm_more_than_64_members():
    """dx keeps the members' row sums in the lanes of the owning wave, 64 members per pass: 70 members take two passes."""
    B, N, M, width = 2, 70, 3, 20
    rs = np.random.RandomState(77)
    x, dout = _randn(rs, B * M, width), _randn(rs, B * N * M, width)
    scale, bias = 1.0 + 0.5 * _randn(rs, B * N, width), _randn(rs, B * N, width)

    def oracle(dtype):
        xs = x.to(dtype).clone().requires_grad_(True)
        xh = F.layer_norm(xs, (width,), None, None, 1e-5).view(B, 1, M, width)
        y = F.silu(scale.to(dtype).view(B, N, 1, width) * xh + bias.to(dtype).view(B, N, 1, width)).reshape(B * N * M, width)
        return torch.autograd.grad((y * dout.to(dtype)).sum(), xs)[0]

    dx = fgn.cond_layernorm_fanout_backward(x.to(DEV), scale.to(DEV), bias.to(DEV), M, N, "silu", dout.to(DEV))[0]
    _bar("fan-out cln 70 members dx", dx, oracle(torch.float64), oracle(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# grouped gather and grouped segment sum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "indexed"])
@pytest.mark.parametrize("k", [0, 9, 16], ids=["no_product", "k9_scalar", "k16_vec"])
@pytest.mark.parametrize("n", [20, 130])  # 130 columns cross one 128-column tile
def test_grouped_gather_equals_repeated_tables_bitwise(n, k, with_idx):
    B, N, R = 2, 3, 150  # 6 copies of 150 rows: 900 rows, more than one 128-row tile, copies that straddle tiles
    C = B * N
    T = 11 if with_idx else R  # table rows per block
    rs = np.random.RandomState(500 + n + k)
    idx = torch.from_numpy(rs.randint(0, T, R).astype(np.int32)).to(DEV) if with_idx else None
    per_copy, per_sample, per_all, per_all0 = _randn(rs, C * T, n).to(DEV), _strided(_randn(rs, B * T, n)), _randn(rs, T, n).to(DEV), \
        _randn(rs, T, n).to(DEV)
    x = _randn(rs, C * R, k).to(DEV) if k else None
    w = _randn(rs, n, k).to(DEV) if k else None
    bias = _randn(rs, n).to(DEV)
    sample_rep = per_sample.reshape(B, 1, T, n).expand(B, N, T, n).reshape(C * T, n).contiguous()
    all_rep = per_all.repeat(C, 1)
    for shares in (((per_copy, 1, T),), ((per_sample, N, T),), ((per_all, C, T),),
                   ((per_copy, 1, T), (per_sample, N, T), (per_all, C, T)), ((per_all0, 1, 0), (per_sample, N, T))):
        adds = [(t, idx, rows_pb, share) for t, share, rows_pb in shares]
        got = fgn.linear_gather_grouped_forward(x, w, bias, False, adds, C * R, R)
        rep = {id(per_copy): per_copy, id(per_sample): sample_rep, id(per_all): all_rep, id(per_all0): per_all0}
        want = wide.linear_gather_forward(x, w, bias, False, [(rep[id(t)], idx, rows_pb) for t, _, rows_pb in shares], C * R, R)
        torch.cuda.synchronize()
        assert got.shape == (C * R, n) and torch.isfinite(got).all() and torch.equal(got, want), [s[1:] for s in shares]
    # and the values themselves, once, against float64
    got = fgn.linear_gather_grouped_forward(x, w, bias, False, [(per_sample, idx, T, N)], C * R, R)
    rows = (idx.long().cpu() if with_idx else torch.arange(R))

    def oracle(dtype):
        t = per_sample.cpu().to(dtype).reshape(B, T, n)[:, rows].repeat_interleave(N, 0).reshape(C * R, n)
        prod = x.cpu().to(dtype) @ w.cpu().to(dtype).T if k else 0
        return prod + bias.cpu().to(dtype) + t

    _bar("grouped gather n %d k %d" % (n, k), got, oracle(torch.float64), oracle(torch.float32))


@pytest.mark.parametrize("width", [5, 20, 300])  # 300 columns take two 256-column blocks
def test_grouped_segment_sum(width):
    B, N, R, n_seg = 2, 3, 41, 9
    C = B * N
    rs = np.random.RandomState(600 + width)
    counts = np.array([0, 1, 9, 4, 0, 13, 5, 2, 7])  # empty segments, runs below and above the four-row unrolling
    assert counts.sum() == R and len(counts) == n_seg
    perm = torch.from_numpy(rs.permutation(R).astype(np.int32))
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    rows = _randn(rs, C * R, width)
    rd = _strided(rows)
    seg_of = torch.zeros(R, dtype=torch.int64)
    seg_of[perm.long()] = torch.repeat_interleave(torch.arange(n_seg), torch.from_numpy(counts))
    for share in (1, N, C):
        def oracle(dtype):
            per_copy = torch.zeros((C, n_seg, width), dtype=dtype).index_add_(1, seg_of, rows.to(dtype).view(C, R, width))
            return per_copy.view(C // share, share, n_seg, width).sum(1).reshape(-1, width)

        got = fgn.segment_sum_rows_grouped(rd, R, C, share, n_seg, ptr.to(DEV), perm.to(DEV))
        again = fgn.segment_sum_rows_grouped(rd, R, C, share, n_seg, ptr.to(DEV), perm.to(DEV))
        torch.cuda.synchronize()
        assert got.shape == (C // share * n_seg, width) and torch.equal(got, again)
        _bar("grouped segment sum width %d share %d" % (width, share), got, oracle(torch.float64), oracle(torch.float32))
        if share in (1, C):  # the existing entry's bits
            assert torch.equal(got, wide.segment_sum_rows(rd, R, C, C // share, n_seg, ptr.to(DEV), perm.to(DEV)))
    # identity (perm NULL): the gradient of a table read without an index
    ident = torch.arange(R + 1, dtype=torch.int32, device=DEV)
    got = fgn.segment_sum_rows_grouped(rd, R, C, N, R, ident, None)
    want64 = rows.double().view(B, N, R, width).sum(1).reshape(-1, width)
    _bar("grouped segment sum identity width %d" % width, got, want64, rows.view(B, N, R, width).sum(1).reshape(-1, width))


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}
CASE_NAMES = list(fo.CASES)


def _case(name, golden_dir):
    """(model on the device, input and noise on the CPU, loss weights, float64 and float32 restatements: output and gradients,
    the fixture), once."""
    if name in _MODELS:
        return _MODELS[name]
    _, kw, B, N, seed = fo.CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cpu = fill_(FunctionalGenerativeNetwork(**fo.case_kwargs(name)), seed)
    x, noise = fo.case_input(name), torch.from_numpy(g["noise"])
    # a loss that weights the members differently: member n's weights are scaled by 1 + n
    w = _randn(np.random.RandomState(seed + 100), B, N, cpu.num_lon, cpu.num_lat, cpu.output_features_dim)
    w = w * (1.0 + torch.arange(N, dtype=torch.float32)).view(1, N, 1, 1, 1)
    graphs = mo.graph_tables(cpu)

    def oracle(dtype):
        p = params(cpu, dtype, requires_grad=True)
        xt = x.to(dtype).clone().requires_grad_(True)
        out = fo.fgn_forward(p, kw, mo.cast_graphs(graphs, dtype), xt, noise.to(dtype))
        keys = list(p)
        grads = torch.autograd.grad((out * w.to(dtype)).sum(), [p[k] for k in keys] + [xt])
        return out.detach(), dict(zip(keys + ["previous_weather_state"], grads))

    _MODELS[name] = (cpu.to(DEV), (x, noise), w, oracle(torch.float64), oracle(torch.float32), g)
    return _MODELS[name]


def _run(model, fn, x, noise, w):
    xd = x.to(DEV).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    out = fn(xd, noise.to(DEV))
    (out * w.to(DEV)).sum().backward()
    grads = {k: v.grad for k, v in model.named_parameters()}
    grads.update(previous_weather_state=xd.grad)
    return out.detach(), grads


def _shared(model):
    return lambda x, noise: model(x, num_ensemble=noise.shape[1], noise_vectors=noise)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fgn_against_the_fixture_and_float64(golden_dir, name):
    model, (x, noise), w, (ref, gref), (yard, gyard), g = _case(name, golden_dir)
    _, kw, B, N, _ = fo.CASES[name]
    model.train()
    out, grads = _run(model, _shared(model), x, noise, w)
    torch.cuda.synchronize()
    assert out.shape == (B, N, model.num_lon, model.num_lat, model.output_features_dim) and out.dtype == torch.float32 and out.is_cuda
    _bar(name + " output", out, ref, yard)
    yard_err = (yard.double() - ref).abs().max().item()
    bar = max(4.0 * yard_err, 1e-6 * ref.abs().max().item())
    members = torch.from_numpy(g["members"]).double()
    fixture_err = (out.cpu().double() - members).abs().max().item()
    print("%s output against the reference's recorded members: %.3e (yardstick %.3e)" % (name, fixture_err, yard_err))
    assert fixture_err <= bar
    forward = torch.from_numpy(g["out"]).double()  # what the reference's forward returned: at B = 1 member 0 only
    kept = out.cpu().double()[:, :forward.shape[1]]
    print("%s output against the reference's forward %s: %.3e" % (name, tuple(forward.shape), (kept - forward).abs().max().item()))
    assert forward.shape[1] == (N if B > 1 else 1) and (kept - forward).abs().max().item() <= bar
    assert set(grads) == set(gref) and len(grads) == len(model.state_dict()) + 1
    for k in gref:
        assert grads[k] is not None, k
        _bar("%s d %s" % (name, k), grads[k], gref[k], gyard[k])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_member_loop_route_agrees(golden_dir, name):
    """The reference's route on this package's kernels, one member at a time: the same bar against float64; whether the two routes
    agree bitwise is reported."""
    model, (x, noise), w, (ref, gref), (yard, gyard), _ = _case(name, golden_dir)
    out, grads = _run(model, lambda a, b: _forward_member_loop(model, a, b), x, noise, w)
    out_s, grads_s = _run(model, _shared(model), x, noise, w)
    torch.cuda.synchronize()
    _bar(name + " member loop output", out, ref, yard)
    for k in gref:
        _bar("%s member loop d %s" % (name, k), grads[k], gref[k], gyard[k])
    same = [k for k in gref if torch.equal(grads[k], grads_s[k])]
    print("%s: shared route and member loop: outputs bitwise equal: %s (largest difference %.3e); gradients bitwise equal: %d of %d"
          % (name, torch.equal(out, out_s), (out - out_s).abs().max().item(), len(same), len(gref)))


@pytest.mark.parametrize("name", ["fgn_model_a", "fgn_model_c"])
def test_default_draws_equal_the_same_vectors_passed_in(golden_dir, name):
    model, (x, _), _, _, _, _ = _case(name, golden_dir)
    _, kw, B, N, _ = fo.CASES[name]
    model.eval()
    xd = x.to(DEV)
    with torch.no_grad():
        torch.manual_seed(5)
        drawn = model(xd, num_ensemble=N)
        torch.manual_seed(5)
        noise = torch.stack([torch.randn((B, kw["noise_dimension"]), device=DEV) for _ in range(N)], dim=1)
        given = model(xd, num_ensemble=N, noise_vectors=noise)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(9)
        drawn_g = model(xd, num_ensemble=N, generator=gen)
        gen.manual_seed(9)
        noise_g = torch.stack([torch.randn((B, kw["noise_dimension"]), device=DEV, generator=gen) for _ in range(N)], dim=1)
        given_g = model(xd, num_ensemble=N, noise_vectors=noise_g)
        three = model(xd, num_ensemble=3, noise_vectors=torch.cat([noise, noise_g[:, :1]], dim=1))
    torch.cuda.synchronize()
    assert torch.equal(drawn, given) and torch.equal(drawn_g, given_g) and not torch.equal(drawn, drawn_g)
    assert not torch.equal(drawn[:, 0], drawn[:, 1])  # the members differ
    assert torch.equal(three[:, :N], given) and torch.equal(three[:, N], given_g[:, 0])  # a member does not depend on the others


def test_training_step_is_bitwise_repeatable(golden_dir):
    model, (x, noise), w, _, _, _ = _case("fgn_model_a", golden_dir)
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def step():
        model.load_state_dict(state)
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        out, grads = _run(model, _shared(model), x, noise, w)
        opt.step()
        return [out] + [grads[k].clone() for k in sorted(grads)] + [v.detach().clone() for v in model.state_dict().values()]

    a, b = step(), step()
    torch.cuda.synchronize()
    model.load_state_dict(state)
    assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.isfinite(p).all() for p in a)


def test_eval_forward_replays_in_a_hip_graph(golden_dir):
    model, (x, noise), _, _, _, _ = _case("fgn_model_a", golden_dir)
    model.eval()
    xd, nd = x.to(DEV).clone(), noise.to(DEV).clone()
    with torch.no_grad():
        first = model(xd, num_ensemble=2, noise_vectors=nd)  # eager: sorts the edges once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = model(xd, num_ensemble=2, noise_vectors=nd)
    rs = np.random.RandomState(61)
    x2, n2 = _randn(rs, *x.shape).to(DEV), _randn(rs, *noise.shape).to(DEV)
    xd.copy_(x2), nd.copy_(n2)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = model(x2, num_ensemble=2, noise_vectors=n2)
    assert torch.equal(y, eager) and torch.isfinite(y).all() and not torch.equal(eager, first)


def test_shared_route_allocates_less_than_the_member_loop(golden_dir):
    """Case b (N = 3), forward + backward: the allocation peak of the shared route is strictly below the member loop's, which
    keeps the encoder's saved activations once per member."""
    model, (x, noise), w, _, _, _ = _case("fgn_model_b", golden_dir)
    assert noise.shape[1] == 3
    model.train()
    peaks = {}
    for route, fn in (("member loop", lambda a, b: _forward_member_loop(model, a, b)), ("shared", _shared(model))):
        _run(model, fn, x, noise, w)  # the plans exist before the measured call
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out, grads = _run(model, fn, x, noise, w)
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - base
        del out, grads
    model.zero_grad(set_to_none=True)
    print("forward + backward allocation peak above the resident model, B = 3, N = 3: shared %d, member loop %d"
          % (peaks["shared"], peaks["member loop"]))
    assert peaks["shared"] < peaks["member loop"]
