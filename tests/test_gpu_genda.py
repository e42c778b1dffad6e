"""GenDA on the GPU: the two row kernels of csrc/gw_genda.hip, the model's ``forward`` and one-pass ``guided_forward``, the
replicated route, the training-time conditioning dropout, training steps, graph replay and the guided Sampler run.

Where the claim is "the same arithmetic" the test asks for bitwise equality: the input rows against the torch expression of the same
float32 operations and against the Denoiser's ``precond_input_forward``, the two copies of a guided pass against one-copy calls,
repeated calls, repeated training steps, graph replay, a dropout hit against zero conditioning.  Everything else is measured against
float64 (tests/genda_oracle.py, or float64 autograd of the expression) under the project's bar: the yardstick is the float32 CPU
restatement's own error against float64 on the same inputs, the kernels may err at most 4 x that, with a floor of 1e-6 of the
result's maximum.  The recorded outputs of the reference (tests/golden) are held to the same bar.  Every figure is printed before it
is asserted.
"""
import os

import numpy as np
import pytest
import torch

from graph_weather_amd import gencast, genda
from graph_weather_amd.genda import GenDA, _forward_replicated
from graph_weather_amd.gencast_sampler import Sampler

from . import genda_oracle as do
from . import gencast_model_oracle as mo
from . import gencast_sampler_oracle as so
from .cafa_oracle import fill_, params
from .test_gpu_gencast_model import _bar, _randn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIGMAS = {1: (0.5,), 3: (0.08, 1.0, 40.0)}  # the noise levels of the model cases
ROWS = (1, 5, 84)  # 84 grid rows: 21 workgroups of four rows per sample; 1 and 5: a workgroup that spans samples and is not full


def _strided(t, pad=3):
    """The same values on the device behind a row stride of width + pad."""
    wide_ = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    wide_[:, :t.shape[1]] = t.to(DEV)
    return wide_[:, :t.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# the input kernel
# ---------------------------------------------------------------------------------------------------------------------
def _input_rows(dtype, z, x, sigma, stat, cols, copies, drop, G):
    """The rows the kernel writes, as torch operations in ``dtype`` in the reference's order: [copies B G, wz + wx + n_cond + ws]."""
    B = sigma.shape[0]
    c_in = (1 / torch.sqrt(sigma ** 2 + 1.0 ** 2)).repeat_interleave(G, 0)
    head, tail = [c_in * z, x], [stat.repeat(B, 1)]
    out = [torch.cat(head + [c * 0.0 if drop else c for c in cols] + tail, dim=-1)]
    if copies == 2:
        out.append(torch.cat(head + [c * 0.0 for c in cols] + tail, dim=-1))
    return torch.cat(out, dim=0)


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("wz,wx,cond,ws", [(5, 6, 2, 3), (2, 6, 2, 3), (4, 8, 0, 4), (1, 0, 1, 0)])
def test_input_kernel(wz, wx, cond, ws, copies, drop):
    for B in (1, 3):
        for G in ROWS:
            rs = np.random.RandomState(1000 * B + 10 * G + wz + 7 * copies + drop)
            z, x, stat = _randn(rs, B * G, wz), _randn(rs, B * G, wx), _randn(rs, G, ws)
            sensors = _randn(rs, B * G, 5)  # mask and values are columns 1 and 3 of a wider tensor
            dout = _randn(rs, copies * B * G, wz + wx + cond + ws)
            sigma = torch.tensor(SIGMAS[B], dtype=torch.float32)[:, None]
            # one conditioning column: the mask alone at B = 1, the values alone at B = 3
            slots = {2: (1, 3), 0: (None, None), 1: ((1, None) if B == 1 else (None, 3))}[cond]
            given = [s for s in slots if s is not None]
            strided = (B + G + wz + copies + drop) % 2 == 1  # half of the cases read nothing but views with a row stride
            what = "input kernel B %d G %d widths %s copies %d drop %d%s" % (B, G, (wz, wx, cond, ws), copies, drop,
                                                                               " strided" if strided else "")

            def oracle(dtype):
                zt, xt = (t.to(dtype).clone().requires_grad_(True) for t in (z, x))
                cols = [sensors[:, s:s + 1].to(dtype).clone().requires_grad_(True) for s in given]
                rows = _input_rows(dtype, zt, xt, sigma.to(dtype), stat.to(dtype), cols, copies, drop, G)
                grads = torch.autograd.grad((rows * dout.to(dtype)).sum(), [zt, xt] + cols, allow_unused=True)
                return rows.detach(), [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, [zt, xt] + cols)]

            (ref, gref), (yard, gyard) = oracle(torch.float64), oracle(torch.float32)
            put = _strided if strided else (lambda t: t.to(DEV))
            zd, xd, sd, dd, sg = put(z), put(x), put(stat), put(dout), sigma.to(DEV)
            wide_ = sensors.to(DEV)
            if strided:
                c0, c1 = (None if s is None else wide_[:, s:s + 1] for s in slots)
            else:
                c0, c1 = (None if s is None else wide_[:, s:s + 1].contiguous() for s in slots)
            rows, c_noise = genda.genda_input_forward(zd, xd, sg, sd, c0, c1, copies, bool(drop))
            rows2, c_noise2 = genda.genda_input_forward(zd, xd, sg, sd, c0, c1, copies, bool(drop))
            grads = genda.genda_input_backward(dd, sg, wz, wx, cond, copies, bool(drop))
            grads2 = genda.genda_input_backward(dd, sg, wz, wx, cond, copies, bool(drop))
            torch.cuda.synchronize()
            assert rows.shape == (copies * B * G, wz + wx + cond + ws) and c_noise.shape == (copies * B, 1), what
            assert torch.isfinite(rows).all() and torch.isfinite(c_noise).all(), what
            # bitwise: the torch expression of the same float32 operations, and a second call
            wrong = int((rows.cpu() != yard).sum())
            print("%s: %d of %d elements differ from the float32 torch expression" % (what, wrong, yard.numel()))
            assert torch.equal(rows.cpu(), yard), what
            assert torch.equal(rows, rows2) and torch.equal(c_noise, c_noise2), what
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads, grads2)), what
            _bar(what + " c_noise", c_noise, (0.25 * torch.log(sigma.double())).repeat(copies, 1),
                 (1 / 4 * torch.log(sigma)).repeat(copies, 1))
            assert torch.equal(c_noise[:B], c_noise[B:2 * B]) or copies == 1, what
            if cond == 0 and not drop:  # the Denoiser's kernel, value for value
                if copies == 1:
                    base, base_noise = gencast.precond_input_forward(zd, xd, sg, sd)
                    assert torch.equal(rows, base) and torch.equal(c_noise, base_noise), what
            if copies == 2:  # copy 0 is the one-copy call; copy 1 the one-copy call on zero conditioning
                one, one_noise = genda.genda_input_forward(zd, xd, sg, sd, c0, c1, 1, bool(drop))
                zero = [None if c is None else torch.zeros_like(c) for c in (c0, c1)]
                unc, _ = genda.genda_input_forward(zd, xd, sg, sd, zero[0], zero[1], 1, False)
                assert torch.equal(rows[:B * G], one) and torch.equal(c_noise[:B], one_noise), what
                assert torch.equal(rows[B * G:], unc), what
            # the gradients against float64 autograd of the expression
            dz, dx, d0, d1 = grads
            assert (d0 is None) == (cond < 1) and (d1 is None) == (cond < 2), what
            for name, got, r_, y_ in zip(("dz", "dx", "dc0", "dc1"), [dz, dx] + [d for d in (d0, d1) if d is not None], gref, gyard):
                if r_.numel():
                    _bar("%s %s" % (what, name), got, r_, y_)
            if drop:
                assert all(d is None or not d.any() for d in (d0, d1)), what  # a dropped column passes no gradient
            # only some outputs wanted
            part = genda.genda_input_backward(dd, sg, wz, wx, cond, copies, bool(drop), want=(False, True, False, cond == 2))
            assert part[0] is None and part[2] is None and torch.equal(part[1], dx) and (cond < 2 or torch.equal(part[3], d1)), what


# ---------------------------------------------------------------------------------------------------------------------
# the guided output kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, -0.5])
@pytest.mark.parametrize("width", [1, 5, 8])
def test_guided_output_kernel(width, gamma):
    for B in (1, 3):
        for G in ROWS:
            rs = np.random.RandomState(2000 * B + 10 * G + width)
            z, preds, dout = _randn(rs, B * G, width), _randn(rs, 2 * B * G, width), _randn(rs, B * G, width)
            sigma = torch.tensor(SIGMAS[B], dtype=torch.float32)[:, None]
            strided = (B + G + width) % 2 == 1
            what = "guided output B %d G %d width %d gamma %s%s" % (B, G, width, gamma, " strided" if strided else "")

            def oracle(dtype):
                zt, pt = (t.to(dtype).clone().requires_grad_(True) for t in (z, preds))
                c_skip, c_out, _, _ = (c.repeat_interleave(G, 0) for c in mo.preconditioner(sigma.to(dtype)))
                o_c, o_u = c_skip * zt + c_out * pt[:B * G], c_skip * zt + c_out * pt[B * G:]
                out = o_u + gamma * (o_c - o_u)
                return [out.detach()] + list(torch.autograd.grad((out * dout.to(dtype)).sum(), (zt, pt)))

            ref, yard = oracle(torch.float64), oracle(torch.float32)
            put = _strided if strided else (lambda t: t.to(DEV))
            zd, pd, dd, sg = put(z), put(preds), put(dout), sigma.to(DEV)
            out = genda.guided_output_forward(zd, pd, sg, gamma)
            dz, dp = genda.guided_output_backward(dd, sg, gamma)
            again = (genda.guided_output_forward(zd, pd, sg, gamma),) + genda.guided_output_backward(dd, sg, gamma)
            torch.cuda.synchronize()
            assert out.shape == (B * G, width) and dz.shape == (B * G, width) and dp.shape == (2 * B * G, width), what
            assert all(torch.equal(a, b) for a, b in zip((out, dz, dp), again)), what
            _bar(what + " out", out, ref[0], yard[0])
            _bar(what + " dz", dz, ref[1], yard[1])
            _bar(what + " dp conditional", dp[:B * G], ref[2][:B * G], yard[2][:B * G])
            _bar(what + " dp unconditional", dp[B * G:], ref[2][B * G:], yard[2][B * G:])


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}
CASE_NAMES = list(do.CASES)
GUIDED = [n for n in CASE_NAMES if do.conditioned(n)]
INPUTS = ("corrupted_targets", "prev_inputs", "sensor_mask", "sensor_values")


def _case(name, golden_dir):
    """(model on the device, inputs on the CPU, loss weights, oracle closure, the fixture), once.  ``oracle(kind)`` -> ((float64
    output, gradients), (float32 output, gradients)) of ``kind`` "forward" or "guided", computed once and left unchanged."""
    if name in _MODELS:
        return _MODELS[name]
    _, kw, B, _, seed = do.CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cpu = fill_(GenDA(**do.case_kwargs(name)), seed).eval()
    inputs = do.case_inputs(name)
    w = _randn(np.random.RandomState(seed + 100), *inputs[0].shape)
    graphs, cache = mo.graph_tables(cpu), {}
    n_in = 5 if do.conditioned(name) else 3

    def oracle(kind):
        if kind not in cache:
            def run(dtype):
                p = params(cpu, dtype, requires_grad=True)
                z, x, s, mask, values = (t.to(dtype).clone() for t in inputs)
                leaves = [t.requires_grad_(True) for t in ((z, x, mask, values) if n_in == 5 else (z, x))]
                args = (z, x, s, mask, values)[:n_in]
                fn = do.genda_forward if kind == "forward" else do.genda_guided
                out = fn(p, kw, mo.cast_graphs(graphs, dtype), *args)
                keys = list(p)
                grads = torch.autograd.grad((out * w.to(dtype)).sum(), [p[k] for k in keys] + leaves)
                return out.detach(), dict(zip(keys + list(INPUTS[:len(leaves)]), grads))

            cache[kind] = (run(torch.float64), run(torch.float32))
        return cache[kind]

    _MODELS[name] = (cpu.to(DEV), inputs, w, oracle, g)
    return _MODELS[name]


def _device_inputs(inputs, n_in, grad=True):
    z, x, s, mask, values = (t.to(DEV) for t in inputs)
    leaves = [z, x] + ([mask, values] if n_in == 5 else [])
    if grad:
        for t in leaves:
            t.requires_grad_(True)
    return (z, x, s, mask, values)[:n_in], leaves


def _run(model, fn, inputs, w, n_in):
    args, leaves = _device_inputs(inputs, n_in)
    model.zero_grad(set_to_none=True)
    out = fn(*args)
    (out * w.to(DEV)).sum().backward()
    grads = {k: v.grad for k, v in model.named_parameters()}
    grads.update(zip(INPUTS, (t.grad for t in leaves)))
    return out.detach(), grads


def _fixture(what, out, recorded, ref, yard):
    yard_err = (yard.double() - ref).abs().max().item()
    bar = max(4.0 * yard_err, 1e-6 * ref.abs().max().item())
    err = (out.cpu().double() - torch.from_numpy(recorded).double()).abs().max().item()
    print("%s against the reference's recorded output: %.3e (yardstick %.3e, bar %.3e), ratio %.2f" % (what, err, yard_err, bar, err / yard_err))
    assert err <= bar, what


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_against_the_fixture_and_float64(golden_dir, name):
    model, inputs, w, oracle, g = _case(name, golden_dir)
    (ref, gref), (yard, gyard) = oracle("forward")
    n_in = 5 if do.conditioned(name) else 3
    model.eval()
    out, grads = _run(model, model, inputs, w, n_in)
    torch.cuda.synchronize()
    assert out.shape == inputs[0].shape and out.dtype == torch.float32 and out.is_cuda
    _bar(name + " forward", out, ref, yard)
    _fixture(name + " forward", out, g["out"], ref, yard)
    assert set(grads) == set(gref) and len(grads) == len(model.state_dict()) + n_in - 1
    for k in gref:
        assert grads[k] is not None, k
        _bar("%s forward d %s" % (name, k), grads[k], gref[k], gyard[k])
    again, grads2 = _run(model, model, inputs, w, n_in)
    assert torch.equal(out, again) and all(torch.equal(grads[k], grads2[k]) for k in grads)  # bitwise repeatable
    if n_in == 5:  # wind_direction is ignored
        args, _ = _device_inputs(inputs, 5, grad=False)
        with torch.no_grad():
            assert torch.equal(model(*args, wind_direction=torch.ones(3, device=DEV)), out)


@pytest.mark.parametrize("name", GUIDED)
def test_guided_forward_against_the_fixture_and_float64(golden_dir, name):
    model, inputs, w, oracle, g = _case(name, golden_dir)
    model.eval()
    args, _ = _device_inputs(inputs, 5, grad=False)
    if name == "genda_model_a":  # value and every gradient
        (ref, gref), (yard, gyard) = oracle("guided")
        out, grads = _run(model, lambda *a: model.guided_forward(*a, gamma=do.GAMMA), inputs, w, 5)
        assert set(grads) == set(gref) and len(grads) == len(model.state_dict()) + 4
        for k in gref:
            assert grads[k] is not None, k
            _bar("%s guided d %s" % (name, k), grads[k], gref[k], gyard[k])
        again, grads2 = _run(model, lambda *a: model.guided_forward(*a, gamma=do.GAMMA), inputs, w, 5)
        assert torch.equal(out, again) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    else:  # the value (the gradients of this case are checked through ``forward``)
        p64, p32 = params(model, torch.float64), params(model, torch.float32)
        graphs = mo.graph_tables(model)
        kw = do.CASES[name][1]
        ref = do.genda_guided(p64, kw, mo.cast_graphs(graphs, torch.float64), *(t.double() for t in inputs), do.GAMMA)
        yard = do.genda_guided(p32, kw, mo.cast_graphs(graphs, torch.float32), *inputs, do.GAMMA)
        with torch.no_grad():
            out = model.guided_forward(*args, gamma=do.GAMMA)
    torch.cuda.synchronize()
    assert out.shape == inputs[0].shape
    _bar(name + " guided", out, ref, yard)
    _fixture(name + " guided", out, g["guided"], ref, yard)
    # the reference's composition on this package's forward: within the same bar; bitwise equality is reported, not required
    with torch.no_grad():
        cond = model(*args)
        uncond = model(*args[:3], torch.zeros_like(args[3]), torch.zeros_like(args[4]))
        two = uncond + do.GAMMA * (cond - uncond)
        default = model.guided_forward(*args)
    _bar(name + " two forwards and the torch combine", two, ref, yard)
    print("%s: one-pass guided_forward and the two-forward composition bitwise equal: %s (largest difference %.3e)"
          % (name, torch.equal(out, two), (out - two).abs().max().item()))
    assert torch.equal(default, out) and do.GAMMA == 2.0  # the default gamma
    assert (cond - uncond).abs().max().item() > 1e-3  # the sensors matter


@pytest.mark.parametrize("name", CASE_NAMES)
def test_replicated_route_agrees(golden_dir, name):
    """The reference's route (replicated graph, public layer forwards, torch-op preconditioning) on this package's kernels: the same
    bar against float64; whether the two routes agree bitwise is reported."""
    model, inputs, w, oracle, _ = _case(name, golden_dir)
    (ref, gref), (yard, gyard) = oracle("forward")
    n_in = 5 if do.conditioned(name) else 3
    model.eval()
    out, grads = _run(model, lambda *a: _forward_replicated(model, *a), inputs, w, n_in)
    out_s, grads_s = _run(model, model, inputs, w, n_in)
    torch.cuda.synchronize()
    _bar(name + " replicated route", out, ref, yard)
    for k in gref:
        _bar("%s replicated route d %s" % (name, k), grads[k], gref[k], gyard[k])
    same = [k for k in gref if torch.equal(grads[k], grads_s[k])]
    print("%s: batch-shared and replicated route: outputs bitwise equal: %s (largest difference %.3e); gradients bitwise equal: %d of %d"
          % (name, torch.equal(out, out_s), (out - out_s).abs().max().item(), len(same), len(gref)))


def test_training_mode_dropout_follows_the_host_draw(golden_dir):
    """Under the recorded seed the reference's training-mode forward dropped the conditioning; under the first seed that does not
    hit it is the eval forward.  A hit is the kernel's flag: bitwise the forward on zero sensors, with zero sensor gradients."""
    model, inputs, w, oracle, g = _case("genda_model_a", golden_dir)
    (ref, _), (yard, _) = oracle("forward")
    args, _ = _device_inputs(inputs, 5, grad=False)
    zeros = (torch.zeros_like(args[3]), torch.zeros_like(args[4]))
    model.eval()
    eval_out, eval_zero = model(*args).detach(), model(*args[:3], *zeros).detach()
    with torch.no_grad():
        eval_guided, eval_guided_zero = model.guided_forward(*args), model.guided_forward(*args[:3], *zeros)
    try:
        model.train()
        torch.manual_seed(int(g["train_seed"]))
        hit, grads = _run(model, model, inputs, w, 5)
        after = torch.rand(1).item()
        torch.manual_seed(int(g["train_seed"]))
        stream = [torch.rand(1).item() for _ in range(3)]
        assert stream[0] < 0.1 and after == stream[1]  # one host draw
        print("training forward under the recorded seed against the eval forward on zero sensors: largest difference %.3e"
              % (hit - eval_zero).abs().max().item())
        assert torch.equal(hit, eval_zero) and not torch.equal(hit, eval_out)
        assert not grads["sensor_mask"].any() and not grads["sensor_values"].any()
        assert grads["corrupted_targets"].abs().max().item() > 0
        # the recorded output is the reference's float32 result on zero conditioning: the yardstick of that computation
        p64, p32 = params(model, torch.float64), params(model, torch.float32)
        graphs, kw = mo.graph_tables(model), do.CASES["genda_model_a"][1]
        z, x, s, mask, values = inputs
        ref0 = do.genda_forward(p64, kw, mo.cast_graphs(graphs, torch.float64), z.double(), x.double(), s.double(),
                                torch.zeros_like(mask).double(), torch.zeros_like(values).double())
        yard0 = do.genda_forward(p32, kw, mo.cast_graphs(graphs, torch.float32), z, x, s, torch.zeros_like(mask), torch.zeros_like(values))
        _bar("training forward under the recorded seed", hit, ref0, yard0)
        _fixture("training forward under the recorded seed", hit, g["train_out"], ref0, yard0)
        torch.manual_seed(int(g["train_miss_seed"]))
        miss = model(*args).detach()
        with torch.no_grad():
            torch.manual_seed(int(g["train_seed"]))
            guided_hit = model.guided_forward(*args)
            after = torch.rand(1).item()
            torch.manual_seed(int(g["train_miss_seed"]))
            guided_miss = model.guided_forward(*args)
        assert torch.equal(miss, eval_out)
        assert after == stream[2]  # two host draws, the first decides the conditional half
        assert torch.equal(guided_hit, eval_guided_zero) and torch.equal(guided_miss, eval_guided)
    finally:
        model.eval()


def test_training_step_is_bitwise_repeatable(golden_dir):
    model, inputs, w, _, _ = _case("genda_model_a", golden_dir)
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def steps():
        model.load_state_dict(state)
        model.train()
        torch.manual_seed(3)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        outs = []
        for fn in (model, model.guided_forward):
            out, _ = _run(model, fn, inputs, w, 5)
            opt.step()
            outs.append(out)
        return outs + [v.detach().clone() for v in model.state_dict().values()]

    try:
        a, b = steps(), steps()
        torch.cuda.synchronize()
    finally:
        model.load_state_dict(state)
        model.eval()
    assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.isfinite(p).all() for p in a)
    assert any(not torch.equal(p, state[k]) for p, k in zip(a[2:], state))  # the steps moved the parameters


def test_eval_forwards_replay_in_a_hip_graph(golden_dir):
    model, inputs, _, _, _ = _case("genda_model_a", golden_dir)
    model.eval()
    args, _ = _device_inputs(inputs, 5, grad=False)
    args = tuple(t.clone() for t in args)
    with torch.no_grad():
        first = (model(*args), model.guided_forward(*args))  # eager: sorts the edges once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y, y_guided = model(*args), model.guided_forward(*args)
    rs = np.random.RandomState(62)
    fresh = [_randn(rs, *t.shape).to(DEV) for t in args]
    fresh[2] = torch.tensor([[1.5], [0.2]], device=DEV)
    fresh[3] = (fresh[3] > 0.5).float()
    for t, f in zip(args, fresh):
        t.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager, eager_guided = model(*fresh), model.guided_forward(*fresh)
    assert torch.equal(y, eager) and torch.equal(y_guided, eager_guided) and torch.isfinite(y).all() and torch.isfinite(y_guided).all()
    assert not torch.equal(eager, first[0]) and not torch.equal(eager_guided, first[1])


# ---------------------------------------------------------------------------------------------------------------------
# the sampler over the guided view
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_over_the_guided_view(golden_dir):
    """``Sampler.sample`` (unchanged) over ``model.guided(mask, values, 2.0)`` on case a at B = 1, with the recorded coefficient draws.
    The reference's own ``Sampler`` calls ``denoiser(x, prev_inputs, noise_levels)`` and so cannot pass sensors to GenDA: the
    restatement ``gencast_sampler_oracle.sampler_sample`` run over the float64 ``genda_guided`` is the only oracle of this test."""
    model, _, _, _, g = _case("genda_model_a", golden_dir)
    model.eval()
    name, kw = "genda_model_a", do.CASES["genda_model_a"][1]
    _, prev, _, mask, values = do.case_inputs(name, batch=1)
    draws = [torch.view_as_complex(torch.from_numpy(d).contiguous()) for d in g["sampler_draws"]]
    graphs = mo.graph_tables(model)
    outs = []
    for dt in (torch.float64, torch.float32):
        p, gr, m, v = params(model, dt), mo.cast_graphs(graphs, dt), mask.to(dt), values.to(dt)
        with torch.no_grad():
            outs.append(so.sampler_sample(lambda x, pr, sig: do.genda_guided(p, kw, gr, x, pr, sig, m, v, 2.0), prev, draws, model.num_lon,
                                          model.num_lat, dt, num_steps=5))
    ref, yard = outs
    scale, yard_err = ref.abs().max().item(), (yard.double() - ref).abs().max().item()
    print("guided sampler: maximum %.3e, float32 restatement error %.3e (%.2e of the maximum)" % (scale, yard_err, yard_err / scale))
    assert yard_err <= 1e-3 * scale, "the trajectory is ill-conditioned: the bar would hide a failure"
    sampler = Sampler(num_steps=5)
    view = model.guided(mask.to(DEV), values.to(DEV), 2.0)
    with torch.no_grad():
        out = sampler.sample(view, prev.to(DEV), coeffs=[d.to(DEV) for d in draws])
        again = sampler.sample(view, prev.to(DEV), coeffs=[d.to(DEV) for d in draws])
        plain = sampler.sample(model.guided(torch.zeros_like(mask).to(DEV), torch.zeros_like(values).to(DEV), 2.0), prev.to(DEV),
                               coeffs=[d.to(DEV) for d in draws])
    torch.cuda.synchronize()
    assert out.shape == (1, model.num_lon, model.num_lat, model.output_features_dim)
    _bar("guided sampler num_steps 5", out, ref, yard)
    assert torch.equal(out, again)
    print("guided sampler: largest difference to the run without sensors %.3e" % (out - plain).abs().max().item())
    assert (out - plain).abs().max().item() > 1e-3 * scale  # the sensors steer the analysis
