"""PhysicalConstraintLayer on the GPU (csrc/gw_constraint.hip): the kernels against fp64 closed forms at ragged sizes, the
constrained forecaster against the oracle plus the closed form (the node -> grid map is not a bijection at 5 and 1 degree),
the reference's own test_model.py constraint cases, gradients against fp64 autograd, and the paths that must stay
bitwise reproducible (eager twice, AutoGraph replay, batch split)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd.constraint import ConstraintFunction, grid_maps, inverse_csr  # noqa: E402
from graph_weather_amd._lib import CONSTRAINT_TYPES  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402
from oracle import reference_math as om  # noqa: E402

from .oracle_gpu import forecast as oracle_forecast  # noqa: E402

DEV = "cuda:0"
TYPES = ("additive", "multiplicative", "softmax")


def closed_form(ctype, hr, lr, index, a=1.0):
    """fp64 (or the inputs' dtype) closed forms with f = 1: hr, lr [B, K, C] rows, index [N] the row each node reads."""
    h, l = hr[:, index], lr[:, index]
    if ctype == "additive":
        return h + (l - h.mean(dim=1, keepdim=True))
    if ctype == "multiplicative":
        return h * (l.mean(dim=1, keepdim=True) / (h.mean(dim=1, keepdim=True) + 1e-8))
    e = torch.exp(a * h)
    return e * (l * (1 / e))


def random_map(N, seed):
    """A node -> row map over K = N rows with duplicates and rows nobody reads (like the 1-degree grid's)."""
    rs = np.random.RandomState(seed)
    m = np.arange(N)
    dup = rs.rand(N) < 0.15
    m[dup] = rs.randint(0, N, size=int(dup.sum()))
    return m


def dev_maps(m, rows):
    ptr, idx = inverse_csr(m, rows)
    return tuple(torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (m, ptr, idx))


def _rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@pytest.mark.parametrize("N,C,B", [(4, 1, 1), (4, 3, 16), (2592, 78, 2), (2592, 605, 1), (64800, 2, 2), (64800, 78, 2)])
@pytest.mark.parametrize("ctype", TYPES)
def test_kernels_against_fp64_closed_forms(ctype, N, C, B):
    m = random_map(N, N + C)
    gen = torch.Generator().manual_seed(N * 7 + C)
    hr = torch.randn(B, N, C, generator=gen) + 1.5  # |mean hr| away from 0 for the multiplicative ratio
    ld = C + 5  # lr read through a row stride, like the forecaster's features
    lr = torch.randn(B, N, ld, generator=gen)
    a = 0.7
    spec = (CONSTRAINT_TYPES[ctype], 1, 1, N, 0, a)
    hr_d, lr_d = hr.to(DEV).requires_grad_(True), lr.to(DEV).requires_grad_(True)
    out = ConstraintFunction.apply(hr_d, lr_d, spec, dev_maps(m, N))
    hr64, lr64 = hr.double().requires_grad_(True), lr.double().requires_grad_(True)
    ref = closed_form(ctype, hr64, lr64[..., :C], m, a)
    assert out.shape == (B, N, C)
    assert _rel(out, ref) <= 2e-6
    g = torch.randn(B, N, C, generator=gen)
    out.backward(g.to(DEV))
    if ctype == "softmax":
        # the true d/dhr is rounding noise: compare with the fp32 autograd of the reference's op sequence, absolute bar
        hr32, lr32 = hr.clone().requires_grad_(True), lr.clone().requires_grad_(True)
        closed_form(ctype, hr32, lr32[..., :C], m, a).backward(g)
        assert (hr_d.grad.cpu() - hr32.grad).abs().max().item() <= 1e-5 * max(1.0, g.abs().max().item())
        assert _rel(lr_d.grad, lr32.grad) <= 2e-6
    else:
        ref.backward(g.double())
        assert _rel(hr_d.grad, hr64.grad) <= 2e-5
        assert _rel(lr_d.grad, lr64.grad) <= 2e-5
    assert torch.count_nonzero(lr_d.grad[..., C:]) == 0


def test_softmax_overflows_where_the_reference_does():
    m = random_map(300, 1)
    hr = torch.randn(1, 300, 4) * 3
    hr[0, 5, 0], hr[0, 9, 1], hr[0, 17, 2] = 200.0, -200.0, 90.0  # exp -> inf, exp -> 0
    lr = torch.randn(1, 300, 4)
    lr[0, 9, 1] = 0.0
    ref = closed_form("softmax", hr, lr, m)  # fp32, the reference's order
    out = ConstraintFunction.apply(hr.to(DEV), lr.to(DEV), (3, 1, 1, 300, 0, 1.0), dev_maps(m, 300)).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.isnan(ref).any()
    fin = torch.isfinite(ref)
    assert torch.allclose(out[fin], ref[fin], rtol=1e-6, atol=1e-6)


class _Grid:
    def __init__(self, H, W):
        self.node_to_grid = [(i, j) for i in range(H) for j in range(W)]
        rs = np.random.RandomState(H * W)
        for n in rs.choice(H * W, size=H * W // 7, replace=False):  # duplicate cells, as truncation makes them
            self.node_to_grid[n] = (int(rs.randint(H)), int(rs.randint(W)))


@pytest.mark.parametrize("f,H,W,B,C", [(2, 6, 12, 2, 3), (3, 9, 12, 1, 78), (2, 36, 72, 2, 5)])
def test_softmax_blocks_against_fp64_autograd(f, H, W, B, C):
    stub = _Grid(H, W)
    layer = gw.PhysicalConstraintLayer(stub, (H, W), f, "softmax", exp_factor=0.6)
    gen = torch.Generator().manual_seed(f * H + C)
    y = torch.randn(B, C, H, W, generator=gen)
    lr = torch.randn(B, C, H // f, W // f, generator=gen)
    g = torch.randn(B, H * W, C, generator=gen)
    yd, lrd = y.to(DEV).requires_grad_(True), lr.to(DEV).requires_grad_(True)
    out = layer(yd, lrd)
    out.backward(g.to(DEV))
    y64, lr64 = y.double().requires_grad_(True), lr.double().requires_grad_(True)
    E = torch.exp(0.6 * y64)
    S = torch.nn.functional.avg_pool2d(E, f) * f * f
    R = E * torch.kron(lr64 * (1 / S), torch.ones(f, f, dtype=torch.float64))
    pi = grid_maps(stub.node_to_grid, (H, W))["pi"]
    ref = R.permute(0, 2, 3, 1).reshape(B, H * W, C)[:, pi]
    ref.backward(g.double())
    assert _rel(out, ref) <= 2e-6
    assert _rel(yd.grad, y64.grad) <= 2e-5
    assert _rel(lrd.grad, lr64.grad) <= 2e-5


@pytest.mark.parametrize("ctype", TYPES)
def test_layer_graph_inputs_read_the_surviving_node(ctype):
    stub = _Grid(6, 12)
    layer = gw.PhysicalConstraintLayer(stub, (6, 12), 1, ctype)
    gen = torch.Generator().manual_seed(3)
    hr, lr = torch.randn(2, 72, 4, generator=gen) + 1.0, torch.randn(2, 72, 4, generator=gen)
    hd = hr.to(DEV).requires_grad_(True)
    out = layer(hd, lr.to(DEV))
    sigma = grid_maps(stub.node_to_grid, (6, 12))["sigma"]
    assert _rel(out, closed_form(ctype, hr.double(), lr.double(), sigma)) <= 2e-6
    out.sum().backward()
    dead = np.setdiff1d(np.arange(72), sigma)
    assert len(dead) and torch.count_nonzero(hd.grad[:, dead]) == 0  # overwritten nodes get no gradient, as in the reference


def _forecaster(res, ctype, seed=1, **kw):
    model = gw.GraphWeatherForecaster(regular_lat_lons(res), constraint_type=ctype, **kw)
    deterministic_fill_(model, seed=seed)
    return model


@pytest.mark.parametrize("ctype", TYPES)
def test_forecaster_5deg_against_oracle_and_closed_form(ctype):
    """fp32 against the oracle plus the closed form; bf16x3 against the closed form applied to the same model's unconstrained
    bf16x3 output (the multiplicative ratio amplifies the mode's own 1e-3-level error by |x| / |mean x|)."""
    model, plain = _forecaster(5.0, ctype), _forecaster(5.0, "none")
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    feats = seeded_features(1, 2592, 102, seed=5)
    pi = torch.from_numpy(grid_maps(model.node_to_grid, model.grid_shape)["pi"]).to(DEV)
    y_ref = oracle_forecast(sd, model.encoder.graphs.as_oracle_dict(), feats, DEV)
    lr64 = feats.to(DEV).double()[..., :78]
    model, plain = model.to(DEV).eval(), plain.to(DEV).eval()
    for dtype in (torch.float32, "bf16x3"):
        model.set_compute_dtype(dtype)
        plain.set_compute_dtype(dtype)
        with torch.no_grad():
            y = model(feats.to(DEV))
            base = y_ref if dtype is torch.float32 else plain(feats.to(DEV)).double()
        ref = closed_form(ctype, base, lr64, pi)
        err = (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
        print(f"[constraint] 5deg {ctype} {dtype}: max rel {err:.2e}")
        assert err <= 1e-5


@pytest.mark.parametrize("ctype", TYPES)
def test_forecaster_1deg_b2_against_oracle(ctype):
    model = _forecaster(1.0, ctype)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    feats = seeded_features(2, 64800, 102, seed=9)
    y_ref = oracle_forecast(sd, model.encoder.graphs.as_oracle_dict(), feats, DEV)
    pi = torch.from_numpy(grid_maps(model.node_to_grid, model.grid_shape)["pi"]).to(DEV)
    ref = closed_form(ctype, y_ref, feats.to(DEV).double()[..., :78], pi)
    del y_ref
    model = model.to(DEV).eval()
    with torch.no_grad():
        y = model(feats.to(DEV))
    err = (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
    print(f"[constraint] 1deg B=2 {ctype}: max rel {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("ctype", TYPES)
def test_reference_test_model_constraint_cases(ctype):
    """tests/test_model.py:374-464 of the reference as written (2 x 2 grid, feature_dim 2, aux_dim 0), on the device."""
    lats = np.linspace(-90, 90, 2)
    lons = np.linspace(-90, 90, 2)
    lat_lons = [(lat, lon) for lat in lats for lon in lons]
    model = gw.GraphWeatherForecaster(lat_lons, constraint_type=ctype, feature_dim=2, aux_dim=0, output_dim=2).to(DEV)
    torch.manual_seed(0)
    inp = torch.randn(1, len(lat_lons), 2)
    output = model(inp.to(DEV))
    assert output.shape == (1, 4, 2) and output.device.type == "cuda"
    lr_input_avg = model.graph_to_grid(inp[..., :2]).mean(dim=(-2, -1))
    lr_output_avg = model.graph_to_grid(output.detach().cpu()).mean(dim=(-2, -1))
    assert torch.allclose(lr_input_avg, lr_output_avg, atol=0.0001), f"Conservation failed: {lr_input_avg} vs {lr_output_avg}"


@pytest.mark.parametrize("res", [10.0, 5.0])
@pytest.mark.parametrize("ctype", ["additive", "multiplicative"])
def test_forecaster_gradients_against_fp64_autograd(ctype, res):
    lat_lons = regular_lat_lons(res)
    model = _forecaster(res, ctype, seed=4, num_blocks=2)
    ref = {k: v.detach().to(DEV, torch.float64).requires_grad_(True) for k, v in model.state_dict().items()}
    g64 = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in model.encoder.graphs.as_oracle_dict().items()}
    g64 = om.graphs_to_dtype(g64, torch.float64)
    G = len(lat_lons)
    feats = seeded_features(2, G, 102, seed=8)
    rs = np.random.RandomState(3)
    target = torch.from_numpy(rs.standard_normal((2, G, 78)).astype(np.float32))
    pi = torch.from_numpy(grid_maps(model.node_to_grid, model.grid_shape)["pi"]).to(DEV)
    f64 = feats.to(DEV, torch.float64).requires_grad_(True)
    with torch.device(DEV):
        y_ref = closed_form(ctype, om.forecaster_forward(ref, g64, f64), f64[..., :78], pi)
        om.normalized_mse_loss(y_ref, target.to(DEV, torch.float64), lat_lons, None, normalize=False).backward()
    model = model.to(DEV).train()
    fd = feats.to(DEV).requires_grad_(True)
    crit = gw.NormalizedMSELoss(lat_lons=lat_lons, feature_variance=[1.0] * 78)
    crit(model(fd), target.to(DEV)).backward()
    # bar as in test_gpu_backward.py: 2e-3, or 4x the oracle's own fp32-vs-fp64 autograd distance (the additive constraint
    # subtracts the gradient's mean: more cancellation); gradients that are zero in exact arithmetic (a bias in front of the
    # additive constraint shifts h and mean h alike) are measured against 1e-4 of the largest gradient
    ref32 = {k: v.detach().float().requires_grad_(True) for k, v in ref.items()}
    f32 = feats.to(DEV).requires_grad_(True)
    g32 = om.graphs_to_dtype(g64, torch.float32)
    with torch.device(DEV):
        y32 = closed_form(ctype, om.forecaster_forward(ref32, g32, f32), f32[..., :78], pi)
        om.normalized_mse_loss(y32, target.to(DEV), lat_lons, None, normalize=False).backward()
    gmax = max(v.grad.abs().max().item() for v in ref.values())

    def rel(a, r):
        return (a.detach().double() - r.detach().double()).abs().max().item() / max(r.abs().max().item(), 1e-4 * gmax)

    noise = max(rel(ref32[k].grad, ref[k].grad) for k in ref)
    bar = max(2e-3, 4 * noise)
    bad = [(k, rel(p.grad, ref[k].grad)) for k, p in model.named_parameters() if rel(p.grad, ref[k].grad) >= bar]
    assert not bad, (bar, bad[:6])
    assert _rel(fd.grad, f64.grad) < bar


def test_adamw_step_of_a_constrained_model():
    model = _forecaster(10.0, "additive", seed=6, num_blocks=2).to(DEV).train()
    feats = seeded_features(1, 648, 102, seed=2).to(DEV)
    crit = gw.NormalizedMSELoss(lat_lons=regular_lat_lons(10.0), feature_variance=[1.0] * 78)
    crit(model(feats), feats[..., :78] * 0.5).backward()
    twin = [p.detach().clone().requires_grad_(True) for p in model.parameters()]
    for t, p in zip(twin, model.parameters()):
        t.grad = p.grad.clone()
    torch.optim.AdamW(twin, lr=1e-3).step()
    gw.AdamW(model.parameters(), lr=1e-3).step()
    for t, p in zip(twin, model.parameters()):
        torch.testing.assert_close(p.detach(), t.detach(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("ctype", TYPES)
def test_bitwise_paths(ctype):
    model = _forecaster(5.0, ctype).to(DEV).eval()
    feats = seeded_features(2, 2592, 102, seed=12).to(DEV)
    with torch.no_grad():
        y_a = model._forward_eager(feats).clone()
        y_b = model._forward_eager(feats).clone()
        assert torch.equal(y_a, y_b)  # fixed-order reduction
        ys = [model(feats).clone() for _ in range(4)]  # AutoGraph replays from the third call
        for y in ys:
            assert torch.equal(y, y_a)
        # per-sample statistics: the layer on a batch of two equals it on each sample
        hr = torch.randn(2, 2592, 78, device=DEV) + 1.0
        both = model.constraint.apply_rows(hr, feats)
        one = torch.cat([model.constraint.apply_rows(hr[i:i + 1], feats[i:i + 1]) for i in range(2)])
        assert torch.equal(one, both)


def test_rollout_of_a_constrained_model():
    model = _forecaster(10.0, "multiplicative").to(DEV).eval()
    feats = seeded_features(1, 648, 102, seed=4).to(DEV)
    with torch.no_grad():
        outs = gw.rollout(model, feats, 2)
        x = feats
        for s in range(2):
            y = model._forward_eager(x)
            assert torch.equal(outs[s] if isinstance(outs, (list, tuple)) else outs[:, s], y)
            x = torch.cat([y, x[..., 78:]], dim=-1).contiguous()
