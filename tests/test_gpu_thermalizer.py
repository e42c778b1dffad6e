"""ThermalizerLayer / AdaptiveUNet on csrc/gw_thermal.hip against the fp64 restatement in tests/thermal_oracle.py: the score
model of both branches, the diffusion step, gradients, the forecaster with the thermalizer, AutoGraph replay, determinism."""
import pytest
import torch

from . import thermal_oracle as to
from .oracle_gpu import graphs_on, params_on

import graph_weather_amd as gw
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features
from oracle import reference_math as om

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _rel(a, b, floor: float = 1e-30) -> float:
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), floor)


def _grad_floor(grads) -> float:
    """A conv bias right before a GroupNorm has a zero gradient (the norm removes it): its fp32 value is rounding noise, so
    max-rel is taken against 1e-4 of the largest gradient of the model."""
    return 1e-4 * max(g.double().abs().max().item() for g in grads if g is not None)


def _sd64(module, prefix=""):
    return {k: v.detach().to(DEV, torch.float64) for k, v in to.strip(module.state_dict(), prefix).items()}


def _unet(cin, cout, seed=0):
    return to.fill_(gw.AdaptiveUNet(cin, cout), seed).to(DEV)


# (B, H, W, C): both branches, (1, N) strips, odd sizes whose UNet levels need the bilinear resize
SCORE_CASES = [(1, 1, 11764, 258), (1, 1, 5, 5), (2, 3, 3, 34), (1, 5, 5, 34), (2, 12, 12, 34), (1, 13, 9, 258), (1, 170, 173, 34),
               (1, 181, 360, 82), (1, 1, 5882, 1026), (1, 13, 9, 1026)]  # (Cin 1026: ThermalizerLayer(1024) of 1024-wide models)


@pytest.mark.parametrize("B,H,W,C", SCORE_CASES)
def test_score_model_forward(B, H, W, C):
    m = _unet(C, C - 2, seed=1)
    g = torch.Generator().manual_seed(B * 7 + H * 3 + W)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    with torch.no_grad():
        y = m(x)
        ref = to.score(_sd64(m), x.double())
    assert y.shape == ref.shape
    # fp32 MFMA chains over K = 49 cin (conv1) through 18 layers: the UNet lands at 1.1e-5 of max|ref|, simple_net well below 1e-5
    assert _rel(y, ref) <= (1e-5 if min(H, W) <= 4 else 2e-5), (B, H, W, C, _rel(y, ref))


LAYER_CASES = [(1, 1, 11764, 256), (1, 3, 3, 32), (2, 5, 5, 3), (2, 6, 8, 32), (2, 13, 9, 32), (1, 170, 173, 32)]


@pytest.mark.parametrize("B,H,W,F", LAYER_CASES)
@pytest.mark.parametrize("t", [0, 500, 999, torch.tensor(500), torch.tensor([1234])])
def test_layer_forward(B, H, W, F, t):
    layer = to.fill_(gw.ThermalizerLayer(F), 2).to(DEV)
    x = torch.randn(B * H * W, F, generator=torch.Generator().manual_seed(H * W + F)).to(DEV)
    with torch.no_grad():
        y = layer(x, t, height=H, width=W, batch=B)
    tv = min(int(torch.as_tensor(t).reshape(-1)[0]), 999)
    ref = to.thermalize(_sd64(layer, "score_model."), x.double(), layer.last_noise, tv, B, H, W)
    assert _rel(y, ref) <= 1e-5, (B, H, W, F, tv, _rel(y, ref))


def test_layer_reads_padded_rows_in_place():
    layer = to.fill_(gw.ThermalizerLayer(32), 3).to(DEV)
    wide = torch.randn(64, 256, device=DEV)
    with torch.no_grad(), pytest.warns(UserWarning):
        y = layer(wide[:, :32], 500)
    ref = to.thermalize(_sd64(layer, "score_model."), wide[:, :32].double(), layer.last_noise, 500, 1, 8, 8)
    assert _rel(y, ref) <= 1e-5


@pytest.mark.parametrize("B,H,W,F", [(2, 1, 40, 8), (1, 4, 4, 8), (1, 13, 9, 8), (2, 12, 12, 8)])
def test_layer_gradients(B, H, W, F):
    layer = to.fill_(gw.ThermalizerLayer(F), 4).to(DEV)
    x = torch.randn(B * H * W, F, generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_(True)
    gout = torch.randn(B * H * W, F, generator=torch.Generator().manual_seed(6)).to(DEV)
    y = layer(x, 500, height=H, width=W, batch=B)
    (y * gout).sum().backward()
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd64(layer, "score_model.").items()}
    x64 = x.detach().double().requires_grad_(True)
    ref = to.thermalize(sd, x64, layer.last_noise, 500, B, H, W)
    (ref * gout.double()).sum().backward()
    assert _rel(x.grad, x64.grad) <= 2e-3
    simple = min(H, W) <= 4
    floor = _grad_floor([v.grad for v in sd.values()])
    for k, p in layer.score_model.named_parameters():
        if k.startswith("simple_net") != simple:
            assert p.grad is None, k  # the branch that did not run
            continue
        assert _rel(p.grad, sd[k].grad, floor) <= 2e-3, (k, _rel(p.grad, sd[k].grad, floor))


@pytest.mark.parametrize("H,W", [(1, 40), (13, 9)])
def test_nan_propagates_like_torch(H, W):
    """torch's ReLU keeps NaN: a diverged input row must not come out finite."""
    layer = to.fill_(gw.ThermalizerLayer(8), 8).to(DEV)
    x = torch.randn(H * W, 8, device=DEV)
    x[3, 2] = float("nan")
    with torch.no_grad():
        y = layer(x, 500, height=H, width=W)
    assert torch.isnan(y).any()


def test_determinism():
    layer = to.fill_(gw.ThermalizerLayer(32), 7).to(DEV)
    x = torch.randn(2 * 13 * 9, 32, device=DEV)
    with torch.no_grad():
        a = layer(x, 500, height=13, width=9, batch=2)
        b = layer(x, 500, height=13, width=9, batch=2, noise=layer.last_noise)
    assert torch.equal(a, b)


def _forecaster(B_res=2, seed=1, **kw):
    model = gw.GraphWeatherForecaster(regular_lat_lons(10.0), resolution=B_res, use_thermalizer=True, **kw)
    deterministic_fill_(model, seed=seed)
    to.fill_(model.processor.thermalizer, seed)
    return model.to(DEV)


def _oracle_forecast(model, feats, noise, t, fdim=78):
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = model.encoder.graphs.as_oracle_dict()
    with torch.no_grad(), torch.device(DEV):
        p = params_on(sd, DEV, torch.float64)
        gg = graphs_on(g, DEV, torch.float64)
        f = feats.to(DEV, torch.float64)
        x, ei, ea = om.encoder_forward(p, gg, f)
        xp = om.processor_forward(p, x, ei, ea)
        H, W = gw.thermalizer.infer_grid_dimensions(int(xp.shape[0]))
        xt = to.thermalize(to.strip(p, "processor.thermalizer.score_model."), xp, noise, t, 1, H, W)
        return om.decoder_forward(p, gg, xt, f[..., :fdim])


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_forecaster_forward(B, dtype):
    model = _forecaster().eval()
    if dtype != "fp32":
        model.set_compute_dtype(dtype)
    feats = seeded_features(B, 648, 102, seed=B)
    with torch.no_grad(), pytest.warns(UserWarning):
        y = model(feats.to(DEV), t=500)
    ref = _oracle_forecast(model, feats, model.processor.thermalizer.last_noise, 500)
    scale = (ref - feats[..., :78].to(DEV, torch.float64)).abs().max().item()
    bar = 2e-4 if dtype == "fp32" else 1e-3
    assert (y.double() - ref).abs().max().item() <= bar * scale


@pytest.mark.parametrize("B", [2, 5])
def test_forecaster_gradients(B):
    model = _forecaster(seed=2)
    feats = seeded_features(B, 648, 102, seed=B + 1)
    target = seeded_features(B, 648, 78, seed=B + 2).to(DEV)
    torch.manual_seed(B)  # (a reproducible noise draw)
    with pytest.warns(UserWarning):
        y = model(feats.to(DEV), t=500)
    ((y - target) ** 2).mean().backward()
    noise = model.processor.thermalizer.last_noise
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = model.encoder.graphs.as_oracle_dict()
    with torch.device(DEV):
        p = params_on(sd, DEV, torch.float64, requires_grad=True)
        gg = graphs_on(g, DEV, torch.float64)
        f = feats.to(DEV, torch.float64)
        x, ei, ea = om.encoder_forward(p, gg, f)
        xp = om.processor_forward(p, x, ei, ea)
        H, W = gw.thermalizer.infer_grid_dimensions(int(xp.shape[0]))
        xt = to.thermalize(to.strip(p, "processor.thermalizer.score_model."), xp, noise, 500, 1, H, W)
        ref = om.decoder_forward(p, gg, xt, f[..., :78])
        ((ref - target.double()) ** 2).mean().backward()
    floor = _grad_floor([v.grad for v in p.values()])
    bad = {}
    for k, prm in model.named_parameters():
        if prm.grad is None:  # only the thermalizer branch that did not run
            assert k.startswith("processor.thermalizer.score_model.") and (".simple_net." in k) != (min(H, W) <= 4), k
            continue
        err = _rel(prm.grad, p[k].grad, floor)
        if "thermalizer" in k and min(H, W) > 4:
            # Behind the UNet's max-pools the fp32 path and the fp64 oracle see inputs that differ by the processor's rounding,
            # so a near-tie can pick a different argmax and move one pixel's gradient: the max-rel error of a weight gradient
            # then jumps (2e-3 to 6e-3 over noise draws) while its relative l2 error stays small.  Both are held.
            d = (prm.grad.double() - p[k].grad).norm().item() / max(p[k].grad.norm().item(), floor)
            if not (err <= 1e-2 and d <= 2e-3):
                bad[k] = (err, d)
        elif not err <= 2e-3:  # the bar of test_gpu_backward.py
            bad[k] = err
    assert not bad, bad


def test_reference_cases():
    """tests/test_gencast_with_thermalizer.py of the reference: 3 x 3 and 2 x 2 grids, feature_dim 3, aux_dim 0, one block."""
    for n, t in ((3, 500), (2, 50)):
        ll = [(i // n, i % n) for i in range(n * n)]
        model = gw.GraphWeatherForecaster(ll, use_thermalizer=True, feature_dim=3, aux_dim=0, node_dim=256, num_blocks=1)
        deterministic_fill_(model, seed=3)
        to.fill_(model.processor.thermalizer, 3)
        model = model.to(DEV).eval()
        feats = torch.randn(1, n * n, 3)
        with torch.no_grad(), pytest.warns(UserWarning):
            y = model(feats.to(DEV), t=t)
        assert y.shape == feats.shape and torch.isfinite(y).all()
        ref = _oracle_forecast(model, feats, model.processor.thermalizer.last_noise, t, fdim=3)
        scale = (ref - feats.to(DEV, torch.float64)).abs().max().item()
        assert (y.double() - ref).abs().max().item() <= 2e-4 * max(scale, 1.0)


def test_narrow_model():
    model = _forecaster(node_dim=32, edge_dim=32, hidden_dim_processor_node=32, hidden_dim_processor_edge=32).eval()
    feats = seeded_features(1, 648, 102, seed=9)
    with torch.no_grad(), pytest.warns(UserWarning):
        y = model(feats.to(DEV), t=500)
    ref = _oracle_forecast(model, feats, model.processor.thermalizer.last_noise, 500)
    scale = (ref - feats[..., :78].to(DEV, torch.float64)).abs().max().item()
    assert (y.double() - ref).abs().max().item() <= 2e-4 * scale


def test_auto_graph_replay():
    model = _forecaster(seed=5).eval()
    feats = seeded_features(2, 648, 102, seed=11).to(DEV)
    th = model.processor.thermalizer
    outs = []
    with torch.no_grad(), pytest.warns(UserWarning):
        for _ in range(4):
            y = model(feats, t=500)
            outs.append((y.clone(), th.last_noise.clone()))
        fg = model.__dict__["_auto"]._fg
        assert fg is not None and fg.captures == 1
        for y, noise in outs:
            ref = _oracle_forecast(model, feats.cpu(), noise, 500)
            scale = (ref - feats[..., :78].double()).abs().max().item()
            assert (y.double() - ref).abs().max().item() <= 2e-4 * scale
        assert not torch.equal(outs[-1][0], outs[-2][0])  # each replay draws fresh noise
    with torch.enable_grad(), pytest.warns(UserWarning):  # an eager call in between (AutoGraph steps aside under grad)
        model(feats, t=500)
    with torch.no_grad():
        y = model(feats, t=500)  # replayed: last_noise is the replay's buffer again, not the eager call's tensor
        assert fg.captures == 1
        ref = _oracle_forecast(model, feats.cpu(), th.last_noise, 500)
        scale = (ref - feats[..., :78].double()).abs().max().item()
        assert (y.double() - ref).abs().max().item() <= 2e-4 * scale
    with torch.no_grad(), pytest.warns(UserWarning):
        y0 = model(feats, t=0)
        ref = _oracle_forecast(model, feats.cpu(), th.last_noise, 0)
        scale = (ref - feats[..., :78].double()).abs().max().item()
        assert (y0.double() - ref).abs().max().item() <= 2e-4 * scale
        assert fg.captures == 1


def test_processor_efficient_batching():
    proc = gw.Processor(input_dim=32, edge_dim=32, num_blocks=1, hidden_dim_processor_node=32, hidden_dim_processor_edge=32,
                        use_thermalizer=True)
    deterministic_fill_(proc, seed=4)
    to.fill_(proc.thermalizer, 4)
    proc = proc.to(DEV)
    M = 64
    ei = torch.stack([torch.arange(M), (torch.arange(M) + 1) % M]).to(DEV)
    ea = torch.randn(M, 32, device=DEV)
    x = torch.randn(3 * M, 32, device=DEV)
    draws, call = [], proc.thermalizer.forward

    def keep(*a, **k):  # every sample's noise, not just the last one's
        y = call(*a, **k)
        draws.append(proc.thermalizer.last_noise)
        return y

    proc.thermalizer.forward = keep
    with torch.no_grad(), pytest.warns(UserWarning):
        plain = proc(x, ei, ea, t=500, batch_size=3, efficient_batching=True)
    assert len(draws) == 3  # one image per sample
    with torch.no_grad():
        base = proc.graph_processor(x, torch.cat([ei + i * M for i in range(3)], 1), ea.repeat(3, 1))[0][:, :32]
    sd = _sd64(proc.thermalizer, "score_model.")
    for i in range(3):
        ref = to.thermalize(sd, base[i * M:(i + 1) * M].double(), draws[i], 500, 1, 8, 8)
        assert _rel(plain[i * M:(i + 1) * M], ref) <= 1e-4, i


def test_wide_forecaster_forward_and_backward():
    """The 1024-wide widths of the reference's train/run.py (605 + 40 -> 605 features; two blocks keep the fp64 oracle small)
    at B=1: ThermalizerLayer(1024), Cin 1026, on a (1, 5 882) strip through the wide path, forward and every gradient."""
    model = gw.GraphWeatherForecaster(regular_lat_lons(10.0), edge_dim=1024, hidden_dim_processor_edge=1024, node_dim=1024,
                                      hidden_dim_processor_node=1024, hidden_dim_decoder=1024, feature_dim=605, aux_dim=40,
                                      num_blocks=2, use_thermalizer=True)
    deterministic_fill_(model, seed=6)
    to.fill_(model.processor.thermalizer, 6)
    model = model.to(DEV)
    th = model.processor.thermalizer
    feats = seeded_features(1, 648, 645, seed=13)
    target = seeded_features(1, 648, 605, seed=14).to(DEV)
    with pytest.warns(UserWarning):
        y = model(feats.to(DEV), t=500)
    ((y - target) ** 2).mean().backward()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = model.encoder.graphs.as_oracle_dict()
    with torch.device(DEV):
        p = params_on(sd, DEV, torch.float64, requires_grad=True)
        gg = graphs_on(g, DEV, torch.float64)
        f = feats.to(DEV, torch.float64)
        x, ei, ea = om.encoder_forward(p, gg, f)
        xp = om.processor_forward(p, x, ei, ea)
        H, W = gw.thermalizer.infer_grid_dimensions(int(xp.shape[0]))
        assert (H, W) == (1, 5882)
        xt = to.thermalize(to.strip(p, "processor.thermalizer.score_model."), xp, th.last_noise, 500, 1, H, W)
        ref = om.decoder_forward(p, gg, xt, f[..., :605])
        ((ref - target.double()) ** 2).mean().backward()
    scale = (ref - f[..., :605]).abs().max().item()
    assert (y.double() - ref).abs().max().item() <= 2e-4 * scale
    floor = _grad_floor([v.grad for v in p.values()])
    bad = {}
    for k, prm in model.named_parameters():
        if prm.grad is None:  # the UNet branch: a (1, N) strip runs simple_net
            assert k.startswith("processor.thermalizer.score_model.") and ".simple_net." not in k, k
            continue
        # the thermalizer holds the 2e-3 bar; the wide path's own layers hold theirs (4e-3, test_gpu_wide.py)
        bar = 2e-3 if k.startswith("processor.thermalizer.") else 4e-3
        err = _rel(prm.grad, p[k].grad, floor)
        if not err <= bar:
            bad[k] = err
    assert not bad, bad
