"""EnsembleCRPSLoss on the GPU (csrc/gw_crps.hip) against the broadcasting restatement in float64 (tests/crps_oracle.py).

The project's bar, as ``_bar`` of tests/test_gpu_fgn.py applies it: the yardstick is the float32 CPU restatement's own error against
float64 on the same case, the kernels may err at most 4 x that, with a floor of 1e-6 of the result's maximum.  The gradient is a sum
of signs times two coefficients, so the yardstick is often zero there and the floor decides.  Where the claim is "the same
arithmetic" - repeated runs, graph replay, a repeated training step, the tied terms - the test asks for bitwise equality.  Every
figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import graph_weather_amd as gw
from graph_weather_amd import ops
from graph_weather_amd.losses import EnsembleCRPSLoss

from . import crps_oracle as co
from . import gencast_model_oracle as mo
from .cafa_oracle import fill_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REG = ops.CRPS_REGISTER_MEMBERS

# (B, N, lon, lat, C).  45 elements per sample take the scalar tail; REG and REG + 1 sit on either side of the register bound; 70
# members take the general kernels; the last has 258 slabs of 4096 elements, more than the 256 threads of the final kernel.
SHAPES = [(1, 2, 4, 3, 1), (2, 3, 5, 3, 3), (1, 5, 12, 7, 5), (2, REG, 9, 5, 3), (2, REG + 1, 9, 5, 3), (1, 70, 6, 4, 2),
          (1, 2, 129, 64, 128)]
ALPHAS = [1.0, 0.95, 0.0]
WEIGHTS = ["absent", "lat", "features", "both"]


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


def _weights(kind, nlat, nvar, rs):
    lat = torch.linspace(-88.0, 88.0, nlat) if kind in ("lat", "both") else None
    fw = torch.from_numpy(rs.uniform(0.25, 2.0, nvar).astype(np.float32)) if kind in ("features", "both") else None
    return lat, fw


def _on_device(pred, target, strided):
    """The operands on the device; ``strided``: pred with the member axis innermost in memory and target inside a wider tensor."""
    if not strided:
        return pred.to(DEV), target.to(DEV)
    p = pred.permute(0, 2, 3, 4, 1).contiguous().to(DEV).permute(0, 4, 1, 2, 3)
    wide = torch.full(tuple(target.shape[:-1]) + (target.shape[-1] + 3,), float("nan"), device=DEV)
    wide[..., 1:1 + target.shape[-1]] = target.to(DEV)
    t = wide[..., 1:1 + target.shape[-1]]
    assert not p.is_contiguous() and not t.is_contiguous()
    return p, t


def _gpu(crit, pred_d, target_d, dout=None):
    x = pred_d.detach().requires_grad_(True)
    out = crit(x, target_d)
    if out.dim() == 0:
        out.backward()
    else:
        out.backward(dout.to(DEV))
    return out.detach(), x.grad


def _check(what, pred, target, lat, fw, alpha, strided=False):
    """Value and dpred of both reductions against the oracle under the bar; returns {reduction: (value, dpred)} as the device gave them."""
    rs = np.random.RandomState(99)
    dout = _randn(rs, *target.shape)
    pd, td = _on_device(pred, target, strided)
    res = {}
    for reduction in ("mean", "none"):
        crit = EnsembleCRPSLoss(grid_lat=lat, features_weights=fw, alpha=alpha, reduction=reduction).to(DEV)
        ref, gref = co.loss_and_grad(pred, target, lat, fw, alpha, reduction, torch.float64, dout)
        yard, gyard = co.loss_and_grad(pred, target, lat, fw, alpha, reduction, torch.float32, dout)
        out, grad = _gpu(crit, pd, td, dout)
        with torch.no_grad():
            plain = crit(pd, td)
        torch.cuda.synchronize()
        assert out.shape == ref.shape and out.dtype == torch.float32 and grad.shape == pred.shape
        assert torch.equal(plain, out)  # the no-grad forward is the training forward
        _bar("%s %s value" % (what, reduction), out, ref, yard)
        _bar("%s %s dpred" % (what, reduction), grad, gref, gyard)
        res[reduction] = (out, grad)
    return res


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_value_and_gradient_against_float64(case, alpha):
    B, N, nlon, nlat, nvar = SHAPES[case]
    rs = np.random.RandomState(100 + case)
    pred, target = _randn(rs, B, N, nlon, nlat, nvar), _randn(rs, B, nlon, nlat, nvar)
    for kind in WEIGHTS:
        lat, fw = _weights(kind, nlat, nvar, rs)
        _check("%s alpha %g weights %s" % (SHAPES[case], alpha, kind), pred, target, lat, fw, alpha, strided=case % 2 == 1)


def test_one_member_is_the_absolute_error():
    rs = np.random.RandomState(7)
    pred, target = _randn(rs, 1, 1, 4, 3, 2), _randn(rs, 1, 4, 3, 2)
    for kind in WEIGHTS:
        lat, fw = _weights(kind, 3, 2, rs)
        res = _check("(1, 1, 4, 3, 2) alpha 0 weights %s" % kind, pred, target, lat, fw, 0.0)
        if kind == "absent":
            assert torch.equal(res["none"][0].cpu(), (pred[:, 0] - target).abs())
    with pytest.raises(ValueError, match="at least two ensemble members"):
        EnsembleCRPSLoss().to(DEV)(pred.to(DEV), target.to(DEV))


def test_target_gets_no_gradient():
    pred, target = torch.zeros(1, 2, 4, 3, 2, device=DEV), torch.zeros(1, 4, 3, 2, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient for target"):
        EnsembleCRPSLoss()(pred, target)
    with torch.no_grad():
        assert EnsembleCRPSLoss()(pred, target).item() == 0.0


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N", [3, REG + 2])
def test_ties_contribute_exactly_zero(N, alpha):
    """Member 1 a copy of member 0; target[0] a copy of member 2 of sample 0; sample 2 has every member on the truth.  dpred agrees
    with the oracle, and without weights and with dout = 1 it is bitwise (1/N) sign(x_i - y) - 2 c2 sum_j sign(x_i - x_j) with
    sign(0) = 0, each product and the difference rounded once."""
    rs = np.random.RandomState(17)
    pred, target = _randn(rs, 3, N, 5, 3, 3), _randn(rs, 3, 5, 3, 3)
    pred[:, 1] = pred[:, 0]
    target[0] = pred[0, 2]
    pred[2] = target[2][None]
    lat, fw = _weights("both", 3, 3, rs)
    _check("ties N %d alpha %g" % (N, alpha), pred, target, lat, fw, alpha)
    crit = EnsembleCRPSLoss(alpha=alpha, reduction="none").to(DEV)
    out, grad = _gpu(crit, pred.to(DEV), target.to(DEV), torch.ones_like(target))
    torch.cuda.synchronize()
    out, grad = out.cpu(), grad.cpu()
    inv_n, two_c2 = np.float32(1.0 / N), np.float32(2.0 * co.c2(N, alpha))
    x, y = pred.numpy(), target.numpy()[:, None]
    s_y = np.sign(x - y).astype(np.float32)
    cnt = np.sign(x[:, :, None] - x[:, None]).sum(2).astype(np.float32)
    want = inv_n * s_y - two_c2 * cnt  # float32 throughout: one rounding per product, one for the difference
    assert want.dtype == np.float32 and np.array_equal(grad.numpy(), want)
    assert torch.equal(grad[:, 0], grad[:, 1])                                    # tied members get the same gradient
    assert np.array_equal(grad[0, 2].numpy(), -two_c2 * cnt[0, 2])                # on the truth: the pairwise term alone
    assert (grad[2] == 0).all() and (out[2] == 0).all()                           # everything tied: exactly nothing
    assert (s_y[0, 2] == 0).all() and (cnt[2] == 0).all() and (cnt[:, 0] == cnt[:, 1]).all()


@pytest.mark.parametrize("N", [4, 16])
def test_offset_data_keeps_the_direct_form_accuracy(N):
    """Members 280 + N(0, 1), a temperature field that is not normalised: the direct differences are exact in float32 where the
    sorted form sum_k (2k - N + 1) x_(k) loses five digits to the offset (1.3e-5 per point against 1.6e-7)."""
    rs = np.random.RandomState(23 + N)
    pred = (280.0 + rs.standard_normal((2, N, 9, 5, 3))).astype(np.float32)
    target = (280.0 + rs.standard_normal((2, 9, 5, 3))).astype(np.float32)
    pred, target = torch.from_numpy(pred), torch.from_numpy(target)
    _check("offset data N %d" % N, pred, target, None, None, 1.0)


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("case", [1, 3, 4, 6])
def test_forward_and_backward_are_bitwise_repeatable(case, reduction):
    B, N, nlon, nlat, nvar = SHAPES[case]
    rs = np.random.RandomState(31 + case)
    pred, target, dout = _randn(rs, B, N, nlon, nlat, nvar).to(DEV), _randn(rs, B, nlon, nlat, nvar).to(DEV), _randn(rs, B, nlon, nlat, nvar)
    lat, fw = _weights("both", nlat, nvar, rs)
    crit = EnsembleCRPSLoss(grid_lat=lat, features_weights=fw, alpha=0.95, reduction=reduction).to(DEV)
    a, b = _gpu(crit, pred, target, dout), _gpu(crit, pred, target, dout)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_mean_is_the_average_of_the_field(case):
    B, N, nlon, nlat, nvar = SHAPES[case]
    rs = np.random.RandomState(41 + case)
    pred, target = _randn(rs, B, N, nlon, nlat, nvar), _randn(rs, B, nlon, nlat, nvar)
    lat, fw = _weights("both", nlat, nvar, rs)
    with torch.no_grad():
        mean = EnsembleCRPSLoss(lat, fw, 0.95, "mean").to(DEV)(pred.to(DEV), target.to(DEV))
        none = EnsembleCRPSLoss(lat, fw, 0.95, "none").to(DEV)(pred.to(DEV), target.to(DEV))
    torch.cuda.synchronize()
    yard = (co.loss(pred, target, lat, fw, 0.95, dtype=torch.float32).double() - co.loss(pred, target, lat, fw, 0.95)).abs().item()
    average = none.cpu().double().mean().item()
    err, bar = abs(mean.item() - average), max(4.0 * yard, 1e-6 * abs(average))
    print("%s: mean %.9g, float64 average of the field %.9g, difference %.3e, yardstick %.3e, bar %.3e" % (SHAPES[case], mean.item(), average, err, yard, bar))
    assert err <= bar


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("N", [4, REG + 1])
def test_no_grad_forward_replays_in_a_hip_graph(N, reduction):
    rs = np.random.RandomState(53)
    shape = (2, N, 12, 7, 4)
    pred, target = _randn(rs, *shape).to(DEV), _randn(rs, 2, 12, 7, 4).to(DEV)
    lat, fw = _weights("both", 7, 4, rs)
    crit = EnsembleCRPSLoss(lat, fw, 0.95, reduction).to(DEV)
    with torch.no_grad():
        first = crit(pred, target)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = crit(pred, target)
    p2, t2 = _randn(rs, *shape).to(DEV), _randn(rs, 2, 12, 7, 4).to(DEV)
    pred.copy_(p2), target.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = crit(p2, t2)
    assert torch.equal(y, eager) and torch.isfinite(y).all() and not torch.equal(eager, first)


def test_no_grad_forward_writes_nothing_of_ensemble_size():
    B, N, nlon, nlat, nvar = 2, 8, 64, 32, 16
    rs = np.random.RandomState(59)
    pred, target = _randn(rs, B, N, nlon, nlat, nvar).to(DEV), _randn(rs, B, nlon, nlat, nvar).to(DEV)
    for reduction, most in (("mean", 8 * B * 8 + 1024), ("none", target.numel() * 4 + 1024)):
        crit = EnsembleCRPSLoss(reduction=reduction).to(DEV)
        with torch.no_grad():
            crit(pred, target)  # the library is loaded before the measured call
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = crit(pred, target)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        print("no-grad forward, reduction %s: allocation peak %d bytes (pred %d, target %d)" % (reduction, peak, pred.numel() * 4, target.numel() * 4))
        assert peak <= most < pred.numel() * 4
        del out


def test_fgn_trains_on_the_loss():
    """The smallest FGN of tests/test_fgn_host.py, B = 2, N = 3: the loss and the gradient that reaches the model's output against the
    oracle on that output, then one AdamW step; the same step from the same state gives bitwise equal parameters."""
    from graph_weather_amd.fgn import FunctionalGenerativeNetwork

    lon, lat = mo.GRIDS["gencast_model_a"]()
    model = FunctionalGenerativeNetwork(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, noise_dimension=4,
                                        hidden_dims=[8, 8], num_blocks=1, splits=1, num_hops=1)
    fill_(model, seed=3)
    model = model.to(DEV).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    rs = np.random.RandomState(67)
    x, noise, target = _randn(rs, 2, len(lon), len(lat), 3).to(DEV), _randn(rs, 2, 3, 4).to(DEV), _randn(rs, 2, len(lon), len(lat), 2)
    grid_lat = torch.as_tensor(np.asarray(lat), dtype=torch.float32)
    crit = EnsembleCRPSLoss(grid_lat=grid_lat).to(DEV)

    def step():
        model.load_state_dict(state)
        opt = gw.AdamW(model.parameters(), lr=1e-3)
        opt.zero_grad(set_to_none=True)
        out = model(x, num_ensemble=3, noise_vectors=noise)
        out.retain_grad()
        loss = crit(out, target.to(DEV))
        loss.backward()
        grads = [p.grad.clone() for p in model.parameters()]
        opt.step()
        return loss.detach(), out.detach(), out.grad, grads, [p.detach().clone() for p in model.parameters()]

    loss, out, dout, grads, new = step()
    loss2, out2, dout2, grads2, new2 = step()
    torch.cuda.synchronize()
    model.load_state_dict(state)
    assert out.shape == (2, 3, len(lon), len(lat), 2)
    ref, gref = co.loss_and_grad(out.cpu(), target, grid_lat, None, 1.0, "mean", torch.float64)
    yard, gyard = co.loss_and_grad(out.cpu(), target, grid_lat, None, 1.0, "mean", torch.float32)
    _bar("FGN loss", loss, ref, yard)
    _bar("FGN d output", dout, gref, gyard)
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max().item() > 0 for g in grads)
    moved = [not torch.equal(p, state[k]) for (k, _), p in zip(model.named_parameters(), new)]
    assert any(moved)
    assert torch.equal(loss, loss2) and torch.equal(out, out2) and torch.equal(dout, dout2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)) and all(torch.equal(a, b) for a, b in zip(new, new2))
