"""EnsembleCRPSLoss, the parts that need no GPU: the constructor and its buffers, every error, the C ABI's argument validation and
workspace size, and the oracle itself (tests/crps_oracle.py) against plain Python loops, hand values and the expected score of a
standard normal ensemble."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from graph_weather_amd import _lib

from . import crps_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gw_ensemble_crps_workspace_bytes", "gw_ensemble_crps_forward", "gw_ensemble_crps_backward")


# ---- public interface --------------------------------------------------------------------------------------------------------
def test_constructor_signature_and_buffers():
    import graph_weather_amd as gw
    from graph_weather_amd.losses import EnsembleCRPSLoss

    assert gw.EnsembleCRPSLoss is EnsembleCRPSLoss
    sig = inspect.signature(EnsembleCRPSLoss.__init__)
    assert [(n, p.default) for n, p in sig.parameters.items() if n != "self"] == [
        ("grid_lat", None), ("features_weights", None), ("alpha", 1.0), ("reduction", "mean")]
    assert list(inspect.signature(EnsembleCRPSLoss.forward).parameters) == ["self", "pred", "target"]

    plain = EnsembleCRPSLoss()
    assert plain.area_weights is None and plain.features_weights is None and plain.alpha == 1.0 and plain.reduction == "mean"
    assert plain.state_dict() == {}

    lat = torch.linspace(-90.0, 90.0, 7)
    fw = torch.tensor([1.0, 0.5, 2.0])
    crit = EnsembleCRPSLoss(grid_lat=lat, features_weights=fw, alpha=0.95, reduction="none")
    want = torch.abs(torch.cos(lat * np.pi / 180.0))
    want = want / torch.mean(want)
    assert torch.equal(crit.area_weights, want) and crit.area_weights.mean().item() == pytest.approx(1.0, abs=1e-6)
    assert torch.equal(crit.features_weights, fw) and crit.features_weights is not fw
    assert dict(crit.named_buffers()).keys() == {"area_weights", "features_weights"}
    assert crit.state_dict() == {}  # both are non-persistent
    assert crit.alpha == 0.95 and crit.reduction == "none"
    assert EnsembleCRPSLoss(grid_lat=lat).features_weights is None and EnsembleCRPSLoss(features_weights=fw).area_weights is None


def test_every_error_has_its_own_text():
    from graph_weather_amd.losses import EnsembleCRPSLoss

    with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\], got 1.5"):
        EnsembleCRPSLoss(alpha=1.5)
    with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\], got -0.1"):
        EnsembleCRPSLoss(alpha=-0.1)
    with pytest.raises(ValueError, match="reduction must be 'mean' or 'none', got 'sum'"):
        EnsembleCRPSLoss(reduction="sum")

    crit = EnsembleCRPSLoss(grid_lat=torch.linspace(-90.0, 90.0, 7), features_weights=torch.ones(5))
    pred, target = torch.zeros(2, 3, 12, 7, 5), torch.zeros(2, 12, 7, 5)
    seen = []
    with pytest.raises(ValueError, match=r"expected shape for predictions is \[batch, ensemble, lon, lat, var\]") as e:
        crit(pred[0], target)
    seen.append(str(e.value))
    for bad in (target[:1], target[:, :11], target[None], pred):
        with pytest.raises(ValueError, match="shape of the predictions without the ensemble axis") as e:
            crit(pred, bad)
    seen.append(str(e.value))
    with pytest.raises(ValueError, match="needs at least two ensemble members") as e:
        crit(pred[:, :1], target)
    seen.append(str(e.value))
    with pytest.raises(ValueError) as e:
        crit(pred[:, :, :, :6], target[:, :, :6])
    assert str(e.value) == "The size of grid_lat at initialization (7) and the number of latitudes in predictions (6) don't match."
    seen.append(str(e.value))
    with pytest.raises(ValueError) as e:
        crit(pred[..., :4], target[..., :4])
    assert str(e.value) == ("The size of features weights at initialization (5) and the number of features in predictions (4) "
                            "don't match.")
    seen.append(str(e.value))
    assert len(set(seen)) == len(seen)


def test_no_cpu_path_and_no_gradient_for_target():
    from graph_weather_amd import ops
    from graph_weather_amd.losses import EnsembleCRPSLoss

    pred, target = torch.zeros(2, 3, 12, 7, 5), torch.zeros(2, 12, 7, 5)
    for crit in (EnsembleCRPSLoss(), EnsembleCRPSLoss(alpha=0.0, reduction="none"),
                 EnsembleCRPSLoss(grid_lat=torch.linspace(-90.0, 90.0, 7), features_weights=torch.ones(5))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            crit(pred, target)
        with pytest.raises(RuntimeError, match="no CPU path"):
            crit(pred.clone().requires_grad_(True), target)
    with pytest.raises(RuntimeError, match="no CPU path"):  # one member is fine at alpha = 0: the device check is what stops it
        EnsembleCRPSLoss(alpha=0.0)(pred[:, :1], target)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ensemble_crps_forward(pred, target, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ensemble_crps_backward(pred, target, None, None, torch.ones(1))
    with pytest.raises(NotImplementedError, match="no gradient for target"):
        EnsembleCRPSLoss()(pred, target.clone().requires_grad_(True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):  # without grad mode a target's flag means nothing
        EnsembleCRPSLoss()(pred, target.clone().requires_grad_(True))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_names_in_exports_and_header():
    text = open(os.path.join(ROOT, "include", "gw_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+GW_CRPS_MEAN\s+0\b", text) and re.search(r"#define\s+GW_CRPS_NONE\s+1\b", text)
    assert (_lib.CRPS_MEAN, _lib.CRPS_NONE) == (0, 1)
    assert _lib.lib().gw_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("shape", [(1, 2, 4, 3, 1), (2, 3, 5, 3, 3), (2, 4, 360, 181, 83), (3, 70, 64, 64, 1), (1, 2, 128, 64, 128),
                                   (5, 1024, 1, 1, 4097)])
def test_workspace_bytes_closed_form(shape):
    """One fp64 partial sum per slab of 4096 elements of one sample: 8 B ceil(lon lat C / 4096), whatever the ensemble size."""
    b, n, nlon, nlat, nvar = shape
    assert _lib.lib().gw_ensemble_crps_workspace_bytes(*shape) == 8 * b * -(-(nlon * nlat * nvar) // 4096)


def test_argument_validation_without_gpu():
    L = _lib.lib()
    p = 256  # a non-null pointer: every call below fails its validation before anything is launched
    for shape in ((0, 2, 4, 3, 1), (1, 0, 4, 3, 1), (1, 2, 0, 3, 1), (1, 2, 4, 0, 1), (1, 2, 4, 3, 0), (1, -1, 4, 3, 1),
                  (1, 1025, 4, 3, 1), (1, 2, 1 << 16, 1 << 16, 1), (1, 2, 1 << 15, 1 << 15, 2)):
        assert L.gw_ensemble_crps_workspace_bytes(*shape) == 0 and b"gw_ensemble_crps_workspace_bytes" in L.gw_last_error(), shape
        assert L.gw_ensemble_crps_forward(*shape, 1.0, 0, p, p, None, None, p, 1 << 30, p, None) < 0, shape
        assert b"gw_ensemble_crps_forward" in L.gw_last_error()
        assert L.gw_ensemble_crps_backward(*shape, 1.0, 0, p, p, None, None, p, p, None) < 0, shape
        assert b"gw_ensemble_crps_backward" in L.gw_last_error()
    ok = (2, 3, 12, 7, 5)
    fwd = lambda alpha=1.0, red=0, pred=p, target=p, ws=p, ws_bytes=64, out=p, shape=ok: L.gw_ensemble_crps_forward(  # noqa: E731
        *shape, alpha, red, pred, target, None, None, ws, ws_bytes, out, None)
    bwd = lambda alpha=1.0, red=0, pred=p, target=p, dout=p, dpred=p, shape=ok: L.gw_ensemble_crps_backward(  # noqa: E731
        *shape, alpha, red, pred, target, None, None, dout, dpred, None)
    for kw in (dict(pred=None), dict(target=None), dict(out=None), dict(alpha=1.5), dict(alpha=-0.01), dict(alpha=float("nan")),
               dict(red=2), dict(red=-1), dict(shape=(2, 1, 12, 7, 5)), dict(shape=(2, 1, 12, 7, 5), alpha=0.5)):
        assert fwd(**kw) == -1 and b"gw_ensemble_crps_forward: bad arguments" in L.gw_last_error(), kw
    assert fwd(ws=None) == -1 and b"workspace" in L.gw_last_error()
    assert fwd(ws_bytes=8) == -1 and b"workspace" in L.gw_last_error()  # two samples, one slab each: 16 bytes
    for kw in (dict(pred=None), dict(target=None), dict(dout=None), dict(dpred=None), dict(alpha=2.0), dict(red=7),
               dict(shape=(2, 1, 12, 7, 5)), dict(red=1, dout=None)):
        assert bwd(**kw) == -1 and b"gw_ensemble_crps_backward: bad arguments" in L.gw_last_error(), kw


# ---- the oracle itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.95, 0.0])
def test_oracle_against_plain_python_loops(alpha):
    rs = np.random.RandomState(5)
    pred = torch.from_numpy(rs.standard_normal((2, 3, 2, 2, 2)))
    target = torch.from_numpy(rs.standard_normal((2, 2, 2, 2)))
    pred[0, 1, 0, 0, 0] = pred[0, 0, 0, 0, 0]  # a tie among members
    target[1, 1, 1, 1] = pred[1, 2, 1, 1, 1]   # and one with the truth
    want = co.triple_loop(pred, target, alpha)
    got = co.field(pred, target, alpha=alpha)
    assert (got - want).abs().max().item() <= 1e-15
    assert abs(co.loss(pred, target, alpha=alpha).item() - want.mean().item()) <= 1e-15
    lat, fw = [-60.0, 30.0], [2.0, 0.5]
    aw = np.abs(np.cos(np.float32(lat) * np.pi / 180.0)).astype(np.float32)
    aw = aw / aw.mean(dtype=np.float32)
    weighted = want * torch.from_numpy(aw.astype(np.float64))[None, None, :, None] * torch.tensor(fw, dtype=torch.float64)
    assert (co.field(pred, target, lat, fw, alpha) - weighted).abs().max().item() <= 1e-6 * weighted.abs().max().item()
    # the gradient: (1/N) sign(x_i - y) - 2 c2 sum_j sign(x_i - x_j), sign(0) = 0
    _, grad = co.loss_and_grad(pred, target, alpha=alpha, reduction="none")
    sign = lambda t: torch.sign(t)  # noqa: E731
    hand = sign(pred - target[:, None]) / 3 - 2 * co.c2(3, alpha) * sign(pred[:, :, None] - pred[:, None]).sum(2)
    assert (grad - hand).abs().max().item() <= 1e-15


def test_oracle_hand_values():
    pred, target = torch.tensor([1.0, 3.0]).reshape(1, 2, 1, 1, 1), torch.tensor([2.0]).reshape(1, 1, 1, 1)
    assert co.loss(pred, target, alpha=1.0).item() == 0.0       # 1 - 4 / (2 * 2 * 1)
    assert co.loss(pred, target, alpha=0.0).item() == 0.5       # 1 - 4 / (2 * 4)
    assert co.loss(pred, target, alpha=0.0, reduction="none").shape == (1, 1, 1, 1)
    assert co.loss(pred[:, :1], target, alpha=0.0).item() == 1.0  # one member: |x - y|
    assert co.c2(1, 1.0) == 0.0 and co.c2(4, 1.0) == 1 / 24 and co.c2(4, 0.0) == 1 / 32


@pytest.mark.parametrize("n", [2, 4, 16])
def test_fair_score_of_a_standard_normal_ensemble(n):
    """Members and truth iid N(0, 1): E|x - y| = 2 / sqrt(pi) and the fair score is unbiased in N, so its mean is 1 / sqrt(pi)."""
    rs = np.random.RandomState(11)
    pred = torch.from_numpy(rs.standard_normal((1, n, 200000, 1, 1)))
    target = torch.from_numpy(rs.standard_normal((1, 200000, 1, 1)))
    got = co.loss(pred, target, alpha=1.0).item()
    print("N = %d: mean fair CRPS %.5f, 1/sqrt(pi) %.5f" % (n, got, 1 / math.sqrt(math.pi)))
    assert abs(got - 1 / math.sqrt(math.pi)) <= 0.01
