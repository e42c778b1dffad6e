"""GenCast's inverse spherical-harmonic transform (csrc/gw_sht.hip), isotropic noise, Sampler and WeightedMSELoss on the GPU.

Everything is measured against the float64 restatements of tests/gencast_sampler_oracle.py under the bar of
tests/test_gpu_gencast_model.py: the yardstick is the float32 CPU restatement's own error against float64 on the same case, the
kernels may err at most 4 x that, with a floor of 1e-6 of the result's maximum.  The reference's recorded results (tests/golden,
written by scripts/gen_gencast_sampler_golden.py) are held to the same bar.  Where the claim is "the same arithmetic" - repeated
calls, ignored imaginary parts, equal seeds, an ensemble against its members - the test asks for bitwise equality.  Every figure
is printed before it is asserted.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from graph_weather_amd import ops
from graph_weather_amd.gencast_model import Denoiser, generate_isotropic_noise
from graph_weather_amd.gencast_sampler import Sampler, WeightedMSELoss

from . import gencast_model_oracle as mo
from . import gencast_sampler_oracle as so
from .cafa_oracle import fill_, params
from .test_gpu_gencast_model import _bar

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _complex(seed, *shape):
    return torch.randn(*shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# the inverse transform, through generate_isotropic_noise with injected coefficients
# ---------------------------------------------------------------------------------------------------------------------
# (nlon, nlat, fields): 132 x 66 has lmax 66 and mmax 67 across the 64-wide tile and the row padding, 17 fields across the 16-field
# accumulator block (34 with batch = 2: across the 32-field tile); 128 x 65 is the 2 (nlat - 1) form with lmax exactly 64
ISHT_CASES = [(8, 4, 1), (12, 7, 2), (16, 9, 5), (132, 66, 17), (128, 65, 3)]


@pytest.mark.parametrize("batch", [None, 2], ids=["no_batch", "batch2"])
@pytest.mark.parametrize("nlon,nlat,fields", ISHT_CASES)
def test_inverse_transform_against_float64(nlon, nlat, fields, batch):
    lmax = so.lmax_of(nlat, nlon)
    n = fields * (batch or 1)
    c = _complex(400 + nlat + n, n, lmax, lmax + 1)
    ref, yard = (so.isotropic_noise(c, nlon, nlat, dt) for dt in (torch.float64, torch.float32))  # [lon, lat, n]
    if batch:  # field b * fields + ch -> [b, lon, lat, ch]
        ref, yard = (t.reshape(nlon, nlat, batch, fields).permute(2, 0, 1, 3) for t in (ref, yard))
    cd = c.to(DEV)
    got = generate_isotropic_noise(nlon, nlat, fields, device=DEV, batch=batch, coeffs=cd)
    again = generate_isotropic_noise(nlon, nlat, fields, device=DEV, batch=batch, coeffs=cd)
    # irfft ignores the imaginary parts of m = 0 and m = nlon / 2 (the last order): so does the kernel
    c2 = c.clone()
    c2[:, :, 0] += 3.0j
    c2[:, :, nlon // 2] -= 2.0j
    ignored = generate_isotropic_noise(nlon, nlat, fields, device=DEV, batch=batch, coeffs=c2.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == ((batch, nlon, nlat, fields) if batch else (nlon, nlat, fields)) and got.dtype == torch.float32
    assert got.is_contiguous()
    _bar("isht %d x %d, %d fields, batch %s" % (nlon, nlat, fields, batch), got, ref, yard)
    assert torch.equal(got, again), "two calls differ"
    assert torch.equal(got, ignored), "the imaginary parts of m = 0 and m = nlon / 2 are not ignored"


def test_transform_alone_with_a_scale():
    c = _complex(431, 6, 8, 9)
    ref, yard = (2.5 * so.isht(c, 9, 16, dt).reshape(2, 3, 9, 16).permute(0, 3, 2, 1) for dt in (torch.float64, torch.float32))
    got = ops.isht_forward(c.to(DEV), 9, 16, 3, 2.5)
    assert got.shape == (2, 16, 9, 3)
    _bar("isht_forward scale 2.5", got, ref, yard)
    with pytest.raises(RuntimeError, match="expects coefficients"):
        ops.isht_forward(c.to(DEV), 9, 16, 4)


# ---------------------------------------------------------------------------------------------------------------------
# noise statistics
# ---------------------------------------------------------------------------------------------------------------------
def test_noise_variance_per_grid_point():
    """4096 samples on the 16 x 9 grid, drawn on the device.  The sample variance (4095 degrees of freedom) of a Gaussian has
    relative standard deviation sqrt(2 / 4095); 6 of them over 144 grid points.  The exact variance comes from the oracle's linear
    map in float64 (it is not 1 and differs at the poles: that is the formula's business, not a tolerance)."""
    n = 4096
    noise = generate_isotropic_noise(16, 9, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    same = generate_isotropic_noise(16, 9, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    other = generate_isotropic_noise(16, 9, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    flat = generate_isotropic_noise(16, 9, 5, isotropic=False, device=DEV, batch=2)
    torch.cuda.synchronize()
    assert noise.shape == (16, 9, n) and flat.shape == (2, 16, 9, 5)
    assert torch.equal(noise, same) and not torch.equal(noise, other)
    var = noise.cpu().double().var(dim=-1, unbiased=True)
    want = so.noise_variance(16, 9)
    dev = ((var - want).abs() / want).max().item()
    allowed = 6 * math.sqrt(2 / (n - 1))
    print("noise variance: largest relative deviation %.4f, allowed %.4f; exact variance %.4f at the pole, %.4f at the equator; "
          "largest |mean| %.4f" % (dev, allowed, want[0, 0], want[0, 4], noise.cpu().double().mean(-1).abs().max()))
    assert dev <= allowed


# ---------------------------------------------------------------------------------------------------------------------
# the combine kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 1027])
def test_combine_against_float64(n):
    rs = np.random.RandomState(500 + n)
    x, y, z = (torch.from_numpy(rs.standard_normal(n + 1).astype(np.float32)) for _ in range(3))
    a, b, c = 0.75, -1.3125, 2.2
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    for off in (0, 1):  # off = 1: views that are not 16-byte aligned take the scalar path
        ops_ = {k: v[off:off + n] for k, v in (("x", x), ("y", y), ("z", z))}
        for use in (("x", "y", "z"), ("y", "z"), ("x", "z"), ("x", "y"), ("x",), ("y",), ("z",)):
            coef = dict(x=a, y=b, z=c)
            ref = sum(float(f32(coef[k])) * ops_[k].double() for k in use)
            yard = sum(f32(coef[k]) * ops_[k] for k in use)
            dev = {k: (v.to(DEV)[off:off + n] if k in use else None) for k, v in (("x", x), ("y", y), ("z", z))}
            out = torch.full((n + 1,), 7.0, device=DEV)[off:off + n]
            ops.sampler_combine(out, a, dev["x"], b, dev["y"], c, dev["z"])
            what = "combine n %d offset %d operands %s" % (n, off, "".join(use))
            _bar(what, out, ref, yard)
            if "x" in use:  # out is x
                alias = dev["x"].clone() if off == 0 else x.to(DEV)[off:off + n]
                ops.sampler_combine(alias, a, alias, b, dev["y"], c, dev["z"])
                assert torch.equal(alias, out), what + " aliased"


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


def _setup(golden_dir):
    """(model on the device, oracle closure, the fixture, the recorded draws), once."""
    if not _STATE:
        name = so.SAMPLER_CASE
        cpu = fill_(Denoiser(**mo.case_kwargs(name)), mo.CASES[name][3])
        graphs = mo.graph_tables(cpu)
        fns = {dt: so.denoiser_fn(params(cpu, dt), mo.CASES[name][0], mo.cast_graphs(graphs, dt)) for dt in (torch.float64, torch.float32)}
        g = np.load(os.path.join(golden_dir, "gencast_sampler_b.npz"))
        draws = [torch.view_as_complex(torch.from_numpy(d).contiguous()) for d in g["draws"]]
        prev, cache = so.sampler_prev_inputs(), {}

        def oracle(**kw):
            """(float64, float32) restatement on the fixture's inputs and its first num_steps draws."""
            key = tuple(sorted(kw.items()))
            if key not in cache:
                with torch.no_grad():
                    cache[key] = tuple(so.sampler_sample(fns[dt], prev, draws[:kw["num_steps"]], cpu.num_lon, cpu.num_lat, dt, **kw)
                                       for dt in (torch.float64, torch.float32))
            return cache[key]

        _STATE.update(model=cpu.to(DEV).eval(), oracle=oracle, golden=g, draws=draws, prev=prev,
                      prev_b=mo.case_inputs(name, batch=2)[1][1:2].clone(), draws_b=[_complex(600 + i, *draws[0].shape) for i in range(8)])
    return _STATE


def _sample(st, sampler, prev, draws):
    out = sampler.sample(st["model"], prev.to(DEV), coeffs=[d.to(DEV) for d in draws])
    torch.cuda.synchronize()
    return out


def test_sampler_against_the_fixture_and_float64(golden_dir):
    st = _setup(golden_dir)
    ref, yard = st["oracle"](**so.SAMPLER_KW)
    scale, yard_err = ref.abs().max().item(), (yard.double() - ref).abs().max().item()
    print("sampler fixture: maximum %.3e, float32 restatement error %.3e (%.2e of the maximum; recorded with the fixture: %.3e)"
          % (scale, yard_err, yard_err / scale, float(st["golden"]["restatement_error"])))
    assert yard_err <= 1e-3 * scale, "the trajectory is ill-conditioned: the bar would hide a failure"
    out = _sample(st, Sampler(**so.SAMPLER_KW), st["prev"], st["draws"])
    assert out.shape == (1, 16, 9, 5)
    _bar("sampler num_steps 5", out, ref, yard)
    want = torch.from_numpy(st["golden"]["out"]).double()
    fixture_err = (out.cpu().double() - want).abs().max().item()
    print("sampler against the reference's recorded output: %.3e (yardstick %.3e)" % (fixture_err, yard_err))
    assert fixture_err <= max(4.0 * yard_err, 1e-6 * scale)
    assert torch.equal(out, _sample(st, Sampler(**so.SAMPLER_KW), st["prev"], st["draws"]))


def test_ensemble_equals_its_members_bitwise(golden_dir):
    """B = 2 with coefficients [c_a; c_b] against the two B = 1 runs: bitwise.  The Denoiser's batch-shared kernels are tested
    bitwise against the replicated graph, the inverse transform and the combine kernel compute an element the same way wherever it
    sits, and the members share the host schedule."""
    st = _setup(golden_dir)
    sampler = Sampler(**so.SAMPLER_KW)
    da, db = st["draws"], st["draws_b"][:len(st["draws"])]
    a = _sample(st, sampler, st["prev"], da)
    b = _sample(st, sampler, st["prev_b"], db)
    both = _sample(st, sampler, torch.cat([st["prev"], st["prev_b"]]), [torch.cat([p, q]) for p, q in zip(da, db)])
    assert both.shape == (2, 16, 9, 5) and not torch.equal(a, b)
    diff = (both - torch.cat([a, b])).abs().max().item()
    print("ensemble B = 2 against its members: largest difference %.3e" % diff)
    assert torch.equal(both, torch.cat([a, b]))


@pytest.mark.parametrize("kw", [dict(num_steps=5, S_churn=0.0), dict(num_steps=2), dict(num_steps=3, r=0.4, S_noise=1.0)],
                         ids=["no_churn", "euler_only", "r_0.4"])
def test_sampler_branches(golden_dir, kw):
    st = _setup(golden_dir)
    draws = st["draws"][:kw["num_steps"]]
    ref, yard = st["oracle"](**kw)
    sampler = Sampler(**kw)
    gammas = sampler._schedule()[1]
    assert (max(gammas) == 0.0) == (kw.get("S_churn") == 0.0) and len(gammas) == kw["num_steps"] - 1
    out = _sample(st, sampler, st["prev"], draws)
    _bar("sampler %s" % kw, out, ref, yard)


def test_same_generator_seed_gives_the_same_sample(golden_dir):
    st = _setup(golden_dir)
    sampler, prev = Sampler(num_steps=3), torch.cat([st["prev"], st["prev_b"]]).to(DEV)
    outs = [sampler.sample(st["model"], prev, generator=torch.Generator(device=DEV).manual_seed(s)) for s in (3, 3, 4)]
    torch.cuda.synchronize()
    assert outs[0].shape == (2, 16, 9, 5) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0][0], outs[0][1])  # the members draw their own noise
    with pytest.raises(ValueError, match="coeffs must hold num_steps = 3 tensors"):
        sampler.sample(st["model"], prev, coeffs=[])
    with pytest.raises(ValueError, match="The shapes of the input tensors don't match"):
        sampler.sample(st["model"], prev[..., :5])


# ---------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(so.LOSS_CASES))
def test_loss_and_gradient_against_float64(golden_dir, name):
    kw, pred, sigma, target = so.loss_case(name)
    with open(os.path.join(golden_dir, "gencast_sampler.json")) as f:
        recorded = json.load(f)["loss"][name]
    res = {}
    for dt in (torch.float64, torch.float32):
        aw, fw = so.loss_weights(**kw, dtype=dt)
        p = pred.to(dt).clone().requires_grad_(True)
        value = so.weighted_mse_loss(p, sigma, target, aw, fw, dt)
        res[dt] = (value.detach(), torch.autograd.grad(value * 1.5, p)[0])
    (ref, gref), (yard, gyard) = res[torch.float64], res[torch.float32]
    loss = WeightedMSELoss(**kw).to(DEV)
    pd = pred.to(DEV).requires_grad_(True)
    value = loss(pd, sigma.to(DEV), target.to(DEV))
    (value * 1.5).backward()
    with torch.no_grad():
        plain = loss(pred.to(DEV), sigma.to(DEV), target.to(DEV))
    pd2 = pred.to(DEV).requires_grad_(True)
    value2 = loss(pd2, sigma.to(DEV), target.to(DEV))
    (value2 * 1.5).backward()
    torch.cuda.synchronize()
    assert value.shape == () and value.dtype == torch.float32
    err, yard_err = abs(value.item() - ref.item()), abs(yard.item() - ref.item())
    bar = max(4.0 * yard_err, 1e-6 * abs(ref.item()))
    rec_err = abs(value.item() - recorded)
    print("loss %s: ours %.9g, float64 %.9g, reference recorded %.9g; error %.3e, yardstick %.3e, bar %.3e; against recorded %.3e"
          % (name, value.item(), ref.item(), recorded, err, yard_err, bar, rec_err))
    assert err <= bar and rec_err <= bar
    _bar("loss %s dpred" % name, pd.grad, gref, gyard)
    assert torch.equal(value, plain) and torch.equal(value, value2) and torch.equal(pd.grad, pd2.grad)


def test_loss_raises_on_nan_and_on_target_gradients():
    kw, pred, sigma, target = so.loss_case("all_weights")
    loss = WeightedMSELoss(**kw).to(DEV)
    bad = pred.clone()
    bad[1, 11, 6, 4] = float("nan")  # the last element
    with pytest.raises(ValueError) as e:
        loss(bad.to(DEV), sigma.to(DEV), target.to(DEV))
    assert str(e.value) == "NaN values encountered in loss calculation."
    with pytest.raises(NotImplementedError, match="no gradient for target"):
        loss(pred.to(DEV), sigma.to(DEV), target.to(DEV).requires_grad_(True))
    assert torch.isfinite(loss(pred.to(DEV), sigma.to(DEV), target.to(DEV)))
