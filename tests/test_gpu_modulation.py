"""StochasticDecompositionLayer, FiLMGenerator and FiLMApplier on csrc/gw_modulate.hip.

Parity: every fixture of scripts/gen_modulation_golden.py (the reference's own fp32 output) against the fp64 restatement in
tests/modulation_oracle.py; the HIP result may be off the restatement by 4x what the reference itself is off (floor 2^-22): the
factor covers fma against separate rounding and the order of a short dot product.  Noise: the values against the numpy
restatement of eps(key, i) evaluated in fp64 (1e-5 absolute: about twice the bound of an fp32 evaluation with library-accurate
functions, 5.89 x (ulp(2 pi) / 2 + 3 ulp) = 4.5e-6) and five-sigma bounds on the moments at the 1 degree shape.  Gradients:
against fp64 autograd of the restatement under the very noise the layer drew; the yardstick is fp32 torch autograd of the same
composition on the CPU and the bar 8x its error (floor 1e-6) on max-abs over max |reference|.  No element is left out."""
import math
import os

import numpy as np
import pytest
import torch

import graph_weather_amd as gw
from graph_weather_amd import ops

from . import modulation_oracle as mo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ONE_DEGREE = (2, 78, 180, 360)
LATENT = (2, 256, 5882)


def _err(a, ref):
    return (a.detach().cpu().double() - ref).abs().max().item() / ref.abs().max().item()


def _golden(golden_dir, name):
    return torch.from_numpy(np.load(os.path.join(golden_dir, name + ".npz"))["out"])


def _check_parity(what, hip, ref, golden):
    e_hip, e_yard = _err(hip, ref), _err(golden, ref)
    print(f"modulation parity {what}: hip {e_hip:.3e} yardstick {e_yard:.3e}")
    assert hip.shape == golden.shape and hip.dtype == torch.float32 and hip.is_cuda
    assert e_hip <= max(4.0 * e_yard, 2.0 ** -22), (what, e_hip, e_yard)


# ---------------------------------------------------------------------------------------------------------------------
# parity with the reference's recorded outputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mo.SDL_CASES))
def test_sdl_parity(golden_dir, name):
    shape, latent, seed = mo.SDL_CASES[name]
    layer = mo.fill_(gw.StochasticDecompositionLayer(shape[1], latent), seed)
    x, z, noise = mo.sdl_inputs(shape, latent, seed)
    ref = mo.sdl(mo.params64(layer), x.double(), z.double(), noise.double())
    layer = layer.to(DEV)
    with torch.no_grad():
        out = layer(x.to(DEV), z.to(DEV), noise=noise.to(DEV))
    _check_parity(name, out, ref, _golden(golden_dir, name))


@pytest.mark.parametrize("name", sorted(mo.GENERATOR_CASES))
def test_film_generator_parity(golden_dir, name):
    n_lead, hidden, feat, batch, lead, seed = mo.GENERATOR_CASES[name]
    gen = mo.fill_(gw.FiLMGenerator(n_lead, hidden, feat), seed)
    ref = torch.stack(mo.film_generate(mo.params64(gen), batch, lead, feat))
    gen = gen.to(DEV)
    with torch.no_grad():
        gamma, beta = gen(batch, lead)
        g2, b2 = gen(batch, lead - n_lead, device=DEV)  # negative indices count from the end, as the reference's indexing does
    assert gamma.shape == beta.shape == (batch, feat)
    _check_parity(name, torch.stack([gamma, beta]), ref, _golden(golden_dir, name))
    assert torch.equal(g2, gamma) and torch.equal(b2, beta)


@pytest.mark.parametrize("name", sorted(mo.APPLIER_CASES))
def test_film_applier_parity(golden_dir, name):
    shape, seed = mo.APPLIER_CASES[name]
    x, gamma, beta = mo.applier_inputs(shape, seed)
    ref = mo.film_apply(x.double(), gamma.double(), beta.double())
    with torch.no_grad():
        out = gw.FiLMApplier()(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    _check_parity(name, out, ref, _golden(golden_dir, name))


def test_inputs_non_contiguous_and_wrong_dtype():
    layer = mo.fill_(gw.StochasticDecompositionLayer(8, 4), 1).to(DEV)
    g = torch.Generator().manual_seed(0)
    x, z, noise = torch.randn(2, 8, 6, 5, generator=g).to(DEV), torch.randn(2, 4, generator=g).to(DEV), torch.randn(2, 8, 6, 5, generator=g).to(DEV)
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    with torch.no_grad():
        assert torch.equal(layer(xt, z, noise=noise), layer(x, z, noise=noise))
        gamma, beta = torch.randn(2, 16, generator=g).to(DEV).chunk(2, dim=1)
        assert not gamma.is_contiguous()
        assert torch.equal(gw.FiLMApplier()(xt, gamma, beta), gw.FiLMApplier()(x, gamma.contiguous(), beta.contiguous()))
    with pytest.raises(TypeError):
        layer(x.half(), z)
    with pytest.raises(TypeError):
        layer(x, z.double())
    with pytest.raises(TypeError):
        gw.FiLMApplier()(x.double(), gamma, beta)
    with pytest.raises(ValueError):
        layer(x[:, :7], z)
    with pytest.raises(ValueError):
        layer(x, z, noise=noise[:, :, :5])


# ---------------------------------------------------------------------------------------------------------------------
# the noise
# ---------------------------------------------------------------------------------------------------------------------
def _noise_layer(channels, latent=4):
    """x = 0, alpha = 1, style_net = (0, 1): the output is the noise itself."""
    layer = gw.StochasticDecompositionLayer(channels, latent).to(DEV)
    with torch.no_grad():
        layer.alpha.fill_(1.0)
        layer.style_net.weight.zero_()
        layer.style_net.bias.fill_(1.0)
    return layer


def _draw(layer, shape, seed):
    """(key the layer drew, its output for x = 0) under torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    key = ops.sdl_key(DEV)
    torch.manual_seed(seed)
    with torch.no_grad():
        out = layer(torch.zeros(shape, device=DEV), torch.zeros(shape[0], layer.latent_dim, device=DEV))
    return key, out


# spatial a multiple of 4; not; element count not a multiple of 4; rows longer than a reduction chunk; scalar spatial
@pytest.mark.parametrize("shape", [(2, 3, 8), (2, 32, 16, 16), (2, 3, 7), (1, 5, 13, 5), (3, 7, 1), (1, 3, 4099), (2, 78, 12, 24)])
def test_noise_values(shape):
    layer = _noise_layer(shape[1])
    key, out = _draw(layer, shape, seed=sum(shape))
    noise = ops.sdl_noise(key, shape)
    assert torch.equal(noise, out)
    # the same values at any offset of a longer draw: a function of the key and the flat index only
    n = noise.numel()
    assert torch.equal(ops.sdl_noise(key, (n + 5,))[:n], noise.reshape(-1))
    ref = mo.eps(int(key.item()), n)
    err = np.abs(noise.cpu().numpy().astype(np.float64).reshape(-1) - ref).max()
    print(f"modulation noise {shape}: max |eps - fp64| {err:.3e}")
    assert err <= 1e-5, (shape, err)
    assert np.abs(ref).max() <= mo.EPS_MAX


def test_noise_values_at_one_degree():
    key = torch.tensor([-0x123456789ABCDEF], dtype=torch.int64, device=DEV)
    noise = ops.sdl_noise(key, ONE_DEGREE)
    ref = mo.eps(int(key.item()), noise.numel())
    err = np.abs(noise.cpu().numpy().astype(np.float64).reshape(-1) - ref).max()
    print(f"modulation noise {ONE_DEGREE}: max |eps - fp64| {err:.3e}")
    assert err <= 1e-5, err


def _moments(e):
    """The statistics of a [B, C, ...] draw in units of their five-sigma bounds (all must be <= 1)."""
    e = e.double()
    n = e.numel()
    flat = e.reshape(-1)
    rows = e.reshape(e.shape[0] * e.shape[1], -1)
    p = 0.0455003
    return {
        "mean": abs(flat.mean().item()) / (5.0 / math.sqrt(n)),
        "var": abs(flat.var(unbiased=False).item() - 1.0) / (5.0 * math.sqrt(2.0 / n)),
        "m4": abs((flat ** 4).mean().item() - 3.0) / (5.0 * math.sqrt(96.0 / n)),
        "lag1": abs((flat[1:] * flat[:-1]).mean().item()) / (5.0 / math.sqrt(n)),
        "rows": abs((rows[1:] * rows[:-1]).mean().item()) / (5.0 / math.sqrt(n)),
        "tail": abs((flat.abs() > 2.0).double().mean().item() - p) / (5.0 * math.sqrt(p * (1.0 - p) / n)),
    }


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noise_statistics(seed):
    layer = _noise_layer(ONE_DEGREE[1])
    _, out = _draw(layer, ONE_DEGREE, seed)
    m = _moments(out)
    print(f"modulation noise statistics seed {seed} (fractions of the five-sigma bounds): " + " ".join(f"{k} {v:.3f}" for k, v in m.items()))
    assert out.abs().max().item() <= mo.EPS_MAX + 1e-5
    for k, v in m.items():
        assert v <= 1.0, (seed, k, v)


def test_seeding_and_successive_calls():
    layer = mo.fill_(gw.StochasticDecompositionLayer(32, 16), 3).to(DEV)
    x, z, _ = (t.to(DEV) for t in mo.sdl_inputs((2, 32, 16, 16), 16, 5))
    with torch.no_grad():
        torch.manual_seed(42)
        a, a2 = layer(x, z), layer(x, z)
        torch.manual_seed(42)
        b = layer(x, z)
        torch.manual_seed(43)
        c = layer(x, z)
    assert torch.equal(a, b)                # the reference's test_reproducibility
    assert not torch.equal(a, a2) and not torch.equal(a, c)


def test_alpha_zero_is_the_identity():
    layer = gw.StochasticDecompositionLayer(78, 32).to(DEV)  # alpha is zero-initialised
    with torch.no_grad():
        layer.style_net.weight.normal_()
    x, z, _ = (t.to(DEV) for t in mo.sdl_inputs((2, 78, 12, 24), 32, 9))
    with torch.no_grad():
        assert torch.equal(layer(x, z), x)


def test_graph_replays_draw_fresh_noise():
    layer = _noise_layer(ONE_DEGREE[1])
    x = torch.zeros(ONE_DEGREE, device=DEV)
    z = torch.zeros(ONE_DEGREE[0], layer.latent_dim, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        layer(x, z)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = layer(x, z)
    graph.replay()
    a = out.clone()
    graph.replay()
    b = out.clone()
    assert not torch.equal(a, b)
    n = a.numel()
    for e in (a, b):
        m = _moments(e)
        print("modulation graph replay: mean %.3f var %.3f (fractions of the five-sigma bounds)" % (m["mean"], m["var"]))
        assert m["mean"] <= 1.0 and m["var"] <= 1.0
    # the two replays are independent draws
    assert abs((a.double() * b.double()).mean().item()) <= 5.0 / math.sqrt(n)


# ---------------------------------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------------------------------
def _check_grads(what, hip, ref, yard):
    for name in ref:
        e_hip, e_yard = _err(hip[name], ref[name]), _err(yard[name], ref[name])
        print(f"modulation gradient {what} {name}: hip {e_hip:.3e} yardstick {e_yard:.3e}")
        assert hip[name].shape == ref[name].shape
        assert e_hip <= max(8.0 * e_yard, 1e-6), (what, name, e_hip, e_yard)


def _upstream(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _sdl_grads_oracle(sd, x, z, noise, g, dtype):
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x, z = x.detach().to(dtype).clone().requires_grad_(True), z.detach().to(dtype).clone().requires_grad_(True)
    mo.sdl(sd, x, z, noise.to(dtype)).backward(g.to(dtype))
    out = {"x": x.grad, "z": z.grad}
    out.update({k: v.grad for k, v in sd.items()})
    return {k: v.double() for k, v in out.items()}


SDL_GRAD_SHAPES = [(s, l) for s, l, _ in mo.SDL_CASES.values()] + [(ONE_DEGREE, 32), (LATENT, 32), ((64, 16, 10), 8), ((3, 5, 67), 4)]


@pytest.mark.parametrize("shape,latent", SDL_GRAD_SHAPES)
def test_sdl_gradients(shape, latent):
    seed = sum(shape)
    layer = mo.fill_(gw.StochasticDecompositionLayer(shape[1], latent), seed)
    sd = mo.params64(layer)
    layer = layer.to(DEV)
    x, z, _ = mo.sdl_inputs(shape, latent, seed)
    g = _upstream(shape, seed + 2)

    def run():
        layer.zero_grad()
        xd, zd = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
        torch.manual_seed(seed)
        key = ops.sdl_key(DEV)
        torch.manual_seed(seed)
        out = layer(xd, zd)
        out.backward(g.to(DEV))
        grads = {"x": xd.grad, "z": zd.grad}
        grads.update({k: p.grad for k, p in layer.named_parameters()})
        return key, out.detach(), {k: v.clone() for k, v in grads.items()}

    key, out, hip = run()
    noise = ops.sdl_noise(key, shape).cpu()
    # the forward under the generated noise, against the restatement under the same noise
    ref_out = mo.sdl(sd, x.double(), z.double(), noise.double())
    yard_out = mo.sdl({k: v.float() for k, v in sd.items()}, x, z, noise)
    e_hip, e_yard = _err(out, ref_out), _err(yard_out, ref_out)
    print(f"modulation forward {shape}: hip {e_hip:.3e} yardstick {e_yard:.3e}")
    assert e_hip <= max(4.0 * e_yard, 2.0 ** -22)
    _check_grads(f"sdl {shape}", hip, _sdl_grads_oracle(sd, x, z, noise, g, torch.float64),
                 _sdl_grads_oracle(sd, x, z, noise, g, torch.float32))
    assert torch.equal(hip["x"].cpu(), g)  # the gradient of x is the incoming one
    # bitwise identical over two runs
    _, out2, hip2 = run()
    assert torch.equal(out, out2)
    for k in hip:
        assert torch.equal(hip[k], hip2[k]), k
    # a supplied noise tensor gives the same gradients as the key that generates it
    layer.zero_grad()
    xd, zd = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    layer(xd, zd, noise=noise.to(DEV)).backward(g.to(DEV))
    for name, got in (("z", zd.grad), ("alpha", layer.alpha.grad)):
        assert _err(got, hip[name].cpu().double()) <= 1e-6, name


def _film_grads_oracle(sd, x, lead, feat, g, dtype):
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = x.detach().to(dtype).clone().requires_grad_(True)
    gamma, beta = mo.film_generate(sd, x.shape[0], lead, feat)
    gamma.retain_grad()
    beta.retain_grad()
    mo.film_apply(x, gamma, beta).backward(g.to(dtype))
    out = {"x": x.grad, "gamma": gamma.grad, "beta": beta.grad}
    out.update({k: v.grad for k, v in sd.items()})
    return {k: v.double() for k, v in out.items()}


FILM_GRAD_SHAPES = [s for s, _ in mo.APPLIER_CASES.values()] + [ONE_DEGREE, LATENT, (64, 16, 10), (4, 16), (3, 5, 67)]


@pytest.mark.parametrize("shape", FILM_GRAD_SHAPES)
def test_film_gradients(shape):
    """Generator -> applier: gradients of x, gamma, beta and the generator's network.* parameters."""
    seed, n_lead, hidden, lead = sum(shape), 10, 32, 7
    feat = shape[1]
    gen = mo.fill_(gw.FiLMGenerator(n_lead, hidden, feat), seed)
    sd = mo.params64(gen)
    gen = gen.to(DEV)
    x = mo.applier_inputs(shape, seed)[0]
    g = _upstream(shape, seed + 2)

    def run():
        gen.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        gamma, beta = gen(shape[0], lead)
        gamma.retain_grad()
        beta.retain_grad()
        gw.FiLMApplier()(xd, gamma, beta).backward(g.to(DEV))
        grads = {"x": xd.grad, "gamma": gamma.grad, "beta": beta.grad}
        grads.update({k: p.grad for k, p in gen.named_parameters()})
        return {k: v.clone() for k, v in grads.items()}

    hip = run()
    _check_grads(f"film {shape}", hip, _film_grads_oracle(sd, x, lead, feat, g, torch.float64),
                 _film_grads_oracle(sd, x, lead, feat, g, torch.float32))
    hip2 = run()
    for k in hip:
        assert torch.equal(hip[k], hip2[k]), k


def test_film_gradients_of_leaf_gamma_and_beta_only():
    """x without a gradient: no dx is written, d_gamma and d_beta are unchanged."""
    shape = (2, 16, 8, 9)
    x, gamma, beta = (t.to(DEV) for t in mo.applier_inputs(shape, 4))
    g = _upstream(shape, 6).to(DEV)
    grads = []
    for need_x in (True, False):
        xd, gd, bd = x.clone().requires_grad_(need_x), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        gw.FiLMApplier()(xd, gd, bd).backward(g)
        grads.append((gd.grad, bd.grad))
        assert (xd.grad is not None) == need_x
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
