"""StochasticDecompositionLayer / FiLMGenerator / FiLMApplier without a GPU: the numpy noise oracle against the published
Philox known answers, the fp64 restatement against the reference's recorded outputs, the alias import paths, state_dict
exchange with the reference's key -> shape tables, and the host-side errors."""
import json
import os

import numpy as np
import pytest
import torch

from . import modulation_oracle as mo
from .test_alias import alias_modules


def _words(hexes):
    return [int(h, 16) for h in hexes.split()]


@pytest.mark.parametrize("counter,key,expect", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    """The three known-answer vectors of philox4x32-10 published with Random123 (kat_vectors)."""
    out = mo.philox4x32_10(_words(counter), _words(key))
    assert [int(v) for v in out] == _words(expect)


def test_noise_oracle_is_a_function_of_key_and_index():
    a = mo.eps(0x0123456789ABCDEF, 1000)
    assert a.dtype == np.float64 and np.isfinite(a).all() and np.abs(a).max() <= mo.EPS_MAX
    # any window of the sequence, aligned to a group of four or not, is the same values
    for start, n in ((0, 7), (5, 13), (998, 2), (4, 4)):
        assert np.array_equal(mo.eps(0x0123456789ABCDEF, n, start), a[start:start + n])
    assert not np.array_equal(mo.eps(0x0123456789ABCDEE, 1000), a)
    # a signed int64 key (what the device tensor holds) is the same key modulo 2^64
    assert np.array_equal(mo.eps(-1, 8), mo.eps(2 ** 64 - 1, 8))
    # counter words: group 2^32 has counter (0, 1, 0, 0)
    w = mo.philox4x32_10((0, 1, 0, 0), mo.split_key(7))
    u = ((int(w[0]) >> 8) + 0.5) * 2.0 ** -24, ((int(w[1]) >> 8) + 0.5) * 2.0 ** -24
    assert mo.eps(7, 1, 4 * 2 ** 32)[0] == np.sqrt(-2.0 * np.log(u[0])) * np.cos(2.0 * np.pi * u[1])


def _golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    return g["meta"], torch.from_numpy(g["out"])


def _close_at_fp32_rounding(ref64, out32, terms):
    """The reference's fp32 result against the fp64 restatement: a few roundings of values of the output's scale (and of a
    dot product of ``terms`` terms where there is one)."""
    scale = ref64.abs().max().item()
    err = (out32.double() - ref64).abs().max().item() / scale
    assert err <= (4 + terms) * 2.0 ** -24, err


@pytest.mark.parametrize("name", sorted(mo.SDL_CASES))
def test_restatement_reproduces_reference_sdl(golden_dir, name):
    import graph_weather_amd as gw

    shape, latent, seed = mo.SDL_CASES[name]
    meta, out = _golden(golden_dir, name)
    assert list(meta) == list(shape) + [latent, seed] and tuple(out.shape) == tuple(shape)
    layer = mo.fill_(gw.StochasticDecompositionLayer(shape[1], latent), seed)
    x, z, noise = mo.sdl_inputs(shape, latent, seed)
    ref = mo.sdl(mo.params64(layer), x.double(), z.double(), noise.double())
    _close_at_fp32_rounding(ref, out, latent)
    assert (out - x).abs().max() > 0.1  # alpha is not zero: the noise term is in the fixture


@pytest.mark.parametrize("name", sorted(mo.GENERATOR_CASES))
def test_restatement_reproduces_reference_generator(golden_dir, name):
    import graph_weather_amd as gw

    n_lead, hidden, feat, batch, lead, seed = mo.GENERATOR_CASES[name]
    meta, out = _golden(golden_dir, name)
    assert list(meta) == [n_lead, hidden, feat, batch, lead, seed] and tuple(out.shape) == (2, batch, feat)
    gen = mo.fill_(gw.FiLMGenerator(n_lead, hidden, feat), seed)
    gamma, beta = mo.film_generate(mo.params64(gen), batch, lead, feat)
    _close_at_fp32_rounding(torch.stack([gamma, beta]), out, hidden)


@pytest.mark.parametrize("name", sorted(mo.APPLIER_CASES))
def test_restatement_reproduces_reference_applier(golden_dir, name):
    shape, seed = mo.APPLIER_CASES[name]
    meta, out = _golden(golden_dir, name)
    assert list(meta) == list(shape) + [seed] and tuple(out.shape) == tuple(shape)
    x, gamma, beta = mo.applier_inputs(shape, seed)
    _close_at_fp32_rounding(mo.film_apply(x.double(), gamma.double(), beta.double()), out, 0)


def test_alias_import_paths():
    import graph_weather_amd as gw

    with alias_modules():
        from graph_weather.models import StochasticDecompositionLayer
        from graph_weather.models.layers.film import FiLMApplier, FiLMGenerator
        from graph_weather.models.layers.stochastic_decomposition import StochasticDecompositionLayer as S2
    assert StochasticDecompositionLayer is S2 is gw.StochasticDecompositionLayer
    assert FiLMGenerator is gw.FiLMGenerator and FiLMApplier is gw.FiLMApplier


def test_reference_state_dicts_load_strict(golden_dir):
    """The reference's key -> shape tables load strict=True into our layers, and ours are exactly those tables, so the
    reference loads ours strict=True too."""
    import graph_weather_amd as gw

    with open(os.path.join(golden_dir, "modulation_state_dict.json")) as fh:
        tables = json.load(fh)
    assert len(tables) == 5
    for ctor, table in tables.items():
        module = eval(ctor, {"StochasticDecompositionLayer": gw.StochasticDecompositionLayer, "FiLMGenerator": gw.FiLMGenerator,
                             "FiLMApplier": gw.FiLMApplier})
        g = torch.Generator().manual_seed(3)
        sd = {k: torch.randn(*shape, generator=g) for k, shape in table.items()}
        res = module.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        ours = module.state_dict()
        assert list(ours) == list(table), ctor
        for k, v in ours.items():
            assert torch.equal(v, sd[k]), (ctor, k)


def test_constructor_attributes_and_initialisation():
    import graph_weather_amd as gw

    layer = gw.StochasticDecompositionLayer(32, 16)
    assert (layer.input_dim, layer.latent_dim) == (32, 16)
    assert layer.alpha.shape == (1, 32, 1) and not layer.alpha.detach().any()
    assert isinstance(layer.style_net, torch.nn.Linear) and layer.style_net.weight.shape == (32, 16)
    gen = gw.FiLMGenerator(10, 8, 16)
    assert (gen.num_lead_times, gen.feature_dim) == (10, 16)
    assert [type(m).__name__ for m in gen.network] == ["Linear", "ReLU", "Linear"]
    assert gen.network[0].weight.shape == (8, 10) and gen.network[2].weight.shape == (32, 8)
    assert not list(gw.FiLMApplier().parameters())


def test_no_cpu_path():
    import graph_weather_amd as gw

    layer = gw.StochasticDecompositionLayer(32, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.zeros(2, 32, 10), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        gw.FiLMApplier()(torch.zeros(2, 16, 4), torch.zeros(2, 16), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        gw.FiLMGenerator(10, 8, 16)(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gw.FiLMGenerator(10, 8, 16)(4, 3, device="cpu")


def test_errors_as_in_the_reference():
    import graph_weather_amd as gw

    layer = gw.StochasticDecompositionLayer(32, 16)
    with pytest.raises(ValueError, match="Expected 32 channels, got 31"):
        layer(torch.zeros(2, 31, 10), torch.zeros(2, 16))
    gen = gw.FiLMGenerator(10, 8, 16)
    for lead in (10, -11, 1000):
        with pytest.raises(IndexError):
            gen(4, lead)


def test_workspace_query_and_argument_checks_are_host_logic():
    from graph_weather_amd import _lib

    L = _lib.lib()
    # fp64: two planes of one partial per (row, chunk of 2048 elements) and one total per row; short rows are one chunk
    assert L.gw_modulate_workspace_bytes(156, 64800) == (2 * 156 * 32 + 156) * 8
    assert L.gw_modulate_workspace_bytes(1024, 10) == (2 * 1024 + 1024) * 8
    assert L.gw_modulate_workspace_bytes(512, 5882) == (2 * 512 * 3 + 512) * 8
    assert L.gw_modulate_workspace_bytes(0, 10) == 0 and b"bad arguments" in L.gw_last_error()
    assert L.gw_modulate_workspace_bytes(2 ** 31, 10) == 0 and b"2^31-1" in L.gw_last_error()
    assert L.gw_sdl_forward(4, 3, 10, 1, 1, 1, 1, None, 1, None) == -1      # rows not a multiple of channels
    assert L.gw_sdl_forward(4, 2, 10, 1, 1, 1, None, None, 1, None) == -1   # neither key nor noise
    assert L.gw_sdl_backward(4, 2, 10, 1, 1, 1, 1, None, None, 0, 1, 1, None) == -1  # no workspace
    assert b"workspace" in L.gw_last_error()
    assert L.gw_film_forward(4, 10, 1, None, 1, 1, None) == -1
    assert L.gw_film_backward(4, 10, 1, None, 1, 1, 8, 1, 1, 1, None) == -1  # d_gamma without x
