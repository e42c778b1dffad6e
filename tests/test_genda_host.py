"""The GenDA model without a GPU: the alias import paths, signatures, ``state_dict`` keys, order and shapes against what the
reference's own classes gave (tests/golden/genda_state_dict.json, scripts/gen_genda_golden.py), the error messages, the float64
restatement of ``forward`` and ``guided_forward`` (tests/genda_oracle.py) against every recorded reference output, and the argument
checks of the four new entry points."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from . import genda_oracle as do
from . import gencast_model_oracle as mo
from .cafa_oracle import fill_, params
from .test_alias import alias_modules
from .test_gencast_model_host import _sig

CASE_NAMES = tuple(do.CASES)
GW_E_BADARG = -1
NEW = ("gw_genda_input_forward", "gw_genda_input_backward", "gw_genda_guided_output_forward", "gw_genda_guided_output_backward")


@pytest.fixture(scope="module")
def tables(golden_dir):
    with open(os.path.join(golden_dir, "genda_state_dict.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models():
    """name -> our GenDA on the CPU with the case's seeded weights (built once)."""
    from graph_weather_amd.genda import GenDA

    return {name: fill_(GenDA(**do.case_kwargs(name)), do.CASES[name][4]).eval() for name in CASE_NAMES}


@pytest.fixture(scope="module")
def oracle64(models):
    """name -> (float64 parameters, keywords, float64 graphs, float64 inputs): shared, left unchanged."""
    out = {}
    for name in CASE_NAMES:
        m = models[name]
        out[name] = (params(m, torch.float64), do.CASES[name][1], mo.cast_graphs(mo.graph_tables(m), torch.float64),
                     tuple(t.double() for t in do.case_inputs(name)))
    return out


def test_alias_imports_give_the_genda_classes():
    from graph_weather_amd import genda

    with alias_modules():
        from graph_weather.models.genda import GenDA
        from graph_weather.models.genda.model import GenDA as G2, GenDAConfig
    assert GenDA is G2 is genda.GenDA and GenDAConfig is genda.GenDAConfig
    assert GenDA.__module__ == "graph_weather_amd.genda"


def test_signatures_equal_the_references(tables):
    from graph_weather_amd.genda import GenDA, GenDAConfig

    for cls in (GenDA, GenDAConfig):
        assert _sig(cls) == tables["signature"][cls.__name__], cls.__name__
    sig = dict((k, v) for k, v in _sig(GenDA))
    assert sig["hidden_dims"] == [512, 512] and sig["num_blocks"] == 16 and sig["conditioning_dim"] == 2 and sig["splits"] == 6
    assert "conditioning_dim" not in dict((k, v) for k, v in _sig(GenDAConfig))
    import inspect

    assert list(inspect.signature(GenDA.forward).parameters)[1:] == ["corrupted_targets", "prev_inputs", "noise_levels", "sensor_mask",
                                                                     "sensor_values", "wind_direction"]
    guided = inspect.signature(GenDA.guided_forward).parameters
    assert list(guided)[1:] == ["corrupted_targets", "prev_inputs", "noise_levels", "sensor_mask", "sensor_values", "gamma"]
    assert guided["gamma"].default == 2.0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_state_dict_keys_order_and_buffers(tables, models, name):
    m = models[name]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == tables["state_dict"][name]
    assert list(m.state_dict()) == list(tables["state_dict"][name])  # the order too
    kw = do.CASES[name][1]
    if name == "genda_model_a":
        assert len(m.state_dict()) == 98
    width = kw["output_features_dim"] + 2 * kw["input_features_dim"] + kw.get("conditioning_dim", 2) + m.graphs.grid_nodes_dim
    assert list(m.state_dict()["encoder.grid_mlp.linears.0.weight"].shape) == [kw["hidden_dims"][0], width]
    assert list(m._buffers) == tables["buffers"] and len(tables["buffers"]) == 14
    assert set(m._non_persistent_buffers_set) == set(tables["buffers"])
    assert (m.khop_mesh_edge_attr is None) == (not kw.get("use_edges_features", True))
    assert m.input_features_dim == kw["input_features_dim"] and m.output_features_dim == kw["output_features_dim"]
    assert m.use_edges_features == kw.get("use_edges_features", True)
    assert m.num_lon == len(do.case_kwargs(name)["grid_lon"]) and m.num_lat == len(do.case_kwargs(name)["grid_lat"])
    assert float(m.precs.sigma_data) == 1.0


def test_the_documented_small_model_has_the_issue_width():
    """Grid a, splits 1, in 3, out 2, hidden [16, 16], 2 blocks, 1 hop: 98 tensors, the encoder's first weight [16, 13]."""
    from graph_weather_amd.genda import GenDA

    lon, lat = mo.GRIDS["gencast_model_a"]()
    m = GenDA(lon, lat, input_features_dim=3, output_features_dim=2, hidden_dims=[16, 16], num_blocks=2, num_hops=1, splits=1)
    assert len(m.state_dict()) == 98 and list(m.state_dict()["encoder.grid_mlp.linears.0.weight"].shape) == [16, 13]


def test_config_builds_the_model_and_hub_mixin():
    from graph_weather_amd.genda import GenDA, GenDAConfig

    lon, lat = mo.GRIDS["gencast_model_a"]()
    cfg = GenDAConfig(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, splits=1, num_hops=1, num_blocks=1,
                      hidden_dims=[8, 8])
    assert GenDAConfig(lon, lat, 1, 1).hidden_dims == [512, 512]
    m = cfg.build()
    assert isinstance(m, GenDA) and len(m.processor.cond_transformers) == 1
    assert m.encoder.grid_mlp.linears[0].in_features == 2 + 6 + 2 + m.graphs.grid_nodes_dim  # the default conditioning_dim
    try:
        from huggingface_hub import PyTorchModelHubMixin
    except Exception:
        return
    assert isinstance(m, PyTorchModelHubMixin)


def test_error_messages(models):
    from graph_weather_amd.genda import GenDA, _forward_replicated

    lon, lat = mo.GRIDS["gencast_model_a"]()
    kw = dict(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, hidden_dims=[8, 8], num_blocks=1, splits=1, num_hops=1)
    with pytest.raises(ValueError, match="Sparse processor don't support edges features."):
        GenDA(sparse=True, **kw)
    with pytest.raises(ValueError, match="Please install DGL to use sparsity."):
        GenDA(sparse=True, use_edges_features=False, **kw)

    m = models["genda_model_a"]
    z, x, s, mask, values = do.case_inputs("genda_model_a")
    shape = (2, 12, 7, 1)
    with pytest.raises(ValueError) as err:
        m(z, x, s, mask[:, :, :5], values)
    assert str(err.value) == f"Expected sensor_mask shape {shape}"
    with pytest.raises(ValueError) as err:
        m(z, x, s, mask, values[..., 0])
    assert str(err.value) == f"Expected sensor_values shape {shape}"
    with pytest.raises(ValueError) as err:  # the mask's check comes first
        m(z[:1], x, s, mask[:1], values)
    assert str(err.value) == f"Expected sensor_mask shape {shape}"
    long = ("The shapes of the input tensors don't match with the initialization parameters: expected (2, 12, 7, 8) for prev_inputs, "
            "(2, 12, 7, 6) for targets and (2, 1) for noise_levels.")
    for bad in ((z[..., :5], x, s), (z, x, s[:, 0]), (z.transpose(1, 2), x, s)):
        with pytest.raises(ValueError) as err:
            m(*bad, mask, values)
        assert str(err.value) == long
        with pytest.raises(ValueError) as err:
            m.guided_forward(*bad, mask, values)
        assert str(err.value) == long
    with pytest.raises(ValueError) as err:  # the shapes come before the noise levels
        m(z[..., :5], x, -s, mask, values)
    assert str(err.value) == long
    with pytest.raises(ValueError) as err:
        m(z, x, -s, mask, values)
    assert str(err.value) == "All the noise levels must be strictly positive."
    with pytest.raises(ValueError) as err:
        m.guided_forward(z, x, torch.zeros_like(s), mask, values)
    assert str(err.value) == "All the noise levels must be strictly positive."
    # the count of conditioning tensors against conditioning_dim: this package's text, after the reference's own checks
    for sensors in ((), (mask,), (None, values)):
        with pytest.raises(ValueError, match=r"conditioning_dim=2 but %d conditioning tensor" % sum(t is not None for t in sensors)):
            m(z, x, s, *sensors)
    with pytest.raises(ValueError, match="All the noise levels must be strictly positive."):
        m(z, x, -s, mask)
    c = models["genda_model_c"]
    zc, xc, sc, maskc, valuesc = do.case_inputs("genda_model_c")
    with pytest.raises(ValueError, match=r"conditioning_dim=0 but 2 conditioning tensor"):
        c(zc, xc, sc, maskc, valuesc)
    with pytest.raises(ValueError, match=r"conditioning_dim=0 but 2 conditioning tensor"):
        c.guided_forward(zc, xc, sc, maskc, valuesc)
    with pytest.raises(ValueError, match=r"conditioning_dim=0 but 2 conditioning tensor"):
        c.guided(maskc, valuesc)
    with pytest.raises(ValueError, match=r"conditioning_dim=0 but 2 conditioning tensor"):
        _forward_replicated(c, zc, xc, sc, maskc, valuesc)
    with pytest.raises(ValueError, match="needs both sensor_mask and sensor_values"):
        m.guided_forward(z, x, s, mask, None)
    with pytest.raises(ValueError, match="needs both sensor_mask and sensor_values"):
        m.guided(None, values)
    view = m.guided(mask, values, 1.5)
    assert (view.num_lon, view.num_lat, view.output_features_dim, view.gamma) == (12, 7, 6, 1.5)
    with pytest.raises(ValueError) as err:
        view._check_shapes(z, x[..., :7], s)
    assert str(err.value) == long
    with pytest.raises(ValueError) as err:
        view._check_shapes(z[:1], x[:1], s[:1])  # the view's sensors are for two samples
    assert str(err.value) == "Expected sensor_mask shape (1, 12, 7, 1)"
    view._check_shapes(z, x, s)
    # well-formed inputs on the host: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(z, x, s, mask, values, wind_direction=torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.guided_forward(z, x, s, mask, values)
    with pytest.raises(RuntimeError, match="no CPU path"):
        view._forward_impl(z, x, s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        c(zc, xc, sc)


def test_training_mode_draws_from_the_host_generator_as_the_reference_does(models, monkeypatch):
    """One draw per ``forward`` with both sensors, two per ``guided_forward``, none in eval mode or without sensors; the outcome
    reaches the input kernel as its ``drop`` flag."""
    from graph_weather_amd import genda

    m = models["genda_model_a"]
    z, x, s, mask, values = do.case_inputs("genda_model_a")
    seen = []
    monkeypatch.setattr(genda.GenDA, "_forward_impl", lambda self, *a: seen.append(("forward", a[-1])))
    monkeypatch.setattr(genda.GenDA, "_guided_impl", lambda self, *a: seen.append(("guided", a[-1])))

    def draws_after(fn, seed=7):
        torch.manual_seed(seed)
        fn()
        after = torch.rand(1).item()
        torch.manual_seed(seed)
        stream = [torch.rand(1).item() for _ in range(4)]
        return stream.index(after), stream

    try:
        m.train()
        n, stream = draws_after(lambda: m(z, x, s, mask, values))
        assert n == 1 and seen[-1] == ("forward", stream[0] < 0.1)
        n, stream = draws_after(lambda: m.guided_forward(z, x, s, mask, values))
        assert n == 2 and seen[-1] == ("guided", stream[0] < 0.1)
        hit = next(k for k in range(1000) if torch.manual_seed(k) and torch.rand(1).item() < 0.1)
        n, stream = draws_after(lambda: m(z, x, s, mask, values), hit)
        assert n == 1 and seen[-1] == ("forward", True)
        n, stream = draws_after(lambda: m.guided_forward(z, x, s, mask, values), hit)
        assert n == 2 and seen[-1] == ("guided", True)  # the first draw decides the conditional half
        c = models["genda_model_c"].train()
        zc, xc, sc, _, _ = do.case_inputs("genda_model_c")
        assert draws_after(lambda: c(zc, xc, sc))[0] == 0 and seen[-1] == ("forward", False)
        m.eval()
        assert draws_after(lambda: m(z, x, s, mask, values))[0] == 0 and seen[-1] == ("forward", False)
        assert draws_after(lambda: m.guided_forward(z, x, s, mask, values))[0] == 0 and seen[-1] == ("guided", False)
    finally:
        m.eval()
        models["genda_model_c"].eval()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_restatement_gives_the_references_outputs(golden_dir, oracle64, name):
    """The oracle the GPU tests use, on our graphs and the seeded weights, against what the reference's own GenDA computed.  Bar: 4 x
    the float32 restatement's error against float64 on the same inputs, at least 1e-6 of the maximum; the recorded outputs are
    float32 results of the reference, so they differ from float64 by about that restatement's error."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    _, kw, B, sigma, seed = do.CASES[name]
    p, kw, graphs, (z, x, s, mask, values) = oracle64[name]
    assert int(g["seed"]) == seed and int(g["meta"][-1]) == B and int(g["meta"][-2]) == kw.get("conditioning_dim", 2)
    assert np.array_equal(g["mask"], mask.numpy().astype(np.float32)) and np.array_equal(g["values"], values.numpy().astype(np.float32))
    assert 0.15 < g["mask"].mean() < 0.45 and set(np.unique(g["mask"])) == {0.0, 1.0} and np.all(g["values"][g["mask"] == 0] == 0)
    sensors = (mask, values) if do.conditioned(name) else ()
    p32, g32 = {k: v.float() for k, v in p.items()}, mo.cast_graphs(graphs, torch.float32)
    f32 = lambda *t: tuple(a.float() for a in t)  # noqa: E731
    checks = [("forward", do.genda_forward(p, kw, graphs, z, x, s, *sensors), do.genda_forward(p32, kw, g32, *f32(z, x, s, *sensors)), g["out"])]
    if sensors:
        assert float(g["gamma"]) == do.GAMMA
        checks.append(("guided", do.genda_guided(p, kw, graphs, z, x, s, mask, values, do.GAMMA),
                       do.genda_guided(p32, kw, g32, *f32(z, x, s, mask, values), do.GAMMA), g["guided"]))
    else:
        assert "guided" not in g.files
    if name == "genda_model_a":  # the reference's training-mode forward under the recorded seed: the conditioning dropped
        zero = (torch.zeros_like(mask), torch.zeros_like(values))
        checks.append(("train", do.genda_forward(p, kw, graphs, z, x, s, *zero), do.genda_forward(p32, kw, g32, *f32(z, x, s, *zero)),
                       g["train_out"]))
        torch.manual_seed(int(g["train_seed"]))
        assert torch.rand(1).item() < 0.1
        torch.manual_seed(int(g["train_miss_seed"]))
        assert torch.rand(1).item() >= 0.1
        assert np.abs(g["train_out"] - g["out"]).max() > 1e-3
    for what, got, got32, rec in checks:
        rec = torch.from_numpy(rec).double()
        top = got.abs().max().item()
        err32 = (got32.double() - got).abs().max().item()
        err = (got - rec).abs().max().item()
        print("%s %s: float64 restatement against the reference's float32 output: %.3e, float32 restatement %.3e (maximum %.3e), "
              "ratio %.2f" % (name, what, err, err32, top, err / max(err32, 1e-300)))
        assert got.shape == rec.shape == z.shape
        assert err <= do.bar(err32, top), (what, err, err32, top)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if do.conditioned(n)])
def test_oracle_guided_is_the_combination_of_its_two_forwards(oracle64, name):
    p, kw, graphs, (z, x, s, mask, values) = oracle64[name]
    for gamma in (2.0, -0.5):
        c = do.genda_forward(p, kw, graphs, z, x, s, mask, values)
        u = do.genda_forward(p, kw, graphs, z, x, s, torch.zeros_like(mask), torch.zeros_like(values))
        assert torch.equal(do.genda_guided(p, kw, graphs, z, x, s, mask, values, gamma), u + gamma * (c - u))
    assert (c - u).abs().max().item() > 1e-3  # the sensors matter
    assert torch.equal(do.genda_guided(p, kw, graphs, z, x, s, mask, values, 0.0), u + 0.0 * (c - u))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {m.group(1) for m in re.finditer(r"\s[TW]\s+(gw_[a-z_0-9]+)$", out, flags=re.M)}


def test_new_entry_points_are_exported_and_refuse_bad_arguments_on_the_host():
    from graph_weather_amd import _lib

    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert set(_lib.EXPORTS) == _exported(_lib.LIB_PATH)
    assert L.gw_version() == _lib.ABI_VERSION == 19
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)

    def fin(batch=2, rows=3, copies=2, drop=0, wz=2, wx=3, ws=4, sd=1.0, ld_z=2, ld_x=3, c0=p, ld_c0=1, c1=p, ld_c1=1, ld_s=4, ld_o=11, sigma=p):
        return L.gw_genda_input_forward(batch, rows, copies, drop, wz, wx, ws, sd, sigma, p, ld_z, p, ld_x, c0, ld_c0, c1, ld_c1, p, ld_s, p,
                                        ld_o, p, None)

    for bad in (dict(batch=0), dict(rows=0), dict(copies=3), dict(copies=0), dict(drop=2), dict(sd=0.0), dict(sd=-1.0), dict(ld_z=1),
                dict(ld_x=2), dict(ld_s=3), dict(ld_o=10), dict(ld_c0=0), dict(ld_c1=0), dict(sigma=None), dict(wz=-1),
                dict(batch=2 ** 16, rows=2 ** 16)):
        assert fin(**bad) == GW_E_BADARG, bad
        assert b"gw_genda_input_forward: bad arguments" in L.gw_last_error()
    assert fin(c1=None, ld_o=9) == GW_E_BADARG  # one column only: the rows are 10 wide

    def bin_(batch=2, rows=3, copies=2, drop=0, wz=2, wx=3, nc=2, sd=1.0, ld_do=7, dz=p, ld_dz=2, dx=p, ld_dx=3, dc0=p, ld_dc0=1, dc1=p, ld_dc1=1):
        return L.gw_genda_input_backward(batch, rows, copies, drop, wz, wx, nc, sd, p, p, ld_do, dz, ld_dz, dx, ld_dx, dc0, ld_dc0, dc1, ld_dc1,
                                         None)

    for bad in (dict(batch=0), dict(copies=3), dict(sd=0.0), dict(ld_do=6), dict(ld_dz=1), dict(ld_dx=2), dict(ld_dc0=0), dict(nc=3),
                dict(nc=1), dict(nc=0), dict(dz=None, dx=None, dc0=None, dc1=None), dict(drop=-1)):
        assert bin_(**bad) == GW_E_BADARG, bad
        assert b"gw_genda_input_backward: bad arguments" in L.gw_last_error()

    def fout(batch=2, rows=3, width=5, sd=1.0, gamma=2.0, ld_z=5, ld_p=5, ld_o=5, z=p):
        return L.gw_genda_guided_output_forward(batch, rows, width, sd, gamma, p, z, ld_z, p, ld_p, p, ld_o, None)

    for bad in (dict(batch=0), dict(rows=0), dict(width=0), dict(sd=0.0), dict(ld_z=4), dict(ld_p=4), dict(ld_o=4), dict(z=None),
                dict(gamma=float("nan"))):
        assert fout(**bad) == GW_E_BADARG, bad
        assert b"gw_genda_guided_output_forward: bad arguments" in L.gw_last_error()

    def bout(batch=2, rows=3, width=5, sd=1.0, gamma=2.0, ld_do=5, dz=p, ld_dz=5, dp=p, ld_dp=5):
        return L.gw_genda_guided_output_backward(batch, rows, width, sd, gamma, p, p, ld_do, dz, ld_dz, dp, ld_dp, None)

    for bad in (dict(batch=0), dict(width=0), dict(sd=0.0), dict(ld_do=4), dict(ld_dz=4), dict(ld_dp=4), dict(dz=None, dp=None)):
        assert bout(**bad) == GW_E_BADARG, bad
        assert b"gw_genda_guided_output_backward: bad arguments" in L.gw_last_error()
    # the Denoiser's entry points keep their signatures and their messages
    assert L.gw_gencast_precond_input_forward(0, 3, 2, 3, 4, 1.0, p, p, 2, p, 3, p, 4, p, 9, p, None) == GW_E_BADARG
    assert b"gw_gencast_precond_input_forward: bad arguments" in L.gw_last_error()
