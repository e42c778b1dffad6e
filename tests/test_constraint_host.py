"""PhysicalConstraintLayer (constraint_type "additive" / "multiplicative" / "softmax"), host side: the node -> grid maps
against the reference's graph_to_grid / grid_to_graph loops, construction through every public path, state_dict /
deepcopy / .to() without the reference's module cycle, clear errors, the C ABI's argument checks, and (reference-marked)
the closed forms of graph_weather_amd/constraint.py against the reference's own constraint_layer.py in fp64."""
import contextlib
import copy
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import graph_weather_amd as gw
from graph_weather_amd import _lib
from graph_weather_amd.constraint import grid_maps, inverse_csr
from graph_weather_amd.utils import regular_lat_lons


def _grid_mapping(res):
    """node_to_grid and grid_shape of the forecaster at ``res`` degrees, without building its graphs."""
    lat_lons = [tuple(ll) for ll in regular_lat_lons(res)]
    ns = types.SimpleNamespace(original_lat_lons=lat_lons)
    lats, lons = sorted(set(a for a, _ in lat_lons)), sorted(set(b for _, b in lat_lons))
    gw.GraphWeatherForecaster._create_grid_mapping(ns, lats, lons)
    return ns.node_to_grid, (len(lats), len(lons))


@pytest.mark.parametrize("res,hit", [(30.0, 72), (5.0, 2376), (1.0, 57800)])
def test_maps_match_the_reference_loops(res, hit):
    node_to_grid, (H, W) = _grid_mapping(res)
    N = len(node_to_grid)
    assert N == H * W
    m = grid_maps(node_to_grid, (H, W))
    # graph_to_grid: grid[row, col] = node (last writer wins); grid_to_graph: node reads grid[row, col]
    grid = [-1] * (H * W)
    for n, (r, c) in enumerate(node_to_grid):
        grid[r * W + c] = n
    pi = np.array([r * W + c for r, c in node_to_grid])
    sigma = np.array([grid[r * W + c] for r, c in node_to_grid])
    np.testing.assert_array_equal(m["pi"], pi)
    np.testing.assert_array_equal(m["sigma"], sigma)
    assert int((m["hit"] > 0).sum()) == hit == sum(g >= 0 for g in grid)
    assert int(m["hit"].sum()) == N
    ptr, idx = inverse_csr(m["pi"], H * W)
    np.testing.assert_array_equal(np.diff(ptr), m["hit"])
    for k in range(0, H * W, max(1, H * W // 997)):  # a sample of rows: the nodes of cell k, ascending
        np.testing.assert_array_equal(idx[ptr[k]:ptr[k + 1]], np.nonzero(pi == k)[0])
    if res == 1.0:
        assert int((pi != np.arange(N)).sum()) == 7340  # nodes that read another node's row
        assert H * W - hit == 7000                      # decoder outputs that never reach the constrained output


@pytest.mark.parametrize("ctype", ["additive", "multiplicative", "softmax"])
def test_constrained_forecaster_constructs_without_module_cycle(ctype):
    lat_lons = regular_lat_lons(30.0)
    plain = gw.GraphWeatherForecaster(lat_lons)
    model = gw.GraphWeatherForecaster(lat_lons, constraint_type=ctype)
    assert model.constraint.constraint_type == ctype and model.constraint.model is model
    assert model.constraint.upsampling_factor == 1 and model.constraint.grid_shape == (6, 12)
    a, b = plain.state_dict(), model.state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape for k in a)
    assert [n for n, _ in model.named_modules() if n.startswith("constraint")] == ["constraint"]
    twin = copy.deepcopy(model)
    assert twin.constraint.model is twin
    assert model.to("cpu") is model
    cfg = gw.GraphWeatherForecasterConfig(lat_lons=lat_lons, constraint_type=ctype).build()
    assert cfg.constraint.constraint_type == ctype


def test_constraint_errors():
    lat_lons = regular_lat_lons(30.0)
    with pytest.raises(ValueError, match="Unknown constraint type"):
        gw.GraphWeatherForecaster(lat_lons, constraint_type="bogus")
    with pytest.raises(ValueError, match="one node per cell"):
        gw.GraphWeatherForecaster(lat_lons[:-1], constraint_type="additive")
    model = gw.GraphWeatherForecaster(lat_lons)
    for ctype in ("additive", "multiplicative"):
        with pytest.raises(ValueError, match="upsampling_factor 1"):
            gw.PhysicalConstraintLayer(model, model.grid_shape, 2, ctype)
    with pytest.raises(ValueError, match="whole"):
        gw.PhysicalConstraintLayer(model, model.grid_shape, 5, "softmax")
    layer = gw.PhysicalConstraintLayer(model, model.grid_shape, 1, "none")
    with pytest.raises(ValueError, match="Unknown constraint type"):
        layer._spec(0)
    layer = gw.PhysicalConstraintLayer(model, model.grid_shape, 1, "additive")
    with pytest.raises(ValueError, match="spatial dimensions"):
        layer(torch.zeros(1, 2, 5, 12), torch.zeros(1, 2, 5, 12))
    with pytest.raises(ValueError, match="3D"):
        layer(torch.zeros(72, 2), torch.zeros(72, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.zeros(1, 72, 2), torch.zeros(1, 72, 2))
    with pytest.raises(ValueError, match="4-D"):
        gw.PhysicalConstraintLayer(model, model.grid_shape, 2, "softmax")(torch.zeros(1, 72, 2), torch.zeros(1, 72, 2))
    stub = types.SimpleNamespace(node_to_grid=model.node_to_grid[:-1])
    with pytest.raises(ValueError, match="do not fill"):
        gw.PhysicalConstraintLayer(stub, model.grid_shape, 1, "softmax")


@contextlib.contextmanager
def _alias_modules():
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "graph_weather" or k.startswith("graph_weather.")}
    try:
        yield
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_alias_import_path():
    with _alias_modules():
        from graph_weather.models.layers.constraint_layer import PhysicalConstraintLayer

        assert PhysicalConstraintLayer is gw.PhysicalConstraintLayer


def _args(**kw):
    base = dict(type=1, batch=2, nodes=72, channels=78, cells=72, f=1, grid_h=6, grid_w=12, graph_rows=0, exp_factor=1.0,
                hr=1, ld_hr=78, lr=1, ld_lr=102, map=1, inv_ptr=1, inv_idx=1)  # pointers only have to be non-null here
    base.update(kw)
    return _lib.GwConstraintArgs(**base)


def test_constraint_argument_validation_without_gpu():
    L = _lib.lib()
    assert L.gw_constraint_forward(None, None, 0, None, 78, None) == -1
    assert b"bad arguments" in L.gw_last_error()
    assert L.gw_constraint_backward(None, None, 78, None, 0, None, 78, None, 78, None) == -1
    assert L.gw_constraint_workspace_bytes(None) == 0
    # the statistics types need a workspace; the softmax with f = 1 none
    n_slabs = 2  # 72 rows in slabs of 64
    want = (4 * 2 * n_slabs * 78 * 8 + 255) // 256 * 256 + (6 * 2 * 78 * 4 + 255) // 256 * 256
    assert L.gw_constraint_workspace_bytes(ctypes.byref(_args())) == want
    assert L.gw_constraint_workspace_bytes(ctypes.byref(_args(type=3))) == 0
    assert L.gw_constraint_workspace_bytes(ctypes.byref(_args(type=3, f=2, cells=72))) == 2 * ((2 * 18 * 78 * 4 + 255) // 256 * 256)
    for bad in (dict(type=0), dict(type=4), dict(hr=None), dict(map=None), dict(ld_hr=77), dict(ld_lr=10), dict(channels=0),
                dict(f=2), dict(type=3, f=5), dict(type=3, f=2, graph_rows=1), dict(type=3, f=2, grid_h=5)):
        a = _args(**bad)
        assert L.gw_constraint_workspace_bytes(ctypes.byref(a)) == 0, bad
        assert L.gw_constraint_forward(ctypes.byref(a), None, 1 << 20, 1, 78, None) == -1, bad
    # a workspace smaller than the query: refused before any launch
    assert L.gw_constraint_forward(ctypes.byref(_args()), 1, 16, 1, 78, None) == -1
    assert b"workspace" in L.gw_last_error()
    assert L.gw_constraint_forward(ctypes.byref(_args()), 1, 1 << 20, None, 78, None) == -1
    assert L.gw_constraint_backward(ctypes.byref(_args()), None, 78, 1, 1 << 20, 1, 78, 1, 102, None) == -1
    # more than 2^31-1 elements: unsupported, like gw_project_forward
    big = _args(batch=16, nodes=1 << 24, cells=1 << 24, ld_hr=78, grid_h=1, grid_w=1 << 24)
    assert L.gw_constraint_forward(ctypes.byref(big), 1, 1 << 40, 1, 78, None) == -2
    assert b"2^31-1" in L.gw_last_error()


def _closed_form(ctype, hr, lr, index, a=1.0):
    """fp64 closed forms (f = 1): hr, lr [B, K, C] rows, index [N] the row each node reads."""
    h, l = hr[:, index], lr[:, index]
    if ctype == "additive":
        return h + (l - h.mean(dim=1, keepdim=True))
    if ctype == "multiplicative":
        return h * (l.mean(dim=1, keepdim=True) / (h.mean(dim=1, keepdim=True) + 1e-8))
    e = torch.exp(a * h)
    return e * (l * (1 / e))


def _softmax_blocks(hr_grid, lr_low, f, a, pi):
    E = torch.exp(a * hr_grid)
    S = torch.nn.functional.avg_pool2d(E, f) * f * f
    R = E * torch.kron(lr_low * (1 / S), torch.ones(f, f, dtype=E.dtype))
    B, C, H, W = R.shape
    return R.permute(0, 2, 3, 1).reshape(B, H * W, C)[:, pi]


@pytest.mark.reference
@pytest.mark.parametrize("res", [5.0, 30.0])
def test_closed_forms_match_the_reference_layer(res):
    from oracle import refload

    if not refload.reference_available():
        pytest.skip("reference tree not present")
    refload.load_reference()
    Ref = sys.modules["graph_weather.models.layers.constraint_layer"].PhysicalConstraintLayer
    node_to_grid, (H, W) = _grid_mapping(res)

    class Stub:  # the reference's graph_to_grid / grid_to_graph loops, in fp64
        def __init__(self):
            self.node_to_grid, self.grid_shape = node_to_grid, (H, W)

        def graph_to_grid(self, g):
            grid = torch.zeros(g.shape[0], g.shape[2], H, W, dtype=torch.float64)
            for n, (r, c) in enumerate(self.node_to_grid):
                grid[..., r, c] = g[..., n, :]
            return grid

        def grid_to_graph(self, grid):
            graph = torch.zeros(grid.shape[0], H * W, grid.shape[1], dtype=torch.float64)
            for n, (r, c) in enumerate(self.node_to_grid):
                graph[..., n, :] = grid[..., r, c]
            return graph

    m = grid_maps(node_to_grid, (H, W))
    gen = torch.Generator().manual_seed(7)
    B, C = 2, 3
    hr = torch.randn(B, H * W, C, generator=gen, dtype=torch.float64) + 0.5
    lr = torch.randn(B, H * W, C, generator=gen, dtype=torch.float64)
    grid = lambda t: t.reshape(B, H, W, C).permute(0, 3, 1, 2)  # forecast.py:235 "b (h w) c -> b c h w"
    for ctype in ("additive", "multiplicative", "softmax"):
        ref = Ref(Stub(), (H, W), 1, ctype)
        torch.testing.assert_close(ref(grid(hr), grid(lr)), _closed_form(ctype, hr, lr, m["pi"]), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref(hr, lr), _closed_form(ctype, hr, lr, m["sigma"]), rtol=1e-12, atol=1e-12)
    f = 2 if H % 2 == 0 and W % 2 == 0 else 3
    ref = Ref(Stub(), (H, W), f, "softmax", exp_factor=0.7)
    lr_low = torch.randn(B, C, H // f, W // f, generator=gen, dtype=torch.float64)
    torch.testing.assert_close(ref(grid(hr), lr_low), _softmax_blocks(grid(hr), lr_low, f, 0.7, m["pi"]), rtol=1e-12, atol=1e-12)
