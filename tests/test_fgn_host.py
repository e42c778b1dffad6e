"""The FGN model without a GPU: the alias import paths, signatures, ``state_dict`` keys, order and shapes against what the
reference's own classes gave (tests/golden/fgn_state_dict.json, scripts/gen_fgn_golden.py), the error messages, the float64
restatement of the forward (tests/fgn_oracle.py) against the three recorded reference outputs, and the argument checks of the new
entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from . import fgn_oracle as fo
from . import gencast_model_oracle as mo
from .cafa_oracle import fill_, params
from .test_alias import alias_modules
from .test_gencast_model_host import _sig

CASE_NAMES = tuple(fo.CASES)
GW_E_BADARG = -1


@pytest.fixture(scope="module")
def tables(golden_dir):
    with open(os.path.join(golden_dir, "fgn_state_dict.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models():
    """name -> our FunctionalGenerativeNetwork on the CPU with the case's seeded weights (built once)."""
    from graph_weather_amd.fgn import FunctionalGenerativeNetwork

    return {name: fill_(FunctionalGenerativeNetwork(**fo.case_kwargs(name)), fo.CASES[name][4]) for name in CASE_NAMES}


def test_alias_imports_give_the_fgn_classes():
    from graph_weather_amd import fgn

    with alias_modules():
        from graph_weather.models.fgn import FunctionalGenerativeNetwork
        from graph_weather.models.fgn.layers import Processor as P1
        from graph_weather.models.fgn.layers.processor import Processor as P2
        from graph_weather.models.fgn.model import FunctionalGenerativeNetwork as F2, FunctionalGenerativeNetworkConfig
    assert FunctionalGenerativeNetwork is F2 is fgn.FunctionalGenerativeNetwork
    assert FunctionalGenerativeNetworkConfig is fgn.FunctionalGenerativeNetworkConfig
    assert P1 is P2 is fgn.Processor
    assert FunctionalGenerativeNetwork.__module__ == P1.__module__ == "graph_weather_amd.fgn"


def test_signatures_equal_the_references(tables):
    from graph_weather_amd.fgn import FunctionalGenerativeNetwork, FunctionalGenerativeNetworkConfig, Processor

    for cls in (FunctionalGenerativeNetwork, Processor, FunctionalGenerativeNetworkConfig):
        assert _sig(cls) == tables["signature"][cls.__name__], cls.__name__
    sig = dict((k, v) for k, v in _sig(FunctionalGenerativeNetwork))
    assert sig["hidden_dims"] == [768, 768] and sig["num_blocks"] == 24 and sig["noise_dimension"] == "<required>"


@pytest.mark.parametrize("name", CASE_NAMES)
def test_state_dict_keys_order_and_buffers(tables, models, name):
    m = models[name]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == tables["state_dict"][name]
    assert list(m.state_dict()) == list(tables["state_dict"][name])  # the order too
    if name == "fgn_model_a":
        assert len(m.state_dict()) == 94
    assert not any("fourier_embedder" in k for k in m.state_dict())
    assert list(m._buffers) == tables["buffers"] and len(tables["buffers"]) == 14
    assert set(m._non_persistent_buffers_set) == set(tables["buffers"])
    kw = fo.CASES[name][1]
    assert (m.khop_mesh_edge_attr is None) == (not kw.get("use_edges_features", True))
    assert m.noise_dimension == kw["noise_dimension"] and m.input_features_dim == kw["input_features_dim"]
    assert m.output_features_dim == kw["output_features_dim"] and m.use_edges_features == kw.get("use_edges_features", True)
    assert m.num_lon == len(fo.case_kwargs(name)["grid_lon"]) and m.num_lat == len(fo.case_kwargs(name)["grid_lat"])
    assert len(m.processor.cond_transformers) == kw["num_blocks"]


def test_config_builds_the_model_and_hub_mixin():
    from graph_weather_amd.fgn import FunctionalGenerativeNetwork, FunctionalGenerativeNetworkConfig

    lon, lat = mo.GRIDS["gencast_model_a"]()
    cfg = FunctionalGenerativeNetworkConfig(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, noise_dimension=5,
                                            splits=1, num_hops=1, num_blocks=1, hidden_dims=[8, 8])
    assert FunctionalGenerativeNetworkConfig(lon, lat, 1, 1, 4).hidden_dims == [768, 768]
    m = cfg.build()
    assert isinstance(m, FunctionalGenerativeNetwork) and len(m.processor.cond_transformers) == 1
    assert m.processor.cond_transformers[0].cond_norm.linear_scale.in_features == 5
    try:
        from huggingface_hub import PyTorchModelHubMixin
    except Exception:
        return
    assert isinstance(m, PyTorchModelHubMixin)


def test_error_messages(models):
    from graph_weather_amd.fgn import FunctionalGenerativeNetwork, Processor, _forward_member_loop

    lon, lat = mo.GRIDS["gencast_model_a"]()
    kw = dict(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, noise_dimension=4, hidden_dims=[8, 8], num_blocks=1,
              splits=1, num_hops=1)
    with pytest.raises(ValueError, match="Sparse processor don't support edges features."):
        FunctionalGenerativeNetwork(sparse=True, **kw)
    with pytest.raises(ValueError, match="Please install DGL to use sparsity."):
        FunctionalGenerativeNetwork(sparse=True, use_edges_features=False, **kw)
    with pytest.raises(ValueError, match="The latent dimension should be divisible by the number of heads."):
        Processor(latent_dim=10, hidden_dims=[8, 10], num_blocks=2, num_heads=4, noise_emb_dim=3)
    with pytest.raises(ValueError, match="Please install DGL to use sparsity."):
        Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, noise_emb_dim=3, sparse=True)
    proc = Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, noise_emb_dim=3)
    assert not hasattr(proc, "fourier_embedder") and not hasattr(proc, "edges_mlp")
    ei = torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ValueError) as err:
        proc(torch.zeros(5, 7), ei, torch.zeros(5, 3))
    assert str(err.value) == "The dimension of the mesh nodes is different from the latent dimension provided at initialization."
    with pytest.raises(ValueError) as err:
        proc(torch.zeros(5, 8), ei, torch.zeros(4, 3))
    assert str(err.value) == ("The number of noise levels and mesh nodes should be the same, but got 5 and 4. Eventually repeat the "
                              " noise level for each node in the same batch.")
    with pytest.raises(ValueError) as err:
        proc(torch.zeros(5, 8), ei, torch.zeros(5, 3), torch.zeros(1, 4))
    assert str(err.value) == "To use input_edge_attr initialize the processor with edges_dim."

    m = models["fgn_model_a"]
    x = fo.case_input("fgn_model_a")
    for bad in (x[:, :, :, :3], x.transpose(1, 2), x[0]):
        with pytest.raises(ValueError, match="shape of the input tensor"):
            m(bad)
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_ensemble"):
            m(x, num_ensemble=n)
    for bad in (torch.zeros(2, 3, 8), torch.zeros(2, 2, 7), torch.zeros(4, 8)):
        with pytest.raises(ValueError, match="noise_vectors must have shape"):
            m(x, num_ensemble=2, noise_vectors=bad)
    with pytest.raises(ValueError, match="noise_vectors must have shape"):
        _forward_member_loop(m, x, torch.zeros(3, 2, 8))
    with pytest.raises(RuntimeError, match="HIP device"):  # well-formed inputs on the host: there is no CPU path
        m(x, num_ensemble=2, noise_vectors=torch.zeros(2, 2, 8))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_restatement_gives_the_references_outputs(golden_dir, models, name):
    """The oracle the GPU tests use, on our graphs and the seeded weights, against what the reference's own FGN computed."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    _, kw, B, N, seed = fo.CASES[name]
    assert int(g["seed"]) == seed and int(g["torch_seed"]) == fo.TORCH_SEED + seed and list(g["meta"][-2:]) == [B, N]
    noise = fo.draw_noise(int(g["torch_seed"]), B, N, kw["noise_dimension"])
    assert np.array_equal(noise.numpy(), g["noise"])  # the recorded vectors are what the seed draws
    m = models[name]
    got = fo.fgn_forward(params(m, torch.float64), kw, mo.cast_graphs(mo.graph_tables(m), torch.float64), fo.case_input(name).double(),
                         noise.double())
    members = torch.from_numpy(g["members"]).double()
    err = (got - members).abs().max().item()
    print("%s: float64 restatement against the reference's members: %.3e (maximum %.3e)" % (name, err, members.abs().max().item()))
    assert got.shape == members.shape == (B, N, m.num_lon, m.num_lat, m.output_features_dim)
    assert err <= 2e-5 * max(members.abs().max().item(), 1.0)
    out = g["out"]
    if B > 1:
        assert np.array_equal(out, g["members"])  # the reference's forward is all members
    else:  # the reference's forward at B = 1: member 0 only
        assert out.shape == (1, 1, m.num_lon, m.num_lat, m.output_features_dim) and np.array_equal(out[:, 0], g["members"][:, 0])
        assert (got[:, :1] - torch.from_numpy(out).double()).abs().max().item() <= 2e-5 * max(members.abs().max().item(), 1.0)
        assert (members[:, 0] - members[:, 1]).abs().max().item() > 1e-3  # the member the reference drops is another forecast


def test_new_entry_points_are_exported_and_refuse_bad_arguments_on_the_host():
    from graph_weather_amd import _lib

    new = ("gw_cond_layernorm_fanout_forward", "gw_cond_layernorm_fanout_workspace_bytes", "gw_cond_layernorm_fanout_backward",
           "gw_linear_gather_grouped_forward", "gw_segment_sum_rows_grouped")
    L = _lib.lib()
    for name in new:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.gw_version() == _lib.ABI_VERSION == 19
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    fwd = [p, 4, p, 4, p, 4, p, 4, None]
    assert L.gw_cond_layernorm_fanout_forward(8, 4, 0, 4, 0, *fwd) == GW_E_BADARG  # no members
    assert b"gw_cond_layernorm_fanout_forward" in L.gw_last_error()
    assert L.gw_cond_layernorm_fanout_forward(8, 4, 0, 3, 2, *fwd) == GW_E_BADARG  # 8 rows do not split into samples of 3
    assert L.gw_cond_layernorm_fanout_forward(8, 4, 3, 4, 2, *fwd) == GW_E_BADARG  # no such activation
    assert L.gw_cond_layernorm_fanout_forward(8, 4, 0, 4, 2, p, 3, p, 4, p, 4, p, 4, None) == GW_E_BADARG  # ld_x below the width
    assert L.gw_cond_layernorm_fanout_forward(8, 4, 0, 1, 40000, *fwd) == GW_E_BADARG  # more than 65535 (sample, member) pairs
    assert L.gw_cond_layernorm_fanout_forward(0, 4, 0, 4, 2, *fwd) == 0  # no rows: nothing is launched
    # statistics of the 600 x rows + (2 samples x 3 members) x 2 slabs x (dscale, dbias) x width
    assert L.gw_cond_layernorm_fanout_workspace_bytes(600, 12, 300, 3) == (600 * 2 + 6 * 2 * 2 * 12) * 4
    assert L.gw_cond_layernorm_fanout_workspace_bytes(600, 12, 300, 0) == 0
    assert L.gw_cond_layernorm_fanout_workspace_bytes(600, 12, 7, 3) == 0
    bwd = [p, 4, p, 4, p, 4, p, 4]
    assert L.gw_cond_layernorm_fanout_backward(8, 4, 0, 4, 2, *bwd, p, 16, p, 4, p, p, 4, None) == GW_E_BADARG  # workspace too small
    assert b"workspace" in L.gw_last_error()
    assert L.gw_cond_layernorm_fanout_backward(8, 4, 0, 4, 2, *bwd, p, 4096, None, 4, None, None, 4, None) == GW_E_BADARG  # nothing wanted
    assert L.gw_cond_layernorm_fanout_backward(8, 4, 0, 4, 2, *bwd, None, 4096, p, 4, p, p, 4, None) == GW_E_BADARG  # no workspace

    tabs, idx = (ctypes.c_void_p * 3)(p, p, p), (ctypes.c_void_p * 3)(None, None, None)
    lds, rpb = (ctypes.c_int32 * 3)(4, 4, 4), (ctypes.c_int32 * 3)(0, 8, 8)

    def gather(share, n_add=2, rows_per_batch=8, ld=4, have_share=True):
        sh = (ctypes.c_int32 * 3)(*share)
        return L.gw_linear_gather_grouped_forward(16, rows_per_batch, 0, 4, None, 0, None, 0, None, n_add, tabs, idx, lds, rpb,
                                                  sh if have_share else None, 0, p, ld, None)

    assert gather((1, 0, 1)) == GW_E_BADARG  # share 0
    assert b"gw_linear_gather_grouped_forward" in L.gw_last_error()
    assert gather((1, -2, 1)) == GW_E_BADARG
    assert gather((1, 2, 1), have_share=False) == GW_E_BADARG  # tables without share counts
    assert gather((1, 2, 1), n_add=0) == GW_E_BADARG  # neither a product nor a table
    assert gather((1, 2, 1), n_add=4) == GW_E_BADARG
    assert gather((1, 2, 1), rows_per_batch=0) == GW_E_BADARG
    assert gather((1, 2, 1), ld=3) == GW_E_BADARG  # ldo below the width
    # the existing entry keeps its checks and its message
    assert L.gw_linear_gather_forward(16, 0, 0, 4, None, 0, None, 0, None, 2, tabs, idx, lds, rpb, 0, p, 4, None) == GW_E_BADARG
    assert b"gw_linear_gather_forward: bad arguments" in L.gw_last_error()

    seg = [p, 4, 8, None, p, p, 4, None]
    assert L.gw_segment_sum_rows_grouped(6, 4, 8, 4, *seg) == GW_E_BADARG  # 6 copies do not split into groups of 4
    assert b"gw_segment_sum_rows_grouped" in L.gw_last_error()
    assert L.gw_segment_sum_rows_grouped(6, 0, 8, 4, *seg) == GW_E_BADARG
    assert L.gw_segment_sum_rows_grouped(0, 1, 8, 4, *seg) == GW_E_BADARG
    assert L.gw_segment_sum_rows_grouped(6, 3, 8, 4, p, 3, 8, None, p, p, 4, None) == GW_E_BADARG  # ld below the width
    assert L.gw_segment_sum_rows_grouped(6, 3, 8, 4, p, 4, 8, None, None, p, 4, None) == GW_E_BADARG  # no pointers
    assert L.gw_segment_sum_rows_grouped(6, 3, 0, 4, *seg) == 0  # no segments: nothing is launched
    assert L.gw_segment_sum_rows_wide(6, 3, 8, 4, *seg) == GW_E_BADARG  # the existing entry: batch_out is batch or 1
    assert b"gw_segment_sum_rows_wide" in L.gw_last_error()
