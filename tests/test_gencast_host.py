"""The GenCast layers without a GPU: the float32 restatement against the reference's recorded outputs, signatures and state_dict
exchange with the reference's tables, the alias import paths, the host-side errors of the modules and of the new C entry points."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from . import gencast_oracle as go
from .test_alias import alias_modules

CLASSES = ("MLP", "InteractionNetwork", "FourierEmbedding", "ConditionalLayerNorm", "CondTransformerBlock", "Encoder", "Processor",
           "Decoder")


@pytest.fixture(scope="module")
def tables(golden_dir):
    with open(os.path.join(golden_dir, "gencast_state_dict.json")) as f:
        return json.load(f)


def test_alias_imports_give_the_gencast_classes():
    from graph_weather_amd import gencast

    with alias_modules():
        import graph_weather.models.gencast  # noqa: F401
        from graph_weather.models.gencast.layers import MLP, Decoder, Encoder, InteractionNetwork
        from graph_weather.models.gencast.layers.decoder import Decoder as D2
        from graph_weather.models.gencast.layers.encoder import Encoder as E2
        from graph_weather.models.gencast.layers.modules import (MLP as M2, ConditionalLayerNorm, CondTransformerBlock,
                                                                 FourierEmbedding, InteractionNetwork as I2)
        from graph_weather.models.gencast.layers.processor import Processor
    assert (MLP, InteractionNetwork, Encoder, Decoder) == (gencast.MLP, gencast.InteractionNetwork, gencast.Encoder, gencast.Decoder)
    assert (M2, I2, E2, D2, Processor) == (gencast.MLP, gencast.InteractionNetwork, gencast.Encoder, gencast.Decoder, gencast.Processor)
    assert (ConditionalLayerNorm, CondTransformerBlock, FourierEmbedding) == (gencast.ConditionalLayerNorm, gencast.CondTransformerBlock,
                                                                             gencast.FourierEmbedding)


def test_the_top_level_names_stay_the_forecasters():
    import graph_weather_amd as gw

    assert gw.gencast.Encoder is not gw.Encoder and gw.gencast.Processor is not gw.Processor
    assert gw.gencast.Decoder is not gw.Decoder and gw.gencast.MLP is not gw.MLP


@pytest.mark.parametrize("cls", CLASSES)
def test_signatures_and_defaults_equal_the_references(tables, cls):
    from graph_weather_amd import gencast

    got = []
    for name, prm in list(inspect.signature(getattr(gencast, cls).__init__).parameters.items())[1:]:
        d = prm.default
        got.append([name, "<required>" if d is inspect.Parameter.empty else (d.__name__ if inspect.isclass(d) else d)])
    assert got == tables["signature"][cls]


def _ours(key):
    from graph_weather_amd import gencast

    cls, _, name = key.partition(":")
    if name in go.CASES:
        return go.build(gencast, name)
    if key == "InteractionNetwork":
        return gencast.InteractionNetwork(sender_dim=5, receiver_dim=6, edge_attr_dim=3, hidden_dims=[9, 8], use_layer_norm=True)
    if key == "ConditionalLayerNorm":
        return gencast.ConditionalLayerNorm(conditioning_dim=5, features_dim=12)
    if key == "CondTransformerBlock":
        return gencast.CondTransformerBlock(input_dim=12, output_dim=4, num_heads=3, conditioning_dim=5, edges_dim=6)
    assert key == "CondTransformerBlock:mean"
    return gencast.CondTransformerBlock(input_dim=12, output_dim=12, num_heads=3, concat=False)


def test_state_dict_keys_order_and_shapes_equal_the_references(tables):
    assert len(tables["state_dict"]) == len(go.CASES) + 4
    for key, want in tables["state_dict"].items():
        module = _ours(key)
        sd = module.state_dict()
        assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, v) for k, v in want.items()], key
        # both ways, strict: a state_dict made from the reference's table loads here, and ours fits the table
        theirs = {k: torch.full(shape, 0.5) for k, shape in want.items()}
        res = module.load_state_dict(theirs, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(v, theirs[k]) for k, v in module.state_dict().items())


@pytest.mark.parametrize("name", list(go.CASES))
def test_restatement_reproduces_the_reference(golden_dir, name):
    from graph_weather_amd import gencast

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    assert int(g["seed"]) == go.CASES[name][3] and list(g["meta"]) == go.meta_of(name)
    module = go.build(gencast, name)
    with torch.no_grad():
        outs = go.run(name, go.params(module, torch.float32), go.cast(go.case_inputs(name), torch.float32))
    assert len(outs) == sum(1 for k in g.files if k.startswith("out"))
    for i, ref in enumerate(outs):
        out = torch.from_numpy(g["out%d" % i])
        assert tuple(ref.shape) == tuple(out.shape)
        err = (out - ref).abs().max().item() / ref.abs().max().item()
        print("%s output %d: the float32 restatement differs from the reference's output by %.3e of the maximum" % (name, i, err))
        assert err <= 1e-6, err
        assert torch.isfinite(ref).all() and ref.abs().max() > 0.1


def test_the_processor_cases_have_nodes_without_edges_and_distinct_noise():
    inp = go.case_inputs("gencast_processor_edges")
    deg = torch.bincount(inp["edge_index"][1], minlength=74)
    assert int(deg.min()) == 0 and int(deg.max()) == 9 and inp["noise_levels"][0] != inp["noise_levels"][-1]
    assert not torch.equal(inp["edge_index"][1], inp["edge_index"][1].sort().values)  # unsorted COO


def test_argument_checks_raise_the_references_errors():
    from graph_weather_amd import gencast

    with pytest.raises(ValueError, match="The latent dimension should be divisible by the number of heads."):
        gencast.Processor(latent_dim=30, hidden_dims=[8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16, noise_emb_dim=4)
    with pytest.raises(ValueError, match="Please install DGL to use sparsity."):
        gencast.Processor(latent_dim=32, hidden_dims=[8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16, noise_emb_dim=4,
                          sparse=True)
    p = gencast.Processor(latent_dim=32, hidden_dims=[8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16, noise_emb_dim=4)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="The dimension of the mesh nodes is different from the latent dimension"):
        p(torch.zeros(5, 31), ei, torch.zeros(5, 1))
    with pytest.raises(ValueError, match="The number of noise levels and mesh nodes should be the same, but got 5 and 4"):
        p(torch.zeros(5, 32), ei, torch.zeros(4, 1))
    with pytest.raises(ValueError, match="To use input_edge_attr initialize the processor with edges_dim."):
        p(torch.zeros(5, 32), ei, torch.zeros(5, 1), torch.zeros(3, 4))
    d = gencast.Decoder(edges_dim=4, output_dim=5, hidden_dims=[8, 6])
    with pytest.raises(ValueError, match="must be equal to the last hidden dimension"):
        d(torch.zeros(3, 6), torch.zeros(4, 7), torch.zeros(2, 4), ei[:, :2])
    c = gencast.ConditionalLayerNorm(conditioning_dim=3, features_dim=6)
    with pytest.raises(ValueError, match="Expected same batch dimension for the input and the conditioning parameter, got 5 and 4"):
        c(torch.zeros(5, 6), torch.zeros(4, 3))


def test_other_activations_and_oversized_heads_are_not_implemented():
    from graph_weather_amd import gencast

    with pytest.raises(NotImplementedError, match="nn.ReLU or nn.SiLU"):
        gencast.MLP(4, [8, 8], activation_layer=nn.GELU)
    with pytest.raises(NotImplementedError, match="nn.ReLU or nn.SiLU"):
        gencast.CondTransformerBlock(8, 4, 2, activation_layer=nn.Tanh)
    with pytest.raises(NotImplementedError, match="heads \\* dim_head <= 4096"):
        gencast.CondTransformerBlock(8, 2048, 4, concat=False)
    gencast.CondTransformerBlock(8, 4, 2, activation_layer=None)


def test_cpu_tensors_raise_no_cpu_path():
    from graph_weather_amd import gencast

    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    for name in go.CASES:
        module, inp = go.build(gencast, name), go.case_inputs(name)
        with pytest.raises(RuntimeError, match="no CPU path"):
            go.call(module, name, inp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gencast.CondTransformerBlock(8, 4, 2)(torch.zeros(3, 8), ei)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gencast.edge_plan(ei, 3, 3)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from graph_weather_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int32 * 64)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)

    def fwd(n_dst=2, n_src=2, E=2, H=2, C=4, dst_ptr=ip, q=p, out=p, lse=p, ld=8):
        return L.gw_graph_attention_forward(n_dst, n_src, E, H, C, dst_ptr, ip, None, q, ld, p, 8, p, 8, None, 0, 0, out, 8, None, 0, lse, None)

    assert fwd(n_dst=-1) == -1 and fwd(E=-1) == -1 and fwd(H=0) == -1 and fwd(C=0) == -1
    assert fwd(dst_ptr=None) == -1 and fwd(q=None) == -1 and fwd(out=None) == -1 and fwd(lse=None) == -1 and fwd(ld=7) == -1
    assert b"gw_graph_attention_forward" in L.gw_last_error()
    assert fwd(H=2, C=4096) == -2 and b"4096" in L.gw_last_error()  # GW_E_UNSUPPORTED
    assert fwd(n_dst=0) == 0 and fwd(E=0) == 0  # empty launches: GW_OK, nothing launched

    def bwd(n_dst=2, E=2, H=2, dst=ip, dout=p, delta=p, dq=p, ld_dq=8):
        return L.gw_graph_attention_backward(n_dst, 2, E, H, 4, ip, ip, dst, None, ip, ip, p, 8, p, 8, p, 8, None, 0, 0, p, 8, dout, 8, p,
                                             delta, dq, ld_dq, p, 8, p, 8, None, 0, None)

    assert bwd(n_dst=-1) == -1 and bwd(H=0) == -1 and bwd(dst=None) == -1 and bwd(dout=None) == -1 and bwd(delta=None) == -1
    assert bwd(dq=None) == -1 and bwd(ld_dq=7) == -1 and bwd(E=0) == 0
    assert L.gw_cond_layernorm_forward(-1, 8, 0, p, 8, p, 8, p, 8, p, 8, None) == -1
    assert L.gw_cond_layernorm_forward(2, 8, 3, p, 8, p, 8, p, 8, p, 8, None) == -1
    assert L.gw_cond_layernorm_forward(2, 8, 0, None, 8, p, 8, p, 8, p, 8, None) == -1
    assert L.gw_cond_layernorm_forward(2, 8, 0, p, 7, p, 8, p, 8, p, 8, None) == -1
    assert L.gw_cond_layernorm_forward(0, 8, 0, p, 8, p, 8, p, 8, p, 8, None) == 0
    assert L.gw_cond_layernorm_backward(2, 8, 0, p, 8, p, 8, p, 8, None, 8, p, 8, p, p, 8, None) == -1
    assert L.gw_cond_layernorm_backward(2, 8, 0, p, 8, p, 8, p, 8, p, 8, None, 8, None, None, 8, None) == -1
    assert L.gw_cond_layernorm_backward(-2, 8, 0, p, 8, p, 8, p, 8, p, 8, p, 8, p, p, 8, None) == -1
    assert L.gw_beta_gate_forward(2, 8, None, 8, p, 8, p, p, 8, p, None) == -1
    assert L.gw_beta_gate_forward(-1, 8, p, 8, p, 8, p, p, 8, p, None) == -1
    assert L.gw_beta_gate_forward(2, 8, p, 8, p, 8, p, p, 8, None, None) == -1
    assert L.gw_beta_gate_workspace_bytes(-1, 8) == 0 and L.gw_beta_gate_workspace_bytes(2, 0) == 0
    assert L.gw_beta_gate_workspace_bytes(300, 8) == 4 * (300 + 2 * 3 * 8)
    assert L.gw_beta_gate_backward(2, 8, p, 8, p, 8, p, p, p, 8, None, 0, p, p, 8, p, None) == -1
    assert L.gw_beta_gate_backward(2, 8, p, 8, p, 8, p, p, p, 8, p, 4, p, p, 8, p, None) == -1  # workspace too small
    assert L.gw_beta_gate_backward(-1, 8, p, 8, p, 8, p, p, p, 8, p, 4096, p, p, 8, p, None) == -1
    assert L.gw_silu_forward(-1, p, p, None) == -1 and L.gw_silu_forward(4, None, p, None) == -1 and L.gw_silu_forward(0, p, p, None) == 0
    assert L.gw_silu_backward(4, p, None, p, None) == -1 and L.gw_silu_backward(-4, p, p, p, None) == -1
    assert L.gw_fourier_forward(2, 0, 16.0, p, p, 8, None) == -1 and L.gw_fourier_forward(2, 4, 0.0, p, p, 8, None) == -1
    assert L.gw_fourier_forward(2, 4, 16.0, None, p, 8, None) == -1 and L.gw_fourier_forward(2, 4, 16.0, p, p, 7, None) == -1
    assert L.gw_fourier_backward(2, 4, 16.0, p, None, 8, p, None) == -1 and L.gw_fourier_backward(-2, 4, 16.0, p, p, 8, p, None) == -1
    assert L.gw_fourier_backward(0, 4, 16.0, p, p, 8, p, None) == 0
