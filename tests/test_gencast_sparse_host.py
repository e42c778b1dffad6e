"""The sparse GenCast processor without a GPU: class attributes and state_dict exchange with the reference's tables, the alias
import paths, the ``sparse`` switch of the processors, models and configs, the restatement of tests/gencast_sparse_oracle.py against
a dense masked softmax and against the reference's recorded outputs, and the host-side checks of the two new C entry points."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from . import gencast_sparse_oracle as so
from .test_alias import alias_modules

DGL_TEXT = "Please install DGL to use sparsity."
EDGES_TEXT = "Sparse processor don't support edges features."


@pytest.fixture(scope="module")
def tables(golden_dir):
    with open(os.path.join(golden_dir, "gencast_sparse_state_dict.json")) as f:
        return json.load(f)


def _classes():
    import types

    from graph_weather_amd import fgn, gencast, gencast_sparse

    return types.SimpleNamespace(SparseAttention=gencast_sparse.SparseAttention, SparseTransformer=gencast_sparse.SparseTransformer,
                                 Processor=gencast.Processor, FgnProcessor=fgn.Processor)


def _model(name, sparse="native"):
    from graph_weather_amd import fgn, gencast_model, genda

    cls = {"denoiser": gencast_model.Denoiser, "genda": genda.GenDA, "fgn": fgn.FunctionalGenerativeNetwork}[so.MODEL_CASES[name][0]]
    return cls(**so.model_kwargs(name, sparse=sparse))


def test_alias_imports_give_the_sparse_classes():
    from graph_weather_amd import gencast_sparse

    with alias_modules():
        from graph_weather.models.gencast.layers.experimental import SparseAttention, SparseTransformer
        from graph_weather.models.gencast.layers.experimental.sparse_transformer import SparseTransformer as S2
    assert (SparseAttention, SparseTransformer, S2) == (gencast_sparse.SparseAttention, gencast_sparse.SparseTransformer,
                                                        gencast_sparse.SparseTransformer)


@pytest.mark.parametrize("name", list(so.CASES))
def test_state_dict_keys_order_shapes_and_attributes_equal_the_references(tables, name):
    module = so.build(_classes(), name, sparse="native")
    got = {k: list(v.shape) for k, v in module.state_dict().items()}
    assert list(got.items()) == list(tables["state_dict"][name].items())
    for attr in tables["attributes"][name]:
        assert hasattr(module, attr), attr


def test_class_attributes_of_the_two_classes():
    from graph_weather_amd import gencast, gencast_sparse

    att = gencast_sparse.SparseAttention(input_dim=12, output_dim=24, num_heads=4)
    assert (att.hidden_size, att.num_heads, att.head_dim, att.scaling) == (24, 4, 6, 6 ** -0.5)
    assert [n for n, _ in att.named_children()] == ["q_proj", "k_proj", "v_proj", "out_proj"]
    blk = gencast_sparse.SparseTransformer(conditioning_dim=5, input_dim=8, output_dim=8, num_heads=2, activation_layer=nn.SiLU,
                                           norm_first=False)
    assert [n for n, _ in blk.named_children()] == ["sparse_attention", "activation", "mlp", "cond_norm_1", "cond_norm_2"]
    assert isinstance(blk.activation, nn.SiLU) and blk.mlp[1] is blk.activation and blk.norm_first is False
    assert isinstance(blk.cond_norm_1, gencast.ConditionalLayerNorm) and isinstance(blk.mlp[0], nn.Linear)


@pytest.mark.parametrize("name", list(so.MODEL_CASES))
def test_models_take_a_reference_state_dict_strictly(tables, name):
    model = _model(name)
    want = tables["state_dict"][name]
    assert list({k: list(v.shape) for k, v in model.state_dict().items()}.items()) == list(want.items())
    rs = np.random.RandomState(5)
    sd = {k: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)) for k, shape in want.items()}
    assert model.load_state_dict(sd, strict=True).missing_keys == []
    assert torch.equal(model.processor.cond_transformers[1].sparse_attention.out_proj.weight,
                       sd["processor.cond_transformers.1.sparse_attention.out_proj.weight"])
    assert model.khop_mesh_edge_attr is None  # the k-hop edge attributes are not built


def test_sparse_true_still_raises_the_pinned_text_and_native_with_edges_raises_the_references():
    from graph_weather_amd import fgn, gencast

    with pytest.raises(ValueError, match=DGL_TEXT):
        gencast.Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16, noise_emb_dim=3,
                          sparse=True)
    with pytest.raises(ValueError, match=DGL_TEXT):
        fgn.Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, noise_emb_dim=3, sparse=True)
    with pytest.raises(ValueError, match=DGL_TEXT):
        gencast.Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16, noise_emb_dim=3,
                          sparse="dgl")
    for name in so.MODEL_CASES:
        kw = so.model_kwargs(name, sparse="native")
        kw["use_edges_features"] = True
        cls = type(_model(name))
        with pytest.raises(ValueError, match=EDGES_TEXT):
            cls(**kw)
        with pytest.raises(ValueError, match=DGL_TEXT):
            cls(**dict(kw, sparse=True, use_edges_features=False))
    plain = gencast.Processor(latent_dim=8, hidden_dims=[8, 8], num_blocks=2, num_heads=4, num_frequencies=4, base_period=16,
                              noise_emb_dim=3)
    assert type(plain.cond_transformers[0]).__name__ == "CondTransformerBlock"  # sparse=False behaves as before


def test_constructor_checks():
    from graph_weather_amd import gencast_sparse

    with pytest.raises(ValueError, match="Output dimension should be divisible by the number of heads."):
        gencast_sparse.SparseAttention(input_dim=8, output_dim=10, num_heads=4)
    with pytest.raises(ValueError, match="must be equal"):
        gencast_sparse.SparseTransformer(conditioning_dim=3, input_dim=8, output_dim=16, num_heads=4)
    with pytest.raises(NotImplementedError, match="nn.ReLU or nn.SiLU"):
        gencast_sparse.SparseTransformer(conditioning_dim=3, input_dim=8, output_dim=8, num_heads=4, activation_layer=nn.Tanh)
    gencast_sparse.SparseAttention(input_dim=8, output_dim=12, num_heads=3)  # different dims are fine for the attention alone


def test_cpu_tensors_raise_no_cpu_path():
    classes = _classes()
    for name in so.CASES:
        module, inp = so.build(classes, name, sparse="native"), so.case_inputs(name)
        with pytest.raises(RuntimeError, match="no CPU path"):
            so.call(module, name, inp)
    from graph_weather_amd import gencast_sparse

    with pytest.raises(RuntimeError, match="no CPU path"):
        gencast_sparse.sparse_plan(torch.tensor([[0, 1], [1, 0]]), 2)
    blk = so.build(classes, "gencast_sparse_block_pre_relu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        blk._forward_shared(torch.zeros(6, 64), torch.tensor([[0, 1], [1, 0]]), torch.zeros(2, 16), 2)


def test_configs_round_trip_native():
    from graph_weather_amd import fgn, gencast_model, genda

    lon, lat = so.model_grid()
    base = dict(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=5, hidden_dims=[16, 16], num_blocks=2, num_heads=4,
                splits=1, num_hops=1, sparse="native", use_edges_features=False)
    for cfg_cls, extra, model_cls in ((gencast_model.DenoiserConfig, {}, gencast_model.Denoiser), (genda.GenDAConfig, {}, genda.GenDA),
                                      (fgn.FunctionalGenerativeNetworkConfig, dict(noise_dimension=6), fgn.FunctionalGenerativeNetwork)):
        cfg = cfg_cls(**base, **extra)
        assert cfg.sparse == "native"
        again = cfg_cls(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg)})
        assert again.sparse == "native"
        model = again.build()
        assert isinstance(model, model_cls) and type(model.processor.cond_transformers[0]).__name__ == "SparseTransformer"
        assert json.loads(json.dumps({"sparse": cfg.sparse}))["sparse"] == "native"  # what the hub mixin's JSON holds
        hub = getattr(model, "_hub_mixin_config", None)
        if hub is not None:
            assert hub.get("sparse") == "native"


def test_head_major_index_is_the_interleave():
    from graph_weather_amd import gencast_sparse

    perm = gencast_sparse.head_major_index(3, 4)
    assert perm.tolist() == [d * 3 + h for h in range(3) for d in range(4)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_oracle_equals_a_dense_masked_softmax(dtype):
    """Direction (row edge_index[0] attends to column edge_index[1]) and the head interleave, independently of the stand-in."""
    rs = np.random.RandomState(9)
    N, nh, dh = 23, 3, 5
    ei = torch.from_numpy(so.sparse_graph(rs, N))
    assert len(set(zip(ei[0].tolist(), ei[1].tolist()))) == ei.shape[1]  # duplicate-free
    q, k, v = (torch.from_numpy(rs.standard_normal((N, nh * dh))).to(dtype) for _ in range(3))
    got = so.sparse_attention_core(q, k, v, ei, nh)
    want = so.dense_masked_attention(q, k, v, ei, nh)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert (got - want).abs().max().item() <= tol * want.abs().max().item()
    flipped = so.sparse_attention_core(q, k, v, ei.flip(0), nh)
    assert (flipped - want).abs().max().item() > 1e-2  # the transposed mask is another answer
    empty = torch.bincount(ei[0], minlength=N) == 0
    assert empty.any() and (got[empty] == 0).all()


@pytest.mark.parametrize("name", list(so.CASES))
def test_oracle_reproduces_the_references_layer_outputs(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    assert int(z["seed"]) == so.CASES[name][3] and np.array_equal(z["out"], z["train_out"])
    inp = so.case_inputs(name)
    for k, v in inp.items():
        assert np.array_equal(z[k], v.numpy()), k
    module = so.build(_classes(), name, sparse="native")
    want = torch.from_numpy(z["out"]).double()
    out32 = so.run(name, so.params(module, torch.float32), so.cast(inp, torch.float32))
    out64 = so.run(name, so.params(module, torch.float64), so.cast(inp, torch.float64))
    scale = want.abs().max().item()
    assert (out32.double() - want).abs().max().item() <= 2e-5 * scale
    assert (out64 - want).abs().max().item() <= 2e-5 * scale  # (the recording is float32 arithmetic)


@pytest.mark.parametrize("name", list(so.MODEL_CASES))
def test_oracle_reproduces_the_references_model_outputs(golden_dir, name):
    from . import gencast_model_oracle as mo

    z = np.load(os.path.join(golden_dir, name + ".npz"))
    model = so.fill_(_model(name), so.MODEL_CASES[name][3])
    assert int(z["khop_entries"]) == model.khop_mesh_edge_index.shape[1] and int(z["mesh_nodes"]) == model.khop_mesh_nodes.shape[0]
    kw, graphs, inputs = so.model_kwargs(name), mo.graph_tables(model), so.model_inputs(name)
    out = so.model_forward(name, so.params(model, torch.float32), kw, graphs, inputs)
    want = torch.from_numpy(z["out"])
    assert (out - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    if so.MODEL_CASES[name][0] == "genda":
        guided = so.model_forward(name, so.params(model, torch.float32), kw, graphs, inputs, guided=True)
        want = torch.from_numpy(z["guided"])
        assert (guided - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from graph_weather_amd import _lib

    L = _lib.lib()
    assert L.gw_version() == 19
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int32 * 64)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)

    def fwd(batch=1, n=2, E=2, H=2, dh=4, scale=0.5, row_ptr=ip, q=p, out=p, lse=p, ld=8):
        return L.gw_sparse_attention_forward(batch, n, n, E, H, dh, scale, row_ptr, ip, q, ld, p, 8, p, 8, out, 8, lse, None)

    assert fwd(batch=0) == -1 and fwd(n=-1) == -1 and fwd(E=-1) == -1 and fwd(H=0) == -1 and fwd(dh=0) == -1
    assert fwd(scale=float("nan")) == -1 and fwd(scale=float("inf")) == -1
    assert fwd(row_ptr=None) == -1 and fwd(q=None) == -1 and fwd(out=None) == -1 and fwd(lse=None) == -1 and fwd(ld=7) == -1
    assert b"gw_sparse_attention_forward" in L.gw_last_error()
    assert fwd(H=2, dh=4096) == -2 and b"4096" in L.gw_last_error()  # GW_E_UNSUPPORTED
    assert fwd(n=0) == 0 and fwd(E=0) == 0  # empty launches: GW_OK, nothing launched

    def bwd(batch=1, n=2, E=2, H=2, row=ip, dout=p, delta=p, dq=p, ld_dq=8):
        return L.gw_sparse_attention_backward(batch, n, n, E, H, 4, 0.5, ip, ip, row, ip, ip, p, 8, p, 8, p, 8, p, 8, dout, 8, p, delta,
                                              dq, ld_dq, p, 8, p, 8, None)

    assert bwd(batch=0) == -1 and bwd(n=-1) == -1 and bwd(H=0) == -1 and bwd(row=None) == -1 and bwd(dout=None) == -1
    assert bwd(delta=None) == -1 and bwd(dq=None) == -1 and bwd(ld_dq=7) == -1
    assert b"gw_sparse_attention_backward" in L.gw_last_error()
    assert bwd(H=2048) == -2 and bwd(E=0) == 0  # 2048 heads x 4 > 4096: GW_E_UNSUPPORTED
