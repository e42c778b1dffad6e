"""The CaFA models without a GPU: the fp64 restatement against the reference's recorded outputs, state_dict exchange with the
reference's key -> shape tables, the alias import paths, the host-side errors of the modules and of the new C entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from . import cafa_oracle as co
from .test_alias import alias_modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(co.CASES))
def test_restatement_reproduces_the_reference(golden_dir, name):
    import graph_weather_amd as gw

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg, (b, h, w), seed = co.CASES[name]
    assert int(g["seed"]) == seed and list(g["meta"]) == [cfg[k] for k in co.META_KEYS] + [b, h, w]
    out = torch.from_numpy(g["out"])
    model, x = co.build(gw, name)
    ref = co.forecaster(co.params(model), x.double(), cfg)
    assert tuple(ref.shape) == tuple(out.shape) == (b, cfg["output_channels"], h, w)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 1e-6, err
    assert torch.isfinite(ref).all() and ref.abs().max() > 0.1


def _ours(gw, key):
    from graph_weather_amd import cafa

    kind, _, name = key.partition(":")
    if kind == "CaFAForecaster":
        return co.build(gw, name)[0]
    return {"CaFAEncoder": lambda: cafa.CaFAEncoder(3, 16, 2), "CaFADecoder": lambda: cafa.CaFADecoder(16, 3, 2),
            "CaFAProcessor": lambda: cafa.CaFAProcessor(16, 2, 2, 8), "AxialAttention": lambda: cafa.AxialAttention(16, 2, 8),
            "FactorizedAttention": lambda: cafa.FactorizedAttention(16, 2, 8),
            "FactorizedTransformerBlock": lambda: cafa.FactorizedTransformerBlock(16, 2, 8)}[kind]()


def test_state_dict_tables_equal_the_reference_and_load_strictly(golden_dir):
    import graph_weather_amd as gw

    with open(os.path.join(golden_dir, "cafa_state_dict.json")) as f:
        tables = json.load(f)
    assert len(tables) == len(co.CASES) + 6
    for key, table in tables.items():
        model = _ours(gw, key)
        assert type(model).__name__ == key.partition(":")[0]
        ours = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert ours == table
        assert list(ours) == list(table)  # same order too
        res = model.load_state_dict({k: torch.full(shape, 0.5) for k, shape in table.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    depth2 = tables["CaFAForecaster:cafa_ref_32x64"]
    assert len(depth2) == 40
    for k in ("encoder.encoder.weight", "processor.blocks.0.attn.attn_height.to_qkv.weight", "processor.blocks.1.ffn.0.weight",
              "processor.blocks.1.ffn.3.weight", "decoder.decoder.weight"):
        assert k in depth2


def test_defaults_and_feed_forward_numbering():
    import inspect

    from graph_weather_amd import cafa

    sig = inspect.signature(cafa.CaFAForecaster.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[3:]] == [
        ("model_dim", 256), ("downsampling_factor", 2), ("processor_depth", 6), ("num_heads", 8), ("dim_head", 64),
        ("feedforward_multiplier", 4), ("dropout", 0.0)]
    ffn = cafa.FeedFoward(8, 4, 0.25)
    assert [type(m).__name__ for m in ffn] == ["Linear", "GELU", "Dropout", "Linear", "Dropout"]
    assert ffn[0].out_features == 32 and ffn[2].p == 0.25


def test_alias_paths_resolve_to_our_classes():
    import graph_weather_amd as gw
    from graph_weather_amd import cafa

    with alias_modules():
        from graph_weather.models.cafa import (AxialAttention, CaFADecoder, CaFAEncoder, CaFAForecaster, CaFAProcessor,
                                               FactorizedAttention, FactorizedTransformerBlock)
        from graph_weather.models.cafa.decoder import CaFADecoder as D2
        from graph_weather.models.cafa.encoder import CaFAEncoder as E2
        from graph_weather.models.cafa.factorize import AxialAttention as A2, FactorizedAttention as F2, \
            FactorizedTransformerBlock as B2, FeedFoward
        from graph_weather.models.cafa.model import CaFAForecaster as M2
        from graph_weather.models.cafa.processor import CaFAProcessor as P2

    assert CaFAForecaster is M2 is gw.CaFAForecaster is cafa.CaFAForecaster
    assert CaFAEncoder is E2 is gw.CaFAEncoder and CaFADecoder is D2 is gw.CaFADecoder and CaFAProcessor is P2 is gw.CaFAProcessor
    assert AxialAttention is A2 is gw.AxialAttention and FactorizedAttention is F2 is gw.FactorizedAttention
    assert FactorizedTransformerBlock is B2 is gw.FactorizedTransformerBlock and FeedFoward is cafa.FeedFoward


def test_product_does_not_import_einops():
    for path in [os.path.join(ROOT, "graph_weather_amd", "cafa.py")] + \
            [os.path.join(ROOT, "graph_weather", "models", "cafa", f) for f in os.listdir(os.path.join(ROOT, "graph_weather", "models", "cafa"))
             if f.endswith(".py")]:
        src = open(path).read()
        assert "import einops" not in src and "from einops" not in src, path


def test_cpu_tensor_and_bad_arguments_raise():
    import graph_weather_amd as gw
    from graph_weather_amd import cafa

    model, x = co.build(gw, "cafa_f1_9x17")
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cafa.CaFAEncoder(3, 8, 2)(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cafa.CaFAProcessor(8, 1, 2, 4)(torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cafa.CaFADecoder(8, 3, 2)(torch.zeros(1, 8, 4, 4))
    attn = cafa.AxialAttention(8, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        attn(torch.zeros(1, 3, 4, 8), axis=1)
    for axis in (0, 3, -1):
        with pytest.raises(ValueError, match="Axis must be 1"):
            attn(torch.zeros(1, 3, 4, 8), axis=axis)
    with pytest.raises(ValueError, match="Axis must be 1"):
        cafa.attention_axial_forward(torch.zeros(12, 24), 1, 3, 4, 0, 2, 4, 0.5)
    with pytest.raises(NotImplementedError, match="dim_head"):
        cafa.AxialAttention(8, 2, 160)
    with pytest.raises(NotImplementedError, match="dim_head"):
        gw.CaFAForecaster(3, 3, model_dim=16, processor_depth=1, num_heads=1, dim_head=160)
    assert gw.CaFAForecaster(3, 3, model_dim=16, processor_depth=1, num_heads=1, dim_head=128) is not None


def test_dropout_only_where_it_is_the_identity():
    import graph_weather_amd as gw

    model = gw.CaFAForecaster(3, 3, model_dim=16, processor_depth=1, num_heads=2, dim_head=8, dropout=0.1)
    x = torch.zeros(1, 3, 4, 4)
    model.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        model(x)
    with pytest.raises(NotImplementedError, match="dropout"):
        model.processor(torch.zeros(1, 16, 2, 2))
    with pytest.raises(NotImplementedError, match="dropout"):
        model.processor.blocks[0].attn.attn_width(torch.zeros(1, 2, 2, 16), axis=2)
    model.eval()  # dropout is the identity: the forward goes on to its first kernel, which a CPU tensor cannot reach
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(x)
    plain = gw.CaFAForecaster(3, 3, model_dim=16, processor_depth=1, num_heads=2, dim_head=8).train()
    with pytest.raises(RuntimeError, match="no CPU path"):
        plain(x)


def _bad(L, rc):
    assert rc == -1, rc
    assert b"bad arguments" in L.gw_last_error()


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from graph_weather_amd import _lib

    L = _lib.lib()
    st = (ctypes.c_int64 * 3)(96, 24, 24)
    p = 256  # any non-null address: nothing is launched
    fwd = lambda o=1, i=2, h=1, n=4, d=8, q=p, out=p, lse=p, sq=st, so=st: L.gw_attention_axial_forward(  # noqa: E731
        o, i, h, n, d, q, q, q, sq, 0.5, out, so, lse, None)
    for kw in (dict(q=None), dict(out=None), dict(lse=None), dict(sq=None), dict(so=None), dict(o=0), dict(i=0), dict(h=-1), dict(n=0),
               dict(d=0), dict(d=129), dict(d=160)):
        _bad(L, fwd(**kw))
        assert b"gw_attention_axial_forward" in L.gw_last_error()
    bwd = lambda o=1, i=2, h=1, n=4, d=8, q=p, dout=p, delta=p, dq=p, sd=st: L.gw_attention_axial_backward(  # noqa: E731
        o, i, h, n, d, q, q, q, st, 0.5, p, st, dout, st, p, delta, dq, dq, dq, sd, None)
    for kw in (dict(q=None), dict(dout=None), dict(delta=None), dict(dq=None), dict(sd=None), dict(o=0), dict(i=-3), dict(h=0), dict(n=0),
               dict(d=0), dict(d=160)):
        _bad(L, bwd(**kw))
        assert b"gw_attention_axial_backward" in L.gw_last_error()
    geo = dict(b=1, c=3, h=5, w=7, f=2, d=8)
    dims = lambda g: (g["b"], g["c"], g["h"], g["w"], g["f"], g["d"])  # noqa: E731
    assert L.gw_patch_workspace_bytes(*dims(geo)) == 1 * (8 + 1) * (12 + 1) * 4  # one slab of (dim + 1) x (c f f + 1) floats
    assert L.gw_patch_workspace_bytes(2, 78, 180, 360, 2, 256) == 32 * 257 * 313 * 4  # 32 400 patches: 32 slabs of 1 024
    for key in geo:
        g = dict(geo, **{key: 0})
        assert L.gw_patch_workspace_bytes(*dims(g)) == 0 and b"bad arguments" in L.gw_last_error()
        _bad(L, L.gw_patch_embed_forward(*dims(g), p, p, p, p, 8, None))
        _bad(L, L.gw_patch_embed_backward(*dims(g), p, p, p, 8, p, 1 << 20, p, p, p, None))
        _bad(L, L.gw_patch_expand_forward(*dims(g), p, 8, p, p, p, None))
        _bad(L, L.gw_patch_expand_backward(*dims(g), p, 8, p, p, p, 1 << 20, p, 8, p, p, None))
    d = dims(geo)
    _bad(L, L.gw_patch_embed_forward(*d, None, p, p, p, 8, None))
    _bad(L, L.gw_patch_embed_forward(*d, p, None, p, p, 8, None))
    _bad(L, L.gw_patch_embed_forward(*d, p, p, p, None, 8, None))
    _bad(L, L.gw_patch_embed_forward(*d, p, p, p, p, 7, None))             # ld_out < dim
    _bad(L, L.gw_patch_embed_backward(*d, p, p, None, 8, p, 1 << 20, p, p, p, None))
    _bad(L, L.gw_patch_embed_backward(*d, p, p, p, 8, p, 1 << 20, p, p, None, None))   # dweight without dbias
    _bad(L, L.gw_patch_embed_backward(*d, p, p, p, 8, p, 16, p, p, p, None))            # workspace too small
    _bad(L, L.gw_patch_embed_backward(*d, p, p, p, 8, None, 0, None, None, None, None))  # nothing asked for
    _bad(L, L.gw_patch_expand_forward(*d, None, 8, p, p, p, None))
    _bad(L, L.gw_patch_expand_forward(*d, p, 8, p, p, None, None))
    _bad(L, L.gw_patch_expand_forward(*d, p, 4, p, p, p, None))
    _bad(L, L.gw_patch_expand_backward(*d, p, 8, p, None, p, 1 << 20, p, 8, p, p, None))
    _bad(L, L.gw_patch_expand_backward(*d, p, 8, p, p, p, 1 << 20, p, 7, p, p, None))
    _bad(L, L.gw_patch_expand_backward(*d, p, 8, p, p, p, 16, p, 8, p, p, None))
