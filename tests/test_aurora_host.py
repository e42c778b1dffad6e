"""The Aurora models without a GPU: the fp64 restatement against the reference's recorded outputs, state_dict exchange with the
reference's key -> shape tables, the alias import paths, the host-side errors of the modules and of the new C entry points."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from . import aurora_oracle as ao
from .test_alias import alias_modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meta(name):
    _, cfg, spec, _ = ao.CASES[name]
    out = []
    for d in (cfg, spec):
        for v in d.values():
            for x in (v if isinstance(v, tuple) else (v,)):
                if isinstance(x, (bool, int)):
                    out.append(int(x))
    return out


@pytest.mark.parametrize("name", list(ao.CASES))
def test_restatement_reproduces_the_reference(golden_dir, name):
    from graph_weather_amd import aurora

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    kind, _, _, seed = ao.CASES[name]
    assert int(g["seed"]) == seed and list(g["meta"]) == _meta(name)
    out = torch.from_numpy(g["out"])
    module = ao.build(aurora, name)
    ref = ao.run(name, None if kind == "loss" else ao.params(module), ao.case_inputs(name))
    assert tuple(ref.shape) == tuple(out.shape)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s: the restatement differs from the reference's fp32 output by %.3e of the maximum" % (name, err))
    assert err <= 1e-6, err
    assert torch.isfinite(ref).all() and ref.abs().max() > 0.1
    if kind == "loss":
        assert (ref > 0.1).all()  # every term is active on this case


def test_the_lattice_keeps_every_pair_away_from_the_radius():
    pts = ao.lattice(23).astype(np.float64)
    assert pts.shape == (108, 2)
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    assert np.abs(d - 5.0).min() > 0.5
    assert 0.05 < (d < 5.0).mean() < 0.10
    with pytest.raises(AssertionError, match="too close to the radius"):
        ao.lattice(1, spacing=2.5, jitter=0.0)  # neighbours two steps apart lie at exactly 5 degrees


def _ours(key):
    from graph_weather_amd import aurora

    kind, _, name = key.partition(":")
    if name:
        return ao.build(aurora, name)
    return {"AuroraModel": lambda: aurora.AuroraModel(3, 2, latent_dim=32, num_layers=2), "Swin3DEncoder": aurora.Swin3DEncoder,
            "PerceiverProcessor": lambda: aurora.PerceiverProcessor(aurora.ProcessorConfig(
                input_dim=16, latent_dim=24, d_model=16, num_self_attention_layers=1, num_attention_heads=2)),
            "Decoder3D": aurora.Decoder3D}[kind]()


def test_state_dict_tables_equal_the_reference_and_load_strictly(golden_dir):
    with open(os.path.join(golden_dir, "aurora_state_dict.json")) as f:
        tables = json.load(f)
    assert len(tables) == len(ao.CASES) - 1 + 4
    for key, table in tables.items():
        model = _ours(key)
        assert type(model).__name__ == key.partition(":")[0]
        ours = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert ours == table
        assert list(ours) == list(table)  # same order too
        res = model.load_state_dict({k: torch.full(shape, 0.5) for k, shape in table.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    model2 = tables["AuroraModel"]
    assert len(model2) == 42
    for k in ("processor.layers.0.attention.in_proj_weight", "processor.layers.1.attention.in_proj_bias",
              "processor.layers.1.attention.out_proj.weight", "processor.layers.1.attention.out_proj.bias",
              "encoder.coord_encoder.0.weight", "decoder.decoder.2.bias"):
        assert k in model2
    swin = tables["Swin3DEncoder"]
    assert len(swin) == 128
    for k in ("swin_transformer.encoder.norm.weight", "swin_transformer.decoder.layers.3.multihead_attn.in_proj_weight",
              "swin_transformer.decoder.norm.bias", "conv1.weight"):
        assert k in swin
    assert swin["conv1.weight"] == [96, 1, 3, 3, 3] and tables["Decoder3D"]["deconv1.weight"] == [96, 1, 3, 3, 3]


def test_constructor_signatures_and_defaults():
    from graph_weather_amd import aurora

    def sig(f):
        return [(k, p.default) for k, p in list(inspect.signature(f).parameters.items())[1:]]

    e = inspect.Parameter.empty
    assert sig(aurora.AuroraModel.__init__) == [("input_features", e), ("output_features", e), ("latent_dim", 256), ("num_layers", 4),
                                                ("max_points", 10000), ("max_seq_len", 1024), ("use_checkpointing", False)]
    assert sig(aurora.EarthSystemLoss.__init__) == [("alpha", 0.5), ("beta", 0.3), ("gamma", 0.2)]
    assert sig(aurora.Swin3DEncoder.__init__) == [("in_channels", 1), ("embed_dim", 96)]
    assert sig(aurora.Decoder3D.__init__) == [("output_channels", 1), ("embed_dim", 96), ("target_shape", (32, 32, 32))]
    assert sig(aurora.PerceiverProcessor.__init__) == [("config", None)]
    assert sig(aurora.PointEncoder.__init__) == [("input_features", e), ("embed_dim", e), ("max_seq_len", 1024)]
    assert sig(aurora.PointCloudProcessor.__init__) == [("embed_dim", e), ("num_layers", 4)]
    cfg = aurora.ProcessorConfig()
    assert (cfg.input_dim, cfg.latent_dim, cfg.d_model, cfg.max_seq_len, cfg.num_self_attention_layers, cfg.num_cross_attention_layers,
            cfg.num_attention_heads, cfg.hidden_dropout, cfg.attention_dropout, cfg.qk_head_dim, cfg.activation_fn,
            cfg.layer_norm_eps) == (256, 512, 256, 4096, 6, 2, 8, 0.1, 0.1, 32, "gelu", 1e-12)
    model = aurora.AuroraModel(3, 2, latent_dim=32, num_layers=1)
    assert model.processor.layers[0].attention.num_heads == 8 and model.processor.layers[0].attention.dropout == 0.0
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in model.modules() if isinstance(m, torch.nn.Linear))  # _init_weights
    w = model.decoder.decoder[0].weight
    assert float(w.detach().abs().max()) <= (6.0 / 64) ** 0.5 + 1e-6  # Xavier-uniform bound of a [32, 32] matrix
    swin = aurora.Swin3DEncoder()
    assert swin.swin_transformer.encoder.layers[0].self_attn.embed_dim // 8 == 12
    assert aurora.create_loss(0.1, 0.2, 0.7).gamma == 0.7 and sorted(aurora.MODEL_CONFIGS) == ["base", "large", "tiny"]
    with pytest.raises(ValueError, match="Unknown configuration"):
        aurora.create_model("huge")
    assert aurora.__all__ == ["AuroraModel", "EarthSystemLoss", "Swin3DEncoder", "Decoder3D", "PerceiverProcessor"]


def test_processor_config_validation():
    from graph_weather_amd.aurora import ProcessorConfig

    for kw in (dict(input_dim=0), dict(max_seq_len=0), dict(num_attention_heads=0), dict(hidden_dropout=1.5), dict(attention_dropout=-0.1)):
        with pytest.raises(ValueError):
            ProcessorConfig(**kw)


def test_alias_paths_resolve_to_our_classes():
    import graph_weather_amd as gw
    from graph_weather_amd import aurora

    with alias_modules():
        from graph_weather.models.aurora import (MODEL_CONFIGS, AuroraModel, Decoder3D, EarthSystemLoss, PerceiverProcessor,
                                                 Swin3DEncoder, create_loss, create_model)
        from graph_weather.models.aurora import __all__ as names
        from graph_weather.models.aurora.decoder import Decoder3D as D2
        from graph_weather.models.aurora.encoder import Swin3DEncoder as S2
        from graph_weather.models.aurora.model import AuroraModel as M2, EarthSystemLoss as L2, PointCloudProcessor, PointDecoder, \
            PointEncoder, SelfAttentionLayer
        from graph_weather.models.aurora.processor import PerceiverProcessor as P2, ProcessorConfig

    assert AuroraModel is M2 is gw.AuroraModel is aurora.AuroraModel and EarthSystemLoss is L2 is gw.EarthSystemLoss
    assert Swin3DEncoder is S2 is gw.Swin3DEncoder and Decoder3D is D2 is gw.Decoder3D
    assert PerceiverProcessor is P2 is gw.PerceiverProcessor and ProcessorConfig is gw.ProcessorConfig
    assert PointEncoder is gw.PointEncoder and PointDecoder is gw.PointDecoder and PointCloudProcessor is gw.PointCloudProcessor
    assert SelfAttentionLayer is gw.SelfAttentionLayer
    assert create_loss is aurora.create_loss and create_model is aurora.create_model and MODEL_CONFIGS is aurora.MODEL_CONFIGS
    assert names == aurora.__all__


def test_product_and_oracle_imports():
    paths = [os.path.join(ROOT, "graph_weather_amd", "aurora.py")] + \
        [os.path.join(ROOT, "graph_weather", "models", "aurora", f) for f in os.listdir(os.path.join(ROOT, "graph_weather", "models", "aurora"))
         if f.endswith(".py")]
    for path in paths:
        src = open(path).read()
        assert "import einops" not in src and "from einops" not in src, path
    oracle_src = open(os.path.join(ROOT, "tests", "aurora_oracle.py")).read().partition('"""\nfrom __future__')[2]
    assert "MultiheadAttention" not in oracle_src and "einops" not in oracle_src and "refload" not in oracle_src


def test_host_side_errors():
    from graph_weather_amd import aurora

    model = aurora.AuroraModel(3, 2, latent_dim=32, num_layers=1, max_points=50)
    with pytest.raises(ValueError, match="exceeds maximum"):
        model(torch.zeros(1, 51, 2), torch.zeros(1, 51, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 10, 2), torch.zeros(1, 10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.encoder(torch.zeros(1, 10, 2), torch.zeros(1, 10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.processor(torch.zeros(1, 10, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.decoder(torch.zeros(1, 10, 32))
    with pytest.raises(NotImplementedError, match="dim_head"):
        aurora.AuroraModel(3, 2, latent_dim=8 * 160, num_layers=1)

    loss = aurora.EarthSystemLoss()
    pred, pts = torch.zeros(2, 6, 3), torch.zeros(2, 6, 2)
    with pytest.raises(RuntimeError, match="one sample"):
        loss(pred, pred, pts)
    with pytest.raises(RuntimeError, match="one sample"):
        loss.spatial_correlation_loss(pred, pred, pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(pred[:1], pred[:1], pts[:1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.physical_loss(pred, pts)

    proc = aurora.PerceiverProcessor(aurora.ProcessorConfig(input_dim=8, latent_dim=8, d_model=16, num_self_attention_layers=1,
                                                            num_attention_heads=2, hidden_dropout=0.0)).eval()
    with pytest.raises(RuntimeError, match="4 dimensions"):
        proc(torch.zeros(1, 2, 3, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        proc(torch.zeros(1, 5, 8))

    dec = aurora.Decoder3D(1, 3, (2, 2, 2))
    with pytest.raises(RuntimeError, match="view size is not compatible"):
        dec(torch.zeros(1, 3, 8).transpose(1, 2))  # [1, 8, 3] rows that do not lie as [1, 3, 2, 2, 2]
    with pytest.raises(RuntimeError, match="no CPU path"):
        dec(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        aurora.Swin3DEncoder(1, 16).eval()(torch.zeros(1, 1, 2, 2, 2))


def test_dropout_only_where_it_is_the_identity():
    from graph_weather_amd import aurora

    swin = aurora.Swin3DEncoder(1, 16)
    x = torch.zeros(1, 1, 2, 2, 2)
    with pytest.raises(NotImplementedError, match="dropout"):
        swin.train()(x)
    with pytest.raises(RuntimeError, match="no CPU path"):  # eval(): the forward goes on to its first kernel
        swin.eval()(x)
    cfg = dict(input_dim=8, latent_dim=8, d_model=16, num_self_attention_layers=1, num_attention_heads=2)
    proc = aurora.PerceiverProcessor(aurora.ProcessorConfig(**cfg))
    with pytest.raises(NotImplementedError, match="dropout"):
        proc.train()(torch.zeros(1, 5, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        proc.eval()(torch.zeros(1, 5, 8))
    plain = aurora.PerceiverProcessor(aurora.ProcessorConfig(hidden_dropout=0.0, **cfg)).train()
    with pytest.raises(RuntimeError, match="no CPU path"):
        plain(torch.zeros(1, 5, 8))
    model = aurora.AuroraModel(3, 2, latent_dim=32, num_layers=1).train()  # no dropout anywhere: trains as it is
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 10, 2), torch.zeros(1, 10, 3))


def _bad(L, rc, name):
    assert rc == -1, (name, rc)
    assert b"bad arguments" in L.gw_last_error() and name.encode() in L.gw_last_error()


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from graph_weather_amd import _lib

    L = _lib.lib()
    st = (ctypes.c_int64 * 3)(96, 0, 24)
    p = 256  # any non-null address: nothing is launched
    fwd = lambda o=1, i=1, h=1, n=4, d=8, q=p, bias=p, out=p, lse=p, sq=st, so=st: L.gw_attention_masked_forward(  # noqa: E731
        o, i, h, n, d, q, q, q, sq, bias, 0.5, out, so, lse, None)
    for kw in (dict(q=None), dict(bias=None), dict(out=None), dict(lse=None), dict(sq=None), dict(so=None), dict(o=0), dict(i=0),
               dict(h=-1), dict(n=0), dict(d=0), dict(d=129)):
        _bad(L, fwd(**kw), "gw_attention_masked_forward")
    bwd = lambda o=1, i=1, h=1, n=4, d=8, q=p, bias=p, dout=p, delta=p, dq=p, sd=st: L.gw_attention_masked_backward(  # noqa: E731
        o, i, h, n, d, q, q, q, st, bias, 0.5, p, st, dout, st, p, delta, dq, dq, dq, sd, None)
    for kw in (dict(q=None), dict(bias=None), dict(dout=None), dict(delta=None), dict(dq=None), dict(sd=None), dict(o=0), dict(i=-3),
               dict(h=0), dict(n=0), dict(d=0), dict(d=160)):
        _bad(L, bwd(**kw), "gw_attention_masked_backward")

    # EarthSystemLoss: partials of 4 + 2 + 1 doubles for one workgroup of each kernel
    assert L.gw_earth_loss_workspace_bytes(1, 32, 3) == 7 * 8
    assert L.gw_earth_loss_workspace_bytes(1, 10000, 78) == (4 * 762 + 2 * 40 + 313) * 8
    for dims in ((0, 4, 3), (1, 0, 3), (1, 4, 0)):
        assert L.gw_earth_loss_workspace_bytes(*dims) == 0 and b"bad arguments" in L.gw_last_error()
    lf = lambda b=1, n=4, c=3, pred=p, target=p, pts=p, sp=1, ws=p, nb=1 << 12, out=p, G=p, stats=p: L.gw_earth_loss_forward(  # noqa: E731
        b, n, c, pred, target, pts, sp, 0.5, 0.3, 0.2, ws, nb, out, G, stats, None)
    for kw in (dict(pred=None), dict(pts=None), dict(ws=None), dict(out=None), dict(stats=None), dict(target=None), dict(G=None),
               dict(b=2), dict(b=0), dict(n=0), dict(c=0), dict(nb=8), dict(ws=260)):
        _bad(L, lf(**kw), "gw_earth_loss_forward")
    assert lf(c=129) == -2 and b"128 channels" in L.gw_last_error()  # GW_E_UNSUPPORTED, nothing launched
    lb = lambda b=1, n=4, c=3, pred=p, target=p, pts=p, sp=1, G=p, stats=p, gout=p, dp=p, dt=p: L.gw_earth_loss_backward(  # noqa: E731
        b, n, c, pred, target, pts, sp, 0.5, 0.3, 0.2, G, stats, gout, dp, dt, None)
    for kw in (dict(pred=None), dict(pts=None), dict(stats=None), dict(gout=None), dict(dp=None, dt=None), dict(target=None),
               dict(G=None), dict(b=2), dict(n=0), dict(c=-1)):
        _bad(L, lb(**kw), "gw_earth_loss_backward")

    _bad(L, L.gw_token_mean_forward(1, 4, 8, None, 8, p, 8, None), "gw_token_mean_forward")
    _bad(L, L.gw_token_mean_forward(1, 4, 8, p, 8, None, 8, None), "gw_token_mean_forward")
    _bad(L, L.gw_token_mean_forward(0, 4, 8, p, 8, p, 8, None), "gw_token_mean_forward")
    _bad(L, L.gw_token_mean_forward(1, 0, 8, p, 8, p, 8, None), "gw_token_mean_forward")
    _bad(L, L.gw_token_mean_forward(1, 4, 8, p, 7, p, 8, None), "gw_token_mean_forward")
    _bad(L, L.gw_token_mean_backward(1, 4, 8, None, 8, p, 8, None), "gw_token_mean_backward")
    _bad(L, L.gw_token_mean_backward(1, 4, 8, p, 8, p, 7, None), "gw_token_mean_backward")
    _bad(L, L.gw_token_mean_backward(1, 4, 0, p, 8, p, 8, None), "gw_token_mean_backward")
    _bad(L, L.gw_relu_forward(4, None, p, None), "gw_relu_forward")
    _bad(L, L.gw_relu_forward(-1, p, p, None), "gw_relu_forward")
    _bad(L, L.gw_row_scale(4, 3, p, 3, None, p, 3, None), "gw_row_scale")
    _bad(L, L.gw_row_scale(4, 3, p, 2, p, p, 3, None), "gw_row_scale")
    _bad(L, L.gw_row_scale(4, 0, p, 3, p, p, 3, None), "gw_row_scale")

    # 3 x 3 x 3 convolutions: one partial of (cout + 1) x (27 cin + 1) floats per slab of 1024 voxels (transposed: (cin + 1) x (27 cout + 1))
    assert L.gw_conv3d_workspace_bytes(2, 3, 8, 8, 9, 17, 0) == 3 * 9 * 82 * 4
    assert L.gw_conv3d_workspace_bytes(2, 96, 1, 8, 9, 17, 1) == 3 * 97 * 28 * 4
    geo = dict(b=1, ci=2, co=4, d=3, h=4, w=5)
    dims = lambda g, t=0: (g["b"], g["ci"], g["co"], g["d"], g["h"], g["w"], t)  # noqa: E731
    for key in geo:
        g = dict(geo, **{key: 0})
        assert L.gw_conv3d_workspace_bytes(*dims(g)) == 0 and b"bad arguments" in L.gw_last_error()
        _bad(L, L.gw_conv3d_forward(*dims(g), p, st, p, p, p, st, None), "gw_conv3d_forward")
        _bad(L, L.gw_conv3d_backward(*dims(g, 1), p, st, p, p, st, p, 1 << 20, p, st, p, p, None), "gw_conv3d_backward")
    d = dims(geo)
    _bad(L, L.gw_conv3d_forward(*d, None, st, p, p, p, st, None), "gw_conv3d_forward")
    _bad(L, L.gw_conv3d_forward(*d, p, None, p, p, p, st, None), "gw_conv3d_forward")
    _bad(L, L.gw_conv3d_forward(*d, p, st, None, p, p, st, None), "gw_conv3d_forward")
    _bad(L, L.gw_conv3d_forward(*d, p, st, p, p, None, st, None), "gw_conv3d_forward")
    _bad(L, L.gw_conv3d_forward(*d, p, st, p, p, p, None, None), "gw_conv3d_forward")
    _bad(L, L.gw_conv3d_backward(*d, p, st, p, None, st, p, 1 << 20, p, st, p, p, None), "gw_conv3d_backward")
    _bad(L, L.gw_conv3d_backward(*d, p, st, p, p, st, p, 1 << 20, p, st, p, None, None), "gw_conv3d_backward")   # dweight without dbias
    _bad(L, L.gw_conv3d_backward(*d, p, st, p, p, st, p, 16, p, st, p, p, None), "gw_conv3d_backward")            # workspace too small
    _bad(L, L.gw_conv3d_backward(*d, p, st, p, p, st, None, 0, None, st, None, None, None), "gw_conv3d_backward")  # nothing asked for
    _bad(L, L.gw_conv3d_backward(*d, p, st, p, p, st, p, 1 << 20, p, None, p, p, None), "gw_conv3d_backward")     # dx without strides

    # the ordered weight-gradient kernels: one partial of m x (n + 1) floats per slab of 1024 rows; LayerNorm: (mean, rstd) per row and
    # two rows of `width` per slab of 256 rows
    assert L.gw_gemm_tn_ordered_workspace_bytes(70, 130, 2500) == 3 * 70 * 131 * 4
    assert L.gw_layernorm_backward_ordered_workspace_bytes(300, 96) == (2 * 300 + 2 * 2 * 96) * 4
    for dims in ((0, 4, 8), (4, 0, 8), (4, 4, 0)):
        assert L.gw_gemm_tn_ordered_workspace_bytes(*dims) == 0 and b"bad arguments" in L.gw_last_error()
    for dims in ((0, 8), (4, 0), (4, 4097)):
        assert L.gw_layernorm_backward_ordered_workspace_bytes(*dims) == 0 and b"bad arguments" in L.gw_last_error()
    tn = lambda m=4, n=3, rows=8, a=p, lda=4, b=p, ldb=3, ws=p, nb=1 << 12, c=p, ldc=3: L.gw_gemm_tn_ordered(  # noqa: E731
        m, n, rows, a, lda, b, ldb, ws, nb, c, ldc, None, None)
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(ws=None), dict(m=0), dict(n=0), dict(rows=0), dict(lda=3), dict(ldb=2),
               dict(ldc=2), dict(nb=16)):
        _bad(L, tn(**kw), "gw_gemm_tn_ordered")
    ln = lambda rows=8, w=16, dn=p, ld=16, y=p, g=p, ws=p, nb=1 << 12, dy=p, dg=p, db=p: L.gw_layernorm_backward_ordered(  # noqa: E731
        rows, w, dn, ld, y, ld, g, ws, nb, dy, ld, dg, db, None)
    for kw in (dict(dn=None), dict(y=None), dict(g=None), dict(ws=None), dict(dy=None), dict(dg=None), dict(db=None), dict(rows=0),
               dict(w=0), dict(w=4097), dict(ld=8), dict(nb=16)):
        _bad(L, ln(**kw), "gw_layernorm_backward_ordered")
