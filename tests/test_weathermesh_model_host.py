"""WeatherMesh's blocks, encoder, decoder and model on the host: the recorded ``state_dict`` tables and signatures, the alias import
paths, the nested configs, every argument the classes refuse, the output-length formula and the upsampling weights.  No GPU."""
import dataclasses
import inspect
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import graph_weather_amd
from graph_weather_amd import _lib, weathermesh, weathermesh_model as wm

from . import weathermesh_model_oracle as mo
from .test_alias import alias_modules

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorded():
    with open(os.path.join(GOLDEN, "weathermesh_model_state_dict.json")) as f:
        return json.load(f)


def _signature(cls):
    out = []
    for name, prm in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = prm.default
        out.append([name, "<required>" if d is inspect.Parameter.empty else
                    d if isinstance(d, (bool, int, float, list, type(None))) else str(d)])
    return out


def test_model_state_dict_equals_the_recorded_one_loads_strictly_and_holds_no_processors():
    rec = _recorded()
    for name in mo.CASES:
        model = wm.WeatherMesh(**mo.MODEL_KW)
        table = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert table == rec["state_dict"][name] and list(table) == list(rec["state_dict"][name])  # the order too
        sd = {k: torch.zeros(s, dtype=model.state_dict()[k].dtype) for k, s in rec["state_dict"][name].items()}
        model.load_state_dict(sd, strict=True)
        assert not any(k.startswith("processors") for k in table)
        assert isinstance(model.processors, list) and len(model.processors) == 2
        own = {id(p) for p in model.parameters()}
        assert all(id(p) not in own for q in model.processors for p in q.parameters())
        assert model.timesteps == [1, 6]


def test_block_state_dicts_equal_the_recorded_ones_and_children_are_torch_modules():
    rec = _recorded()["state_dict"]
    blocks = {"ConvDownBlock(3, 8)": wm.ConvDownBlock(3, 8),
              "ConvDownBlock(4, 8, stride=(1, 2, 2), is_3d=True)": wm.ConvDownBlock(4, 8, stride=(1, 2, 2), is_3d=True),
              "ConvUpBlock(8, 3)": wm.ConvUpBlock(8, 3), "ConvUpBlock(16, 5, is_3d=True)": wm.ConvUpBlock(16, 5, is_3d=True)}
    for key, block in blocks.items():
        table = {k: list(v.shape) for k, v in block.state_dict().items()}
        assert table == rec[key] and list(table) == list(rec[key]), key
        block.load_state_dict({k: torch.zeros(s, dtype=block.state_dict()[k].dtype) for k, s in rec[key].items()}, strict=True)
    down, up = blocks["ConvDownBlock(4, 8, stride=(1, 2, 2), is_3d=True)"], blocks["ConvUpBlock(8, 3)"]
    assert list(down._modules) == ["conv1", "bn1", "activation1", "conv2", "bn2", "activation2", "downsample", "bn_down"]
    assert list(up._modules) == ["conv1", "bn1", "activation1", "conv2", "bn2", "activation2", "upsample", "bn_up"]
    assert down.activation1 is down.activation2  # one instance under two names, as in the reference
    assert isinstance(down.conv1, nn.Conv3d) and isinstance(down.bn_down, nn.BatchNorm3d) and down.conv1.bias is None
    assert down.conv1.stride == (1, 1, 1) and down.conv2.stride == (1, 2, 2) and down.downsample.stride == (1, 2, 2)
    assert down.downsample.kernel_size == (1, 1, 1) and down.bn1.eps == 1e-5 and down.bn1.momentum == 0.1
    assert isinstance(up.conv1, nn.Conv2d) and (up.conv1.in_channels, up.conv1.out_channels, up.conv2.out_channels) == (8, 8, 3)
    assert up.is_3d is False and up.scale_factor == 2 and up.upsample.kernel_size == (1, 1) and up.upsample.stride == (1, 1)


def test_signatures_config_fields_and_output_fields_equal_the_recorded_ones():
    rec = _recorded()
    for name in ("ConvDownBlock", "ConvUpBlock", "WeatherMeshEncoder", "WeatherMeshDecoder", "WeatherMesh"):
        assert _signature(getattr(wm, name)) == rec["signature"][name], name
    assert len(rec["signature"]["WeatherMesh"]) == 17 and all(d == "<required>" for _, d in rec["signature"]["WeatherMesh"])
    for name, fields in rec["config_fields"].items():
        assert [[f.name, mo.type_name(f.type)] for f in dataclasses.fields(getattr(wm, name))] == fields, name
    assert [f.name for f in dataclasses.fields(wm.WeatherMeshOutput)] == rec["output_fields"] == ["surface", "pressure"]


def test_encoder_and_decoder_structure():
    enc = wm.WeatherMeshEncoder(3, 4, 8, n_pressure_levels=99, num_conv_blocks=2, hidden_dim=4, kernel_size=(3, 3, 3), num_heads=2,
                                num_transformer_layers=1)
    assert [(b.conv1.in_channels, b.conv2.out_channels) for b in enc.surface_path] == [(3, 8), (8, 16)]
    assert [(b.conv1.in_channels, b.conv2.out_channels) for b in enc.pressure_path] == [(4, 8), (8, 16)]
    assert all(isinstance(b.conv1, nn.Conv2d) and b.conv2.stride == (2, 2) for b in enc.surface_path)
    assert all(isinstance(b.conv1, nn.Conv3d) and b.conv2.stride == (1, 2, 2) for b in enc.pressure_path)
    assert isinstance(enc.to_latent, nn.Conv3d) and enc.to_latent.weight.shape == (8, 16, 1, 1, 1) and enc.to_latent.bias is not None
    assert isinstance(enc.transformer_layers[0], weathermesh.NeighborhoodAttention3D)
    dec = wm.WeatherMeshDecoder(8, 3, 4, n_conv_blocks=2, hidden_dim=4, kernel_size=(3, 3, 3), num_heads=2, num_transformer_layers=1)
    assert [(b.conv1.in_channels, b.conv2.out_channels) for b in dec.pressure_path] == [(16, 8), (8, 4)]
    assert [(b.conv1.in_channels, b.conv2.out_channels) for b in dec.surface_path] == [(16, 8), (8, 3)]
    assert dec.split.weight.shape == (16, 8, 1, 1, 1) and [n for n, _ in dec.named_children()][:2] == ["transformer_layers", "split"]
    default = wm.WeatherMeshEncoder(2, 2, 16, 13, hidden_dim=2)
    assert len(default.surface_path) == 3 and len(default.transformer_layers) == 3
    assert default.transformer_layers[0].kernel_size == (5, 7, 7) and default.transformer_layers[0].num_heads == 8
    given = wm.WeatherMesh(enc, [weathermesh.WeatherMeshProcessor(8, 1, 3, 2)], dec, [6], *([None] * 13))
    assert given.encoder is enc and given.decoder is dec and len(given.processors) == 1
    with pytest.raises(AssertionError, match="Number of processors"):
        wm.WeatherMesh(enc, [], dec, [6], *([None] * 13))


def test_alias_import_paths_resolve_to_these_classes():
    with alias_modules():
        import graph_weather.models.weathermesh as pkg
        from graph_weather.models.weathermesh.decoder import WeatherMeshDecoder, WeatherMeshDecoderConfig
        from graph_weather.models.weathermesh.encoder import WeatherMeshEncoder, WeatherMeshEncoderConfig
        from graph_weather.models.weathermesh.layers import ConvDownBlock, ConvUpBlock
        from graph_weather.models.weathermesh.weathermesh2 import WeatherMesh, WeatherMeshConfig, WeatherMeshOutput

        here = os.path.dirname(os.path.abspath(pkg.__file__))
    got = dict(ConvDownBlock=ConvDownBlock, ConvUpBlock=ConvUpBlock, WeatherMeshEncoder=WeatherMeshEncoder,
               WeatherMeshEncoderConfig=WeatherMeshEncoderConfig, WeatherMeshDecoder=WeatherMeshDecoder,
               WeatherMeshDecoderConfig=WeatherMeshDecoderConfig, WeatherMesh=WeatherMesh, WeatherMeshConfig=WeatherMeshConfig,
               WeatherMeshOutput=WeatherMeshOutput)
    for name, cls in got.items():
        assert cls is getattr(wm, name) is getattr(graph_weather_amd, name) is getattr(pkg, name), name
    # the four are sub-package directories: the .py files of the package stay the two that tests/test_weathermesh_host.py expects
    assert sorted(f for f in os.listdir(here) if f.endswith(".py")) == ["__init__.py", "processor.py"]
    for sub in ("layers", "encoder", "decoder", "weathermesh2"):
        assert os.listdir(os.path.join(here, sub)) == ["__init__.py"] or sorted(os.listdir(os.path.join(here, sub))) == ["__init__.py", "__pycache__"]


def test_nested_config_round_trip_and_type_errors():
    rec = _recorded()
    cfg = wm.WeatherMeshConfig.from_json(mo.CONFIG_JSON)
    assert isinstance(cfg.encoder, wm.WeatherMeshEncoderConfig) and isinstance(cfg.decoder, wm.WeatherMeshDecoderConfig)
    assert len(cfg.processors) == 2 and all(isinstance(p, weathermesh.WeatherMeshProcessorConfig) for p in cfg.processors)
    assert cfg.encoder.kernel_size == (3, 3, 3) and cfg.processors[1].kernel == (3, 3, 3) and cfg.timesteps == [1, 6]
    assert cfg.to_json() == dataclasses.asdict(cfg) == mo.CONFIG_JSON

    def lists(v):  # JSON has no tuples
        return {k: lists(x) for k, x in v.items()} if isinstance(v, dict) else [lists(x) for x in v] if isinstance(v, (list, tuple)) else v

    assert lists(cfg.to_json()) == rec["config_round_trip"]
    assert wm.WeatherMeshConfig.from_json(cfg.to_json()) == cfg
    assert wm.WeatherMeshConfig.from_json(dict(mo.CONFIG_JSON, encoder=cfg.encoder)) == cfg  # an instance is taken as it is
    enc = wm.WeatherMeshEncoderConfig.from_json(mo.CONFIG_JSON["encoder"])
    assert enc == cfg.encoder and enc.to_json() == mo.CONFIG_JSON["encoder"]
    wm.WeatherMeshEncoder(**enc.to_json())
    wm.WeatherMeshDecoder(**wm.WeatherMeshDecoderConfig.from_json(mo.CONFIG_JSON["decoder"]).to_json())
    with pytest.raises(ValueError, match="missing value"):
        wm.WeatherMeshConfig.from_json({k: v for k, v in mo.CONFIG_JSON.items() if k != "decoder"})
    with pytest.raises(ValueError, match="missing value"):
        wm.WeatherMeshConfig.from_json(dict(mo.CONFIG_JSON, encoder={"latent_dim": 8}))
    for bad in (dict(kernel=[3, 3, 3]), dict(latent_dim="8"), dict(encoder=3), dict(processors=mo.CONFIG_JSON["processors"][0]),
                dict(timesteps=(1, 6)), dict(timesteps=[1, "6"]), dict(processors=[dict(mo.CONFIG_JSON["processors"][0], kernel=[3, 3, 3])]),
                dict(decoder=dict(mo.CONFIG_JSON["decoder"], hidden_dim=4.0))):
        with pytest.raises(TypeError, match="wrong value type"):
            wm.WeatherMeshConfig.from_json(dict(mo.CONFIG_JSON, **bad))
    with pytest.raises(TypeError, match="wrong value type"):
        wm.WeatherMeshDecoderConfig.from_json(dict(mo.CONFIG_JSON["decoder"], kernel_size=[3, 3, 3]))


def test_refused_arguments():
    for cls in (wm.ConvDownBlock, wm.ConvUpBlock):
        for kw in (dict(groups=2), dict(kernel_size=5), dict(kernel_size=1), dict(padding=0), dict(padding=2), dict(activation=nn.ReLU()),
                   dict(activation=nn.GELU(approximate="tanh")), dict(activation=nn.SiLU())):
            with pytest.raises(NotImplementedError, match="not built"):
                cls(4, 8, **kw)
        cls(4, 8, activation=nn.GELU())
    for stride in (3, 4, (2, 3), 0):
        with pytest.raises(NotImplementedError, match="not built"):
            wm.ConvDownBlock(4, 8, stride=stride)
    with pytest.raises(NotImplementedError, match="not built"):
        wm.ConvDownBlock(4, 8, stride=(1, 2, 4), is_3d=True)
    wm.ConvDownBlock(4, 8, stride=1), wm.ConvDownBlock(4, 8, stride=(2, 1)), wm.ConvDownBlock(4, 8, stride=(2, 2, 2), is_3d=True)
    for scale in (1, 3, 4, (1, 2, 2)):
        with pytest.raises(NotImplementedError, match="not built"):
            wm.ConvUpBlock(8, 4, scale_factor=scale)


def test_cpu_and_non_fp32_tensors_and_wrong_channel_counts_are_refused():
    down, up = wm.ConvDownBlock(3, 8), wm.ConvUpBlock(8, 3, is_3d=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        down(torch.zeros(2, 3, 6, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        up(torch.zeros(2, 8, 2, 3, 3))
    for fn in (wm.upsample2x_forward, wm.upsample2x_backward):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros(1, 1, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        wm.convnd_forward(torch.zeros(1, 3, 4, 4), down.conv1.weight, 1)
    model = wm.WeatherMesh(**mo.MODEL_KW)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(2, 3, 13, 18), torch.zeros(2, 4, 3, 13, 18), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.decoder(torch.zeros(2, 4, 4, 5, 8))
    with pytest.raises(RuntimeError, match="float32"):  # the dtype is checked where the device is
        wm._need_hip(_FakeHalf(), "x")
    for bad in (torch.zeros(2, 4, 6, 6), torch.zeros(2, 3, 2, 6, 6), torch.zeros(3, 6, 6)):
        with pytest.raises(ValueError, match="expects"):
            down(bad)
    with pytest.raises(ValueError, match="expects"):
        up(torch.zeros(2, 3, 2, 3, 3))
    with pytest.raises(ValueError, match="expects"):
        model(torch.zeros(2, 3, 13, 18), torch.zeros(2, 4, 3, 13, 17), 1)
    with pytest.raises(ValueError, match="expects"):
        model.decoder(torch.zeros(2, 4, 4, 5, 7))


class _FakeHalf:
    """What ``_need_hip`` looks at of a HIP tensor that is not float32 (no GPU here to make one)."""

    is_cuda, dtype = True, torch.float16


def test_training_batchnorm_on_one_value_per_channel_raises_torchs_error():
    down = wm.ConvDownBlock(3, 8).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        down(torch.zeros(1, 3, 2, 2))  # conv2's output is [1, 8, 1, 1]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        down(torch.zeros(1, 3, 1, 1))
    with pytest.raises(ValueError, match=r"got input size torch.Size\(\[1, 8, 1, 1, 1\]\)"):
        wm.ConvDownBlock(3, 8, stride=(1, 2, 2), is_3d=True).train()(torch.zeros(1, 3, 1, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):  # two values per channel, and eval mode, get as far as the device check
        down(torch.zeros(2, 3, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        down.eval()(torch.zeros(1, 3, 2, 2))
    ref = nn.Sequential(nn.Conv2d(3, 8, 3, 2, 1), nn.BatchNorm2d(8)).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ref(torch.zeros(1, 3, 2, 2))


@pytest.mark.parametrize("length", range(1, 12))
@pytest.mark.parametrize("stride", [1, 2])
def test_output_length_formula_for_both_kernel_sizes(length, stride):
    """(L - 1) // s + 1 is the length of the padded 3-tap and of the unpadded 1-tap convolution: the residual sum is shaped alike."""
    x = torch.zeros(1, 1, length)
    want = wm.conv_out_length(length, stride)
    assert want == (length - 1) // stride + 1
    assert F.conv1d(x, torch.zeros(1, 1, 3), stride=stride, padding=1).shape[-1] == want
    assert F.conv1d(x, torch.zeros(1, 1, 1), stride=stride, padding=0).shape[-1] == want
    assert wm._out_shape((2, 5, length, 7, length), 9, (1, stride, stride)) == (2, 9, length, wm.conv_out_length(7, stride), want)


@pytest.mark.parametrize("length", [1, 2, 3, 6])
def test_upsampling_weights_against_interpolate_in_float64(length):
    """Output 2 i = 0.25 x[i - 1] + 0.75 x[i], output 2 i + 1 = 0.75 x[i] + 0.25 x[i + 1], indices clamped: the matrix of
    F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) along one axis, and of the trilinear (1, 2, 2) form."""
    lo, hi = wm.UPSAMPLE_TAPS
    want = torch.zeros(2 * length, length, dtype=torch.float64)
    for i in range(length):
        want[2 * i, max(i - 1, 0)] += lo
        want[2 * i, i] += hi
        want[2 * i + 1, i] += hi
        want[2 * i + 1, min(i + 1, length - 1)] += lo
    eye = torch.eye(length, dtype=torch.float64)
    rows = F.interpolate(eye.view(length, 1, length, 1).expand(length, 1, length, 2), scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(rows[:, 0, :, 0].t(), want)  # quarters and three quarters are exact in binary
    vol = F.interpolate(eye.view(length, 1, 1, 1, length), scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    assert vol.shape == (length, 1, 1, 2, 2 * length) and torch.equal(vol[:, 0, 0, 0].t(), want)
    assert (want.sum(1) == 1).all() and (want.sum(0) == 2).all()  # a source voxel's weights over the (at most 4) outputs that read it


def test_the_library_exports_the_convnd_symbols():
    names = ["gw_convnd_workspace_bytes", "gw_convnd_forward", "gw_convnd_dgrad", "gw_convnd_wgrad", "gw_convnd_bn_stats",
             "gw_convnd_tail_forward", "gw_convnd_tail_backward", "gw_convnd_upsample2x"]
    assert all(n in _lib.EXPORTS for n in names)
    L = _lib.lib()
    assert L.gw_version() == _lib.ABI_VERSION == 19
    import ctypes

    geo = lambda *v: (ctypes.c_int32 * 12)(*v)  # noqa: E731
    # slabs of 1024 output voxels x cout x (cin taps + 1) floats: 2 x 3 x 7 x 9 output voxels of a (1, 2, 2) convolution -> 1 slab
    assert L.gw_convnd_workspace_bytes(geo(2, 4, 8, 3, 13, 18, 3, 3, 3, 1, 2, 2)) == 1 * 8 * (4 * 27 + 1) * 4
    assert L.gw_convnd_workspace_bytes(geo(2, 3, 8, 1, 64, 64, 1, 1, 1, 1, 1, 1)) == 8 * 8 * (3 + 1) * 4
    assert L.gw_convnd_workspace_bytes(geo(2, 3, 8, 1, 64, 64, 1, 2, 1, 1, 1, 1)) == 0 and b"bad arguments" in L.gw_last_error()
    assert L.gw_convnd_workspace_bytes(geo(2, 3, 8, 1, 64, 64, 1, 3, 3, 1, 3, 1)) == 0
    assert L.gw_convnd_workspace_bytes(geo(0, 3, 8, 1, 64, 64, 1, 3, 3, 1, 1, 1)) == 0
    assert L.gw_convnd_workspace_bytes(None) == 0
    assert L.gw_convnd_forward(geo(2, 3, 8, 1, 6, 6, 1, 3, 3, 1, 2, 2), 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.gw_convnd_upsample2x(1, 1, 1, 0, 2, 0, None, None, None, None, None) == -1
