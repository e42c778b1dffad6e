"""ThermalizerLayer without a GPU: alias import, state_dict tables, grid inference, argument errors, the fp64 restatement
against the golden fixtures written from the reference, and the ISA of csrc/gw_thermal.hip."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import thermal_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_alias_import():
    import importlib.util

    import graph_weather_amd as gw

    # loaded from its file: another test may have put the reference's module under the same name in sys.modules
    path = os.path.join(ROOT, "graph_weather", "models", "layers", "thermalizer.py")
    spec = importlib.util.spec_from_file_location("_alias_thermalizer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.ThermalizerLayer is gw.ThermalizerLayer and mod.AdaptiveUNet is gw.AdaptiveUNet


def test_grid_inference_matches_reference_fixture():
    """Against the reference's own _infer_grid_dimensions (pinned in thermalizer_grid.json by scripts/gen_thermalizer_golden.py)."""
    from graph_weather_amd.thermalizer import infer_grid_dimensions

    with open(os.path.join(GOLDEN, "thermalizer_grid.json")) as f:
        pinned = json.load(f)
    assert len(pinned) > 2000
    for n, h, w in pinned:
        assert infer_grid_dimensions(n) == (h, w), n
    want = {5882: (1, 5882), 11764: (1, 11764), 29410: (170, 173), 117640: (340, 346), 123522: (346, 357)}
    for n, hw in want.items():
        assert infer_grid_dimensions(n) == hw


@pytest.mark.reference
def test_grid_inference_matches_reference_sweep():
    from oracle import refload

    from graph_weather_amd.thermalizer import infer_grid_dimensions

    if not refload.reference_available():
        pytest.skip("reference tree not present")
    refload.load_reference()
    ref = sys.modules["graph_weather.models.layers.thermalizer"].ThermalizerLayer(3)._infer_grid_dimensions
    for n in range(1, 300001):
        assert infer_grid_dimensions(n) == ref(n), n


def test_attributes_and_schedule():
    import graph_weather_amd as gw

    layer = gw.ThermalizerLayer(32, timesteps=1000)
    assert layer.timesteps == 1000 and layer.score_model.in_channels == 34 and layer.score_model.out_channels == 32
    assert layer.betas.dtype == torch.float64 and layer.betas.min() >= 0 and layer.betas.max() <= 0.999
    assert torch.equal(layer.alphas_cumprod, to.alphas_cumprod())
    assert not any(k in ("betas", "alphas", "alphas_cumprod") for k in layer.state_dict())


def test_state_dict_tables():
    import graph_weather_amd as gw
    from graph_weather_amd.utils import regular_lat_lons

    with open(os.path.join(GOLDEN, "thermalizer_state_dict.json")) as f:
        tables = json.load(f)
    mods = {"ThermalizerLayer(256)": gw.ThermalizerLayer(256), "ThermalizerLayer(32)": gw.ThermalizerLayer(32),
            "GraphWeatherForecaster(30deg, use_thermalizer=True)": gw.GraphWeatherForecaster(regular_lat_lons(30.0),
                                                                                             use_thermalizer=True)}
    for name, m in mods.items():
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == tables[name], name
        m.load_state_dict({k: torch.zeros(v) for k, v in tables[name].items()}, strict=True)


def test_group_norm_width_error_like_reference():
    import graph_weather_amd as gw

    with pytest.raises(ValueError):  # GroupNorm(8, 78) in upconv1, as in the reference
        gw.ThermalizerLayer(78)


def test_processor_and_forecaster_construct():
    import graph_weather_amd as gw
    from graph_weather_amd.utils import regular_lat_lons

    p = gw.Processor(input_dim=32, edge_dim=32, num_blocks=1, use_thermalizer=True)
    assert p.thermalizer.score_model.in_channels == 34
    cfg = gw.GraphWeatherForecasterConfig(lat_lons=regular_lat_lons(30.0), use_thermalizer=True)
    assert cfg.build().processor.thermalizer.score_model.out_channels == 256


def test_argument_errors():
    import graph_weather_amd as gw

    layer = gw.ThermalizerLayer(8)
    x = torch.zeros(12, 8)
    with pytest.raises(ValueError):
        layer(x, 5, height=5, width=5)
    with pytest.raises(TypeError):
        layer(x, 5.0, height=3, width=4)
    with pytest.warns(UserWarning):
        with pytest.raises(RuntimeError):  # inference passes; the CPU tensor is refused (there is no CPU path)
            layer(x, 5)
    with pytest.raises(RuntimeError):
        layer(x, 5, height=3, width=4)


@pytest.mark.parametrize("path", sorted(p for p in os.listdir(GOLDEN) if p.startswith("thermalizer_") and p.endswith(".npz")))
def test_oracle_matches_reference_fixtures(path):
    import graph_weather_amd as gw

    z = np.load(os.path.join(GOLDEN, path))
    B, H, W, F, t, seed = (int(v) for v in z["meta"])
    layer = to.fill_(gw.ThermalizerLayer(F), seed)
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((B * H * W, F)).astype(np.float32))
    noise = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((B, F, H, W)).astype(np.float32))
    noise_rows = noise.permute(0, 2, 3, 1).reshape(B * H * W, F)
    sd = {k: v.double() for k, v in to.strip(layer.state_dict(), "score_model.").items()}
    y = to.thermalize(sd, x.double(), noise_rows, t, B, H, W)
    ref = torch.from_numpy(z["out"]).double()
    assert (y - ref).abs().max().item() <= 1e-4 * max(ref.abs().max().item(), 1.0)


def test_isa_of_thermal_kernels(tmp_path):
    src = os.path.join(ROOT, "graph_weather_amd", "csrc", "gw_thermal.hip")
    out = tmp_path / "gw_thermal.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o",
                    str(out)], check=True)
    asm = out.read_text()
    bodies = re.split(r"\n(?=\S+:\s*; @)", asm)
    gemm = [b for b in bodies if re.match(r"_ZN[^:]*conv_(nt|tn)_kernel", b)]
    assert len(gemm) >= 9
    for b in gemm:
        assert "v_mfma_f32_16x16x4_f32" in b or "v_mfma_f32_16x16x4f32" in b
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", asm):
        assert int(m.group(1)) == 0


@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 13, 9), (2, 12, 12)])
def test_per_operation_oracle_composes_to_score_and_thermalize(B, H, W):
    """The per-operation row helpers of thermal_oracle.py (what tests/test_gpu_thermal_kernels.py holds each kernel against),
    composed into simple_net / the UNet and into the diffusion step, are ``score`` and ``thermalize`` (pinned to the reference's
    fixtures above) to fp64 rounding."""
    import graph_weather_amd as gw

    F = 6
    layer = to.fill_(gw.ThermalizerLayer(F), 5)
    sd = {k: v.double() for k, v in to.strip(layer.state_dict(), "score_model.").items()}
    g = torch.Generator().manual_seed(100 * B + 10 * H + W)
    x = torch.randn(B * H * W, F + 2, generator=g, dtype=torch.float64)
    noise = torch.randn(B * H * W, F, generator=g, dtype=torch.float64)
    ref = to.score(sd, to.to_image(x, B, H, W))
    got = to.to_image(to.score_rows(sd, x, B, H, W), B, H, W)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    for t in (0, 500, 999):
        ref = to.thermalize(sd, x[:, :F], noise, t, B, H, W)
        got = to.thermalize_rows(sd, x[:, :F], noise, t, B, H, W)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), t
    # the pieces the two nets do not use: pooling indices, the gradient-side row operations and the column sum
    y, idx = to.max_pool_rows(x, B, H, W)
    img = x.reshape(B, H * W, F + 2)
    assert torch.equal(torch.gather(img, 1, idx.reshape(B, -1, F + 2)).reshape(y.shape), y)
    assert torch.equal(to.rows_scale(x, 0.5), 0.5 * x) and torch.equal(to.rows_axpy(x, x, 2.0), 3.0 * x)
    assert (to.colsum_rows(x) - x.t().sum(1)).abs().max().item() <= 1e-12 * x.abs().sum(0).max().item()
    mean, rstd, scale, shift = to.group_norm_stats(x, torch.ones(F + 2, dtype=x.dtype), torch.zeros(F + 2, dtype=x.dtype), B, 2)
    z = to.group_norm_rows(x, torch.ones(F + 2, dtype=x.dtype), torch.zeros(F + 2, dtype=x.dtype), B, 2)
    assert (to.affine_relu_rows(x, scale, shift, B) - torch.relu(z)).abs().max().item() <= 1e-12
