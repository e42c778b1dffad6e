"""CPU checks of the decoder form of the fp32 edge update (csrc/gw_edge_stream.hip): its ISA (no scratch, register budget of
two workgroups per CU, no register touched while a hidden load is in flight) and the route that selects it."""
import os
import re
import subprocess
import sys

import pytest
import torch

from graph_weather_amd import _lib, routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_weather_amd", "csrc")

def test_no_residual_edge_kernel_isa(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(CSRC, "gw_edge_stream.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Werror", "-c", src, "-o", "e.o", "-save-temps"]
    subprocess.run(cmd, check=True, cwd=tmp_path)  # (-Werror: the translation unit compiles clean)
    asm = tmp_path / "gw_edge_stream-hip-amdgcn-amd-amdhsa-gfx950.s"
    text = asm.read_text()
    kernels = re.findall(r"^(_Z\w*estream_kernel\w*):", text, re.M)
    assert len(kernels) == 2, kernels  # one and two projected operands
    assert not re.search(r"edge_kernel", text)  # tests/test_isa_audit.py counts that name in gw_edge.hip alone
    for field, ok in ((r"\.private_segment_fixed_size:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_spill_count:\s+(\d+)", lambda v: v == 0),
                      (r"\.sgpr_spill_count:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_count:\s+(\d+)", lambda v: 0 < v <= 256),
                      (r"\.group_segment_fixed_size:\s+(\d+)", lambda v: v == 0)):
        vals = [int(x) for x in re.findall(field, text)]
        assert len(vals) == 2 and all(ok(v) for v in vals), (field, vals)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_audit.py"), str(asm), "estream_kernel"],
                         capture_output=True, text=True, check=True).stdout
    counts = [int(x) for x in re.findall(r"hidden-load register hazards: (\d+)", out)]
    assert counts == [0, 0], out
    # the weight ring is edge_kernel's: 8 DMA pieces per wave and chunk, 16 chunks of 8 K-steps x 16 MFMAs per tile
    for k in kernels:
        body = text[text.index(k + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert len(re.findall(r"global_load_lds_dwordx4", body)) == 16 * 8  # 16 chunks
        assert len(re.findall(r"v_mfma_f32_16x16x4_f32|v_mfma_f32_16x16x4f32", body)) == 16 * 16 * 8


def test_product_library_holds_the_kernel_and_adds_no_export():
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T " in ln and ln.split()[-1].startswith("gw_")}
    assert exported == set(_lib.EXPORTS)
    raw = open(_lib.LIB_PATH, "rb").read()
    assert b"estream_kernel" in raw


F32, BF16 = torch.float32, torch.bfloat16


def test_decoder_route():
    form = routes.MlpForm(F32, 1, 0, True)
    assert routes.decoder_stream(form, F32, 1000, False, False, False, True)
    assert not routes.decoder_stream(form, F32, 1000, False, False, False, False)  # the switch (ops.EDGE_STREAM)
    assert not routes.decoder_stream(form, F32, 1000, True, False, False, True)
    assert not routes.decoder_stream(form, F32, 1000, False, True, False, True)    # training keeps the per-edge residual
    assert not routes.decoder_stream(form, F32, 1000, False, False, True, True)    # ... and so does deterministic mode
    assert not routes.decoder_stream(form, F32, 0, False, False, False, True)
    assert not routes.decoder_stream(form, routes.BF16X3, 1000, False, False, False, True)
    assert not routes.decoder_stream(routes.MlpForm(F32, 2, 0, True), F32, 1000, False, False, False, True)
    assert not routes.decoder_stream(routes.MlpForm(F32, 1, 128, True), F32, 1000, False, False, False, True)
    assert not routes.decoder_stream(routes.MlpForm(F32, 1, 0, False), F32, 1000, False, False, False, True)
    assert not routes.decoder_stream(routes.MlpForm(BF16, 1, 0, True), BF16, 1000, False, False, False, True)


def test_decoder_takes_the_route_by_shape_alone_and_follows_the_switch():
    """Host only: asking for the route packs no weights (the module lives on the CPU here)."""
    import graph_weather_amd as gw
    from graph_weather_amd import ops
    from graph_weather_amd.utils import regular_lat_lons

    model = gw.GraphWeatherForecaster(regular_lat_lons(30.0)).eval()
    dec = model.decoder
    with torch.no_grad():
        assert dec.stream_path()
        try:
            ops.EDGE_STREAM = False
            assert not dec.stream_path()
        finally:
            ops.EDGE_STREAM = True
        model.set_deterministic(True)
        assert not dec.stream_path()
        model.set_deterministic(False)
        model.set_compute_dtype(ops.BF16X3)
        assert not dec.stream_path()
    model.set_compute_dtype(torch.float32)
    assert not dec.stream_path()  # grad mode with trainable parameters: the differentiable path keeps the residual
