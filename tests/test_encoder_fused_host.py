"""CPU checks of the fp32 encoder stage in one launch (csrc/gw_encoder_fused.hip): its ISA (no scratch, register budget of two
workgroups per CU, no register touched while a hidden load is in flight, the chunk schedule of its weight ring), its place in the
product library and the route that selects it."""
import os
import re
import subprocess
import sys

import torch

from graph_weather_amd import _lib, routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_weather_amd", "csrc")


def test_fused_encoder_kernel_isa(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # (the compiler the library itself was built with)
    src = os.path.join(CSRC, "gw_encoder_fused.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Werror", "-c", src, "-o", "e.o", "-save-temps"]
    subprocess.run(cmd, check=True, cwd=tmp_path)  # (-Werror: the translation unit compiles clean)
    asm = tmp_path / "gw_encoder_fused-hip-amdgcn-amd-amdhsa-gfx950.s"
    text = asm.read_text()
    kernels = re.findall(r"^(_Z\w*encfused_kernel\w*):", text, re.M)
    assert len(kernels) == 4, kernels  # <RES, NPROJ> = <true | false, 1 | 2>
    assert not re.search(r"edge_kernel|estream_kernel|elds_kernel|chain_kernel", text)  # other tests count those names in their own files
    for field, ok in ((r"\.private_segment_fixed_size:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_spill_count:\s+(\d+)", lambda v: v == 0),
                      (r"\.sgpr_spill_count:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_count:\s+(\d+)", lambda v: 0 < v <= 256),
                      (r"\.group_segment_fixed_size:\s+(\d+)", lambda v: v == 0)):
        vals = [int(x) for x in re.findall(field, text)]
        assert len(vals) == 4 and all(ok(v) for v in vals), (field, vals)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_audit.py"), str(asm), "encfused_kernel"],
                         capture_output=True, text=True, check=True).stdout
    counts = [int(x) for x in re.findall(r"hidden-load register hazards: (\d+)", out)]
    assert counts == [0, 0, 0, 0], out
    # Chunk schedule of a tile: the node encoder's first layer in 28 K-steps = three chunks of 8 (8 DMA pieces per wave) and one
    # of 4 (4 pieces), then five 256 x 256 matrices of 8 chunks each; 16 MFMAs per K-step.  Vector-memory instructions left per
    # wave and tile: 2 indices + 10 constant floats (once, to LDS), the feature row (14 pairs, or 28 floats at odd addresses),
    # the ring of projected slices and - RES only - the residual row, as 16-byte loads.  No constant is fetched twice.
    for k in kernels:
        res, nproj = re.search(r"encfused_kernelILb([01])ELi(\d)E", k).groups()
        body = text[text.index(k + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert len(re.findall(r"global_load_lds_dwordx4", body)) == 3 * 8 + 4 + 40 * 8
        assert len(re.findall(r"v_mfma_f32_16x16x4_f32|v_mfma_f32_16x16x4f32", body)) == (28 + 5 * 64) * 16
        assert len(re.findall(r"global_load_dword\s", body)) == 2 + 10 + 28
        assert len(re.findall(r"global_load_dwordx2\s", body)) == 14
        assert len(re.findall(r"global_load_dwordx4\s", body)) == 16 * int(nproj) + (16 if res == "1" else 0)
        assert len(re.findall(r"global_store_dwordx[234]", body)) == 0  # no row table is written: the aggregate leaves float by float
    assert "77056" in open(src).read()  # the LDS budget the static_assert pins: 66 560 + 256 + 10 240 B, two workgroups per CU


def test_product_library_holds_the_kernel_and_the_one_new_export():
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T " in ln and ln.split()[-1].startswith("gw_")}
    assert exported == set(_lib.EXPORTS)
    assert "gw_encoder_fused_forward" in exported
    raw = open(_lib.LIB_PATH, "rb").read()
    assert b"encfused_kernel" in raw
    assert _lib.lib().gw_version() == 19  # the export was added the way the Aurora exports were: no version bump


F32, BF16 = torch.float32, torch.bfloat16


def test_encoder_route():
    form = routes.MlpForm(F32, 1, 0, True)

    def route(ne=form, k=102, edge=form, node=F32, n_edges=648, grid=648, wide=False, autograd=False, det=False, enabled=True):
        return routes.encoder_fused(ne, k, edge, node, n_edges, grid, wide, autograd, det, enabled)

    assert route()
    assert not route(enabled=False)       # the switch (ops.ENCODER_FUSED)
    assert not route(wide=True)
    assert not route(autograd=True)       # training keeps the two launches
    assert not route(det=True)            # ... and so does deterministic mode
    assert not route(n_edges=0, grid=0)
    assert not route(n_edges=649)         # not one edge per grid node: a grid row would be encoded more than once
    assert route(k=17) and route(k=112)
    assert not route(k=16) and not route(k=113) and not route(k=256)  # first layers that are not packed in 28 K-steps
    assert not route(node=routes.BF16X3)
    for bad in (routes.MlpForm(F32, 2, 0, True), routes.MlpForm(F32, 1, 128, True), routes.MlpForm(F32, 1, 0, False),
                routes.MlpForm(BF16, 1, 0, True), routes.MlpForm(routes.BF16X3, 1, 0, True)):
        assert not route(ne=bad)
        assert not route(edge=bad)


def test_encoder_takes_the_route_by_shape_alone_and_follows_the_switch():
    """Host only: asking for the route packs no weights (the module lives on the CPU here)."""
    import graph_weather_amd as gw
    from graph_weather_amd import ops
    from graph_weather_amd.utils import regular_lat_lons

    model = gw.GraphWeatherForecaster(regular_lat_lons(30.0)).eval()
    enc = model.encoder
    with torch.no_grad():
        assert enc.fused_path()
        try:
            ops.ENCODER_FUSED = False
            assert not enc.fused_path()
        finally:
            ops.ENCODER_FUSED = True
        model.set_deterministic(True)
        assert not enc.fused_path()
        model.set_deterministic(False)
        model.set_compute_dtype(ops.BF16X3)
        assert not enc.fused_path()
    model.set_compute_dtype(torch.float32)
    assert not enc.fused_path()  # grad mode with trainable parameters: the differentiable path keeps the two launches
    narrow = gw.Encoder(regular_lat_lons(30.0), input_dim=8)  # 8 features: a first layer packed in 4 K-steps
    with torch.no_grad():
        assert not narrow.eval().fused_path()


def test_first_pass_of_a_recomputed_training_segment_keeps_the_two_launches():
    """Hierarchical checkpointing runs a segment's forward with grad mode off and takes the gradients from a replay on the
    training kernels: the first pass must give the replay's bits, so it does not take the fused route either."""
    import graph_weather_amd as gw
    from graph_weather_amd import autograd as ag
    from graph_weather_amd.utils import regular_lat_lons

    enc = gw.GraphWeatherForecaster(regular_lat_lons(30.0)).train().encoder
    seen = []

    def segment(x):
        seen.append((torch.is_grad_enabled(), enc.fused_path()))
        return (x * 2.0,)

    x = torch.ones(3, requires_grad=True)
    (y,) = ag.recompute(segment, (x,), enc)
    y.sum().backward()
    assert seen == [(False, False), (True, False)]
    assert not ag.in_recomputed_first_pass()
    with torch.no_grad():
        assert enc.fused_path()  # plain inference of the same module
