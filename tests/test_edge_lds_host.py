"""CPU checks of the inference form of the fp32 edge update with the constants in LDS (csrc/gw_edge_lds.hip): its ISA (no
scratch, register budget of two workgroups per CU, no register touched while a hidden load is in flight, edge_kernel's weight
ring) and its place in the product library."""
import os
import re
import subprocess
import sys

from graph_weather_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_weather_amd", "csrc")


def test_constants_in_lds_edge_kernel_isa(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # (the compiler the library itself was built with)
    src = os.path.join(CSRC, "gw_edge_lds.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Werror", "-c", src, "-o", "e.o", "-save-temps"]
    subprocess.run(cmd, check=True, cwd=tmp_path)  # (-Werror: the translation unit compiles clean)
    asm = tmp_path / "gw_edge_lds-hip-amdgcn-amd-amdhsa-gfx950.s"
    text = asm.read_text()
    kernels = re.findall(r"^(_Z\w*elds_kernel\w*):", text, re.M)
    assert len(kernels) == 3, kernels  # <true, 1>, <true, 2>, <false, 3>
    assert not re.search(r"edge_kernel|estream_kernel", text)  # other tests count those names in their own files alone
    for field, ok in ((r"\.private_segment_fixed_size:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_spill_count:\s+(\d+)", lambda v: v == 0),
                      (r"\.sgpr_spill_count:\s+(\d+)", lambda v: v == 0), (r"\.vgpr_count:\s+(\d+)", lambda v: 0 < v <= 256),
                      (r"\.group_segment_fixed_size:\s+(\d+)", lambda v: v == 0)):
        vals = [int(x) for x in re.findall(field, text)]
        assert len(vals) == 3 and all(ok(v) for v in vals), (field, vals)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_audit.py"), str(asm), "elds_kernel"],
                         capture_output=True, text=True, check=True).stdout
    counts = [int(x) for x in re.findall(r"hidden-load register hazards: (\d+)", out)]
    assert counts == [0, 0, 0], out
    # the weight ring is edge_kernel's: 8 DMA pieces per wave and chunk, chunks of 8 K-steps x 16 MFMAs; 24 chunks per tile
    # with a raw layer-1 pass, 16 without.  And no vector-memory instruction fetches a constant: what is left per wave and tile
    # is 2 indices + 5 constant floats (once, to LDS), [the raw row,] the ring and the residual row, as 16-byte loads.
    for k in kernels:
        raw, nproj = re.search(r"elds_kernelILb([01])ELi(\d)E", k).groups()
        chunks = 24 if raw == "1" else 16
        body = text[text.index(k + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert len(re.findall(r"global_load_lds_dwordx4", body)) == chunks * 8
        assert len(re.findall(r"v_mfma_f32_16x16x4_f32|v_mfma_f32_16x16x4f32", body)) == chunks * 128
        assert len(re.findall(r"global_load_dword\s", body)) == 7
        assert len(re.findall(r"global_load_dwordx4\s", body)) == (16 if raw == "1" else 0) + 16 * int(nproj) + 16


def test_product_library_holds_the_kernel_and_adds_no_export():
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T " in ln and ln.split()[-1].startswith("gw_")}
    assert exported == set(_lib.EXPORTS)
    raw = open(_lib.LIB_PATH, "rb").read()
    assert b"elds_kernel" in raw
