"""Write tests/golden/gencast_model_{a,b}.npz and gencast_model_state_dict.json from the reference's own GenCast graph and
Denoiser files.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_gencast_model_golden.py``.
The reference's files (graph/icosahedral_mesh.py, model_utils.py, grid_mesh_connectivity.py, graph_builder.py, utils/batching.py,
utils/noise.py, the four layer files and denoiser.py) are loaded read-only by path under oracle.refload.REF_ROOT under their own
module names, with the stand-ins of tests/gencast_model_oracle.py registered for dacite, trimesh, xarray, torch_harmonics and
torch_geometric (none is installed, none is part of the reference).  The closest face of a grid point comes from the brute-force
rule of that module; the generator asserts that on both grids the gap between the tied group of closest faces and the next face
is at least 1e-5 for every grid point, so the rule, not rounding, decides every pick.

Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed): the fixtures hold graphs
(case a: all four in full; case b: counts, in-degrees and float64 column sums), seeds, meta, the grid and the outputs - no
weights and no program text.  The JSON records the ``state_dict`` key / shape tables and the constructors' signatures.
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle.refload import REF_ROOT  # noqa: E402
from tests import gencast_model_oracle as mo  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = "graph_weather.models.gencast"
FILES = ("graph.icosahedral_mesh", "graph.model_utils", "graph.grid_mesh_connectivity", "graph.graph_builder", "utils.batching",
         "utils.noise", "layers.modules", "layers.encoder", "layers.processor", "layers.decoder", "denoiser")


def _load_reference():
    stand_ins = mo.stand_in_modules()
    saved = {k: v for k, v in sys.modules.items() if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins}
    for k in saved:
        del sys.modules[k]
    sys.modules.update(stand_ins)
    for name in ("graph_weather", "graph_weather.models", BASE, BASE + ".graph", BASE + ".utils", BASE + ".layers"):
        pkg = types.ModuleType(name)  # empty packages: nothing of this repository's alias tree is imported meanwhile
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    try:
        for name in FILES:
            path = os.path.join(REF_ROOT, *(BASE + "." + name).split(".")) + ".py"
            spec = importlib.util.spec_from_file_location(BASE + "." + name, path)
            mod = importlib.util.module_from_spec(spec)
            sys.modules[BASE + "." + name] = mod
            spec.loader.exec_module(mod)
            parent, _, leaf = (BASE + "." + name).rpartition(".")
            setattr(sys.modules[parent], leaf, mod)  # (graph_builder.py imports its siblings from the package)
            mods[name] = mod
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods


def _signature(cls):
    out = []
    for name, prm in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = prm.default
        if d is inspect.Parameter.empty:
            out.append([name, "<required>"])
        else:
            out.append([name, d if isinstance(d, (bool, int, float, list, type(None))) else str(d)])
    return out


def _check_gaps(model, lon, lat, ref):
    gm = ref["graph.grid_mesh_connectivity"]
    pos = gm._grid_lat_lon_to_coordinates(lat.astype(np.float32), lon.astype(np.float32)).reshape([-1, 3])
    mesh = model.graphs._mesh
    _, _, gap = mo.closest_faces_brute(pos, mesh.vertices, mesh.faces)
    assert gap.min() >= mo.MIN_GAP, "closest-face gap %.3e below %.0e: shift the grid" % (gap.min(), mo.MIN_GAP)
    return float(gap.min())


def main():
    ref = _load_reference()
    Denoiser = ref["denoiser"].Denoiser
    tables = {}
    for name, (_, _, _, seed) in mo.CASES.items():
        kw = mo.case_kwargs(name)
        model = fill_(Denoiser(**kw), seed)
        gap = _check_gaps(model, kw["grid_lon"], kw["grid_lat"], ref)
        z, x, s = mo.case_inputs(name)
        with torch.no_grad():
            out = model(z, x, s)
        graphs = mo.graph_tables(model)
        dims = [getattr(model.graphs, k) for k in ("grid_nodes_dim", "mesh_nodes_dim", "mesh_edges_dim", "g2m_edges_dim", "m2g_edges_dim")]
        keep = dict(seed=np.int64(seed), grid_lon=np.asarray(kw["grid_lon"], dtype=np.float64), grid_lat=np.asarray(kw["grid_lat"], dtype=np.float64),
                    dims=np.array(dims, dtype=np.int64), min_gap=np.float64(gap), out=out.numpy().astype(np.float32),
                    sigma=s.numpy())
        if name == "gencast_model_a":
            keep.update({k: v.numpy() for k, v in graphs.items()})
        else:
            for k, v in graphs.items():
                if v.dtype == torch.int64:
                    n_src = graphs[{"g2m": "g2m_grid_nodes", "m2g": "m2g_mesh_nodes"}.get(k[:3], "mesh_nodes")].shape[0]
                    n_dst = graphs[{"g2m": "g2m_mesh_nodes", "m2g": "m2g_grid_nodes"}.get(k[:3], "mesh_nodes")].shape[0]
                    keep[k + "_count"] = np.int64(v.shape[1])
                    keep[k + "_indeg"] = np.bincount(v[1].numpy(), minlength=n_dst).astype(np.int32)
                    keep[k + "_outdeg"] = np.bincount(v[0].numpy(), minlength=n_src).astype(np.int32)
                else:
                    keep[k + "_shape"] = np.array(v.shape, dtype=np.int64)
                    keep[k + "_colsum"] = v.double().sum(0).numpy()
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **keep)
        tables[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        print(name, "out", tuple(out.shape), "min gap %.3e" % gap, "tensors", len(tables[name]),
              {k: tuple(v.shape) for k, v in graphs.items() if v.dtype == torch.int64})
    out = {"state_dict": tables,
           "buffers": list(mo.GRAPH_KEYS),
           "signature": {"Denoiser": _signature(Denoiser), "GraphBuilder": _signature(ref["graph.graph_builder"].GraphBuilder),
                         "Preconditioner": _signature(ref["utils.noise"].Preconditioner),
                         "DenoiserConfig": _signature(ref["denoiser"].DenoiserConfig)}}
    with open(os.path.join(GOLDEN, "gencast_model_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
