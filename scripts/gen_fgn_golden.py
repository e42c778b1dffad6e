"""Write tests/golden/fgn_model_{a,b,c}.npz and fgn_state_dict.json from the reference's own FGN files.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_fgn_golden.py``.  The reference's
files - the GenCast graph, batching and layer files that scripts/gen_gencast_model_golden.py loads, then fgn/layers/processor.py
and fgn/model.py - are loaded read-only by path under oracle.refload.REF_ROOT under their own module names, with the stand-ins
of tests/gencast_model_oracle.py registered for the packages that are not installed.  The grids are those of
tests/gencast_model_oracle.py; the generator asserts their closest-face gaps as that generator does.

Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed).  The reference draws its noise
vectors inside ``forward``; they are recorded by seeding ``torch.manual_seed(s)`` before the forward, then re-seeding and
re-drawing the N x (B, noise_dimension) vectors (tests/fgn_oracle.draw_noise) - the generator asserts that the reference's own
stages on the re-drawn vectors reproduce its forward bit for bit.  The fixtures hold seeds, meta, the noise vectors and the
outputs - no weights and no program text.  Case c (B = 1) records the reference's ``forward`` output, which holds member 0 only,
and both members computed through the reference's own ``_run_encoder`` / ``_run_processor`` / ``_run_decoder``.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle.refload import REF_ROOT  # noqa: E402
from scripts.gen_gencast_model_golden import _check_gaps, _signature  # noqa: E402
from tests import fgn_oracle as fo  # noqa: E402
from tests import gencast_model_oracle as mo  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = "graph_weather.models"
FILES = ("gencast.graph.icosahedral_mesh", "gencast.graph.model_utils", "gencast.graph.grid_mesh_connectivity", "gencast.graph.graph_builder",
         "gencast.utils.batching", "gencast.layers.modules", "gencast.layers.encoder", "gencast.layers.decoder", "fgn.layers.processor",
         "fgn.model")
PACKAGES = ("graph_weather", MODELS, MODELS + ".gencast", MODELS + ".gencast.graph", MODELS + ".gencast.utils", MODELS + ".gencast.layers",
            MODELS + ".fgn", MODELS + ".fgn.layers")


def _load_reference():
    stand_ins = mo.stand_in_modules()
    saved = {k: v for k, v in sys.modules.items() if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins}
    for k in saved:
        del sys.modules[k]
    sys.modules.update(stand_ins)
    for name in PACKAGES:
        pkg = types.ModuleType(name)  # empty packages: nothing of this repository's alias tree is imported meanwhile
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    try:
        for name in FILES:
            full = MODELS + "." + name
            spec = importlib.util.spec_from_file_location(full, os.path.join(REF_ROOT, *full.split(".")) + ".py")
            mod = importlib.util.module_from_spec(spec)
            sys.modules[full] = mod
            spec.loader.exec_module(mod)
            parent, _, leaf = full.rpartition(".")
            setattr(sys.modules[parent], leaf, mod)
            mods[name] = mod
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods


def _members_by_stages(model, x, noise):
    """[B, N, lon, lat, out] through the reference's own stage methods, member by member, on the given noise vectors."""
    flat = x.reshape(x.shape[0], -1, x.shape[-1])
    outs = []
    for n in range(noise.shape[1]):
        latent_grid, latent_mesh = model._run_encoder(flat)
        latent_mesh = model._run_processor(latent_mesh, noise_vectors=noise[:, n])
        out = model._run_decoder(latent_mesh, latent_grid)
        outs.append(out.reshape(x.shape[0], model.num_lon, model.num_lat, -1))
    return torch.stack(outs, dim=1)


def main():
    ref = _load_reference()
    FGN = ref["fgn.model"].FunctionalGenerativeNetwork
    shim = {"graph.grid_mesh_connectivity": ref["gencast.graph.grid_mesh_connectivity"]}
    tables = {}
    for name, (grid, ckw, B, N, seed) in fo.CASES.items():
        kw = fo.case_kwargs(name)
        model = fill_(FGN(**kw), seed)
        gap = _check_gaps(model, kw["grid_lon"], kw["grid_lat"], shim)
        x = fo.case_input(name)
        tseed = fo.TORCH_SEED + seed
        torch.manual_seed(tseed)
        with torch.no_grad():
            out = model(x, num_ensemble=N)
        noise = fo.draw_noise(tseed, B, N, ckw["noise_dimension"])
        with torch.no_grad():
            members = _members_by_stages(model, x, noise)
        if B > 1:
            assert out.shape == members.shape and torch.equal(out, members), name  # the re-drawn vectors are the forward's
        else:
            assert tuple(out.shape) == (1, 1) + tuple(members.shape[2:]) and torch.equal(out[:, 0], members[:, 0]), name
        meta = [ckw["input_features_dim"], ckw["output_features_dim"], ckw["noise_dimension"], *ckw["hidden_dims"], ckw["num_blocks"],
                ckw["num_heads"], ckw["splits"], ckw["num_hops"], int(ckw.get("use_edges_features", True)), B, N]
        keep = dict(seed=np.int64(seed), torch_seed=np.int64(tseed), meta=np.array(meta, dtype=np.int64), min_gap=np.float64(gap),
                    scale_factor=np.float64(ckw.get("scale_factor", 1.0)), noise=noise.numpy(), out=out.numpy().astype(np.float32),
                    members=members.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **keep)
        tables[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        print(name, "forward", tuple(out.shape), "members", tuple(members.shape), "min gap %.3e" % gap, "tensors", len(tables[name]))
    out = {"state_dict": tables, "buffers": list(mo.GRAPH_KEYS),
           "signature": {"FunctionalGenerativeNetwork": _signature(FGN), "Processor": _signature(ref["fgn.layers.processor"].Processor),
                         "FunctionalGenerativeNetworkConfig": _signature(ref["fgn.model"].FunctionalGenerativeNetworkConfig)}}
    with open(os.path.join(GOLDEN, "fgn_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
