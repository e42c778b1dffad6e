"""Write tests/golden/genda_model_{a,b,c}.npz and genda_state_dict.json from the reference's own GenDA file.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_genda_golden.py``.  The reference's
files - the GenCast graph, batching, noise and layer files that scripts/gen_gencast_model_golden.py loads, then genda/model.py - are
loaded read-only by path under oracle.refload.REF_ROOT under their own module names, with the stand-ins of
tests/gencast_model_oracle.py registered for the packages that are not installed.  The grids are those of
tests/gencast_model_oracle.py; the generator asserts their closest-face gaps as that generator does.

Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed) (tests/genda_oracle.case_inputs:
the sensor mask is Bernoulli(0.3), the values are mask * normal).  Recorded per case: seeds, meta, mask and values, the reference's
eval ``forward`` and - for the cases built with conditioning - its ``guided_forward(gamma=2.0)``; for case a also its TRAINING-mode
``forward`` under the first ``torch.manual_seed`` whose host draw ``torch.rand(1)`` falls below 0.1 (the conditioning dropout
hits; the model has no other randomness), with that seed and the first seed that does not hit.  The fixtures hold no weights and no
program text.  The JSON records the ``state_dict`` key / shape tables, the buffer names and the constructors' signatures.
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
from tests import genda_oracle as do  # noqa: E402
from tests import gencast_model_oracle as mo  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = "graph_weather.models"
FILES = ("gencast.graph.icosahedral_mesh", "gencast.graph.model_utils", "gencast.graph.grid_mesh_connectivity", "gencast.graph.graph_builder",
         "gencast.utils.batching", "gencast.utils.noise", "gencast.layers.modules", "gencast.layers.encoder", "gencast.layers.processor",
         "gencast.layers.decoder", "genda.model")
PACKAGES = ("graph_weather", MODELS, MODELS + ".gencast", MODELS + ".gencast.graph", MODELS + ".gencast.utils", MODELS + ".gencast.layers",
            MODELS + ".genda")


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


def _first_seed(hit: bool) -> int:
    """The first ``torch.manual_seed`` (from 0) whose first host draw is (``hit``) or is not below the dropout probability."""
    for s in range(1000):
        torch.manual_seed(s)
        if (torch.rand(1).item() < 0.1) == hit:
            return s
    raise AssertionError("no seed found")


def main():
    ref = _load_reference()
    GenDA = ref["genda.model"].GenDA
    shim = {"graph.grid_mesh_connectivity": ref["gencast.graph.grid_mesh_connectivity"]}
    tables = {}
    for name, (grid, ckw, B, sigma, seed) in do.CASES.items():
        kw = do.case_kwargs(name)
        model = fill_(GenDA(**kw), seed).eval()
        gap = _check_gaps(model, kw["grid_lon"], kw["grid_lat"], shim)
        z, x, s, mask, values = do.case_inputs(name)
        sensors = dict(sensor_mask=mask, sensor_values=values) if do.conditioned(name) else {}
        with torch.no_grad():
            out = model(z, x, s, **sensors)
        meta = [ckw["input_features_dim"], ckw["output_features_dim"], *ckw["hidden_dims"], ckw["num_blocks"], ckw["num_heads"],
                ckw["splits"], ckw["num_hops"], int(ckw.get("use_edges_features", True)), ckw.get("conditioning_dim", 2), B]
        keep = dict(seed=np.int64(seed), meta=np.array(meta, dtype=np.int64), min_gap=np.float64(gap),
                    scale_factor=np.float64(ckw.get("scale_factor", 1.0)), sigma=s.numpy(), mask=mask.numpy(), values=values.numpy(),
                    out=out.numpy().astype(np.float32))
        if sensors:
            with torch.no_grad():
                keep["guided"] = model.guided_forward(z, x, s, mask, values, gamma=do.GAMMA).numpy().astype(np.float32)
            keep["gamma"] = np.float64(do.GAMMA)
        if name == "genda_model_a":
            hit, miss = _first_seed(True), _first_seed(False)
            model.train()
            outs = {}
            for label, ts in (("hit", hit), ("miss", miss)):
                torch.manual_seed(ts)
                with torch.no_grad():
                    outs[label] = model(z, x, s, **sensors)
            model.eval()
            assert torch.equal(outs["miss"], out)  # no other randomness: without a hit, training mode is the eval forward
            assert (outs["hit"] - out).abs().max().item() > 1e-3  # the dropped conditioning changes the result
            keep.update(train_seed=np.int64(hit), train_miss_seed=np.int64(miss), train_out=outs["hit"].numpy().astype(np.float32))
            # unscaled complex coefficient draws for a 5-step Sampler run at B = 1 (the initial state and one per step), as
            # tests/golden/gencast_sampler_b.npz holds them: [draw, out, lmax, lmax + 1, (re, im)]
            lmax = model.num_lat - 1
            draws = torch.randn(5, ckw["output_features_dim"], lmax, lmax + 1, dtype=torch.complex64,
                                generator=torch.Generator().manual_seed(do.SAMPLER_DRAW_SEED))
            keep["sampler_draws"] = torch.view_as_real(draws).numpy()
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **keep)
        tables[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        print(name, "forward", tuple(out.shape), "guided" if sensors else "no conditioning", "min gap %.3e" % gap, "tensors", len(tables[name]),
              "encoder.grid_mlp.linears.0.weight", tables[name]["encoder.grid_mlp.linears.0.weight"])
    out = {"state_dict": tables, "buffers": list(mo.GRAPH_KEYS),
           "signature": {"GenDA": _signature(GenDA), "GenDAConfig": _signature(ref["genda.model"].GenDAConfig)}}
    with open(os.path.join(GOLDEN, "genda_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
