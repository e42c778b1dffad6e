"""Write tests/golden/weathermesh_processor_*.npz and weathermesh_state_dict.json from the reference's own WeatherMeshProcessor.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_weathermesh_golden.py``.  The
reference's ``graph_weather/models/weathermesh/processor.py`` is loaded read-only by path under oracle.refload.REF_ROOT under its
own module name, with the torch-only stand-ins of tests/weathermesh_oracle.py registered as ``natten`` and ``dacite`` (neither is
installed, neither is part of the reference): the reference's ``WeatherMeshProcessor`` then stacks the stand-in's
``NeighborhoodAttention3D``, whose semantics are restated from NATTEN's documentation and not pinned against NATTEN.

Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed).  Recorded per case: the seed,
the eval output and the training-mode output (the class holds no active dropout: the generator asserts the two are bitwise equal).
The fixtures hold no weights, no inputs and no program text.  The JSON records the ``state_dict`` key / shape table of every case,
the constructors' signatures and the config's fields.
"""
import dataclasses
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle.refload import REF_ROOT  # noqa: E402
from scripts.gen_gencast_model_golden import _signature  # noqa: E402
from tests import weathermesh_oracle as wo  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAME = "graph_weather.models.weathermesh.processor"


def _load_reference():
    stand_ins = dict(wo.natten_modules(), **wo.dacite_modules())
    saved = {k: sys.modules[k] for k in stand_ins if k in sys.modules}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("_reference_weathermesh_processor", os.path.join(REF_ROOT, *NAME.split(".")) + ".py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k in stand_ins:
            del sys.modules[k]
        sys.modules.update(saved)
    return mod


def main():
    ref = _load_reference()
    tables = {}
    for name, (kw, shape, seed) in wo.CASES.items():
        module = fill_(ref.WeatherMeshProcessor(**kw), seed)
        x = wo.case_input(name)
        with torch.no_grad():
            out, train = module.eval()(x), module.train()(x)
        assert torch.equal(out, train)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed), out=out.numpy().astype(np.float32),
                            train_out=train.numpy().astype(np.float32))
        tables[name] = {k: list(v.shape) for k, v in module.state_dict().items()}
        print(name, "out", tuple(out.shape), "tensors", len(tables[name]))
    cfg = ref.WeatherMeshProcessorConfig.from_json({"latent_dim": 8, "n_layers": 2, "kernel": (5, 7, 7), "num_heads": 1})
    out = {"state_dict": tables,
           "signature": {"WeatherMeshProcessor": _signature(ref.WeatherMeshProcessor),
                         "NeighborhoodAttention3D": _signature(wo.NeighborhoodAttention3D)},
           "config_fields": [[f.name, getattr(f.type, "__name__", str(f.type))] for f in dataclasses.fields(ref.WeatherMeshProcessorConfig)],
           "config_round_trip": cfg.to_json()}
    with open(os.path.join(GOLDEN, "weathermesh_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
