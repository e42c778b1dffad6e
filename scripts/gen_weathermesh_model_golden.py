"""Write tests/golden/weathermesh_model_*.npz and weathermesh_model_state_dict.json from the reference's own WeatherMesh classes.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_weathermesh_model_golden.py``.
The reference's ``layers.py``, ``processor.py``, ``encoder.py``, ``decoder.py`` and ``weathermesh2.py`` of
``graph_weather/models/weathermesh`` are loaded read-only by path under oracle.refload.REF_ROOT.  ``encoder.py`` imports
``graph_weather.models.weathermesh.layers`` by that name, so for the duration of the load the reference's own modules are
registered in ``sys.modules`` under their ``graph_weather.models.weathermesh.*`` names (this repository's alias package must not
answer) beside the torch-only stand-ins for ``natten`` (tests/weathermesh_oracle.py) and ``dacite``
(tests/weathermesh_model_oracle.py: the nested one); ``sys.modules`` is restored afterwards.  The convolution towers of these
fixtures are therefore the reference's real code; only the attention is the stand-in.

Weights come from tests/weathermesh_model_oracle.build_model (tests/cafa_oracle.fill_, per-key seeded, running variances made
positive; the processors, which are not in the model's ``state_dict``, from their own seeds) and inputs from
numpy.RandomState(seed).  Recorded per case: the seed, the eval outputs, the training-mode outputs and the running buffers after
that one training-mode forward.  No weights, no inputs, no program text.  The JSON records the key -> shape tables in order, the
constructors' signatures, the configs' fields and a nested config round trip.
"""
import dataclasses
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
from scripts.gen_gencast_model_golden import _signature  # noqa: E402
from tests import weathermesh_model_oracle as mo  # noqa: E402
from tests import weathermesh_oracle as wo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG = "graph_weather.models.weathermesh"
ORDER = ("layers", "processor", "encoder", "decoder", "weathermesh2")


def _load_reference() -> dict:
    stand_ins = dict(wo.natten_modules(), **mo.dacite_modules())
    for name in ("graph_weather", "graph_weather.models", PKG):  # empty shells: the parents of the modules loaded by path
        stand_ins[name] = types.ModuleType(name)
        stand_ins[name].__path__ = []
    saved = {k: v for k, v in sys.modules.items() if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins}
    for k in saved:
        del sys.modules[k]
    sys.modules.update(stand_ins)
    mods = {}
    try:
        for short in ORDER:
            name = PKG + "." + short
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, *name.split(".")) + ".py")
            mods[short] = importlib.util.module_from_spec(spec)
            sys.modules[name] = mods[short]
            spec.loader.exec_module(mods[short])
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods


def main():
    ref = _load_reference()
    WeatherMesh = ref["weathermesh2"].WeatherMesh
    tables = {}
    for name in mo.CASES:
        model = mo.build_model(WeatherMesh, name)
        surface, pressure = mo.case_inputs(name)
        with torch.no_grad():
            ev = model.eval()(surface, pressure, mo.FORECAST_STEPS)
            tr = model.train()(surface, pressure, mo.FORECAST_STEPS)
        buffers = {k: v.numpy().astype(np.float32) for k, v in model.state_dict().items() if "running_" in k}
        assert all(int(v) == 1 for k, v in model.state_dict().items() if k.endswith("num_batches_tracked"))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(mo.CASES[name][2]),
                            surface=ev.surface.numpy(), pressure=ev.pressure.numpy(), train_surface=tr.surface.numpy(),
                            train_pressure=tr.pressure.numpy(), **{"buffer/" + k: v for k, v in buffers.items()})
        tables[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert not any(k.startswith("processors") for k in tables[name]) and len(list(model.parameters())) < len(tables[name])
        print(name, "surface", tuple(ev.surface.shape), "pressure", tuple(ev.pressure.shape), "tensors", len(tables[name]))
    blocks = {"ConvDownBlock(3, 8)": ref["layers"].ConvDownBlock(3, 8),
              "ConvDownBlock(4, 8, stride=(1, 2, 2), is_3d=True)": ref["layers"].ConvDownBlock(4, 8, stride=(1, 2, 2), is_3d=True),
              "ConvUpBlock(8, 3)": ref["layers"].ConvUpBlock(8, 3), "ConvUpBlock(16, 5, is_3d=True)": ref["layers"].ConvUpBlock(16, 5, is_3d=True)}
    for key, block in blocks.items():
        tables[key] = {k: list(v.shape) for k, v in block.state_dict().items()}
    configs = {"WeatherMeshEncoderConfig": ref["encoder"].WeatherMeshEncoderConfig,
               "WeatherMeshDecoderConfig": ref["decoder"].WeatherMeshDecoderConfig, "WeatherMeshConfig": ref["weathermesh2"].WeatherMeshConfig}
    cfg = configs["WeatherMeshConfig"].from_json(mo.CONFIG_JSON)
    assert isinstance(cfg.encoder, configs["WeatherMeshEncoderConfig"]) and isinstance(cfg.processors[1], ref["processor"].WeatherMeshProcessorConfig)
    out = {"state_dict": tables,
           "signature": {"ConvDownBlock": _signature(ref["layers"].ConvDownBlock), "ConvUpBlock": _signature(ref["layers"].ConvUpBlock),
                         "WeatherMeshEncoder": _signature(ref["encoder"].WeatherMeshEncoder),
                         "WeatherMeshDecoder": _signature(ref["decoder"].WeatherMeshDecoder), "WeatherMesh": _signature(WeatherMesh)},
           "config_fields": {k: [[f.name, mo.type_name(f.type)] for f in dataclasses.fields(c)] for k, c in configs.items()},
           "output_fields": [f.name for f in dataclasses.fields(ref["weathermesh2"].WeatherMeshOutput)],
           "config_round_trip": cfg.to_json()}
    with open(os.path.join(GOLDEN, "weathermesh_model_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
