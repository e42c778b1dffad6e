"""Write tests/golden/aurora_*.npz and aurora_state_dict.json from the reference's own Aurora classes.

Run from the repository root, on the CPU, with the reference tree and einops present: ``python scripts/gen_aurora_golden.py``.
The reference's ``graph_weather/models/aurora`` files are loaded read-only by path under oracle.refload.REF_ROOT as a synthetic
package (its ``__init__`` imports them relatively).  Weights come from tests/aurora_oracle.fill_ (per-key seeded) and inputs
from numpy.RandomState(seed): the fixtures hold the seed, the meta and the output - no weights, no inputs.
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

from tests import aurora_oracle as ao  # noqa: E402
from oracle.refload import REF_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG = "_reference_aurora"


def _load_reference():
    base = os.path.join(REF_ROOT, "graph_weather", "models", "aurora")
    pkg = types.ModuleType(PKG)
    pkg.__path__ = [base]
    sys.modules[PKG] = pkg
    for name in ("decoder", "encoder", "model", "processor"):
        spec = importlib.util.spec_from_file_location(PKG + "." + name, os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[PKG + "." + name] = mod
        spec.loader.exec_module(mod)
        for attr in ("AuroraModel", "EarthSystemLoss", "Swin3DEncoder", "Decoder3D", "PerceiverProcessor", "ProcessorConfig"):
            if hasattr(mod, attr):
                setattr(pkg, attr, getattr(mod, attr))
    return pkg


def meta_of(name):
    """The integers that pin a case: every integer of its configuration and of its input description, in order."""
    _, cfg, spec, _ = ao.CASES[name]
    out = []
    for d in (cfg, spec):
        for v in d.values():
            for x in (v if isinstance(v, tuple) else (v,)):
                if isinstance(x, (bool, int)):
                    out.append(int(x))
    return out


def main():
    ref = _load_reference()
    tables = {}
    for name, (kind, cfg, _, seed) in ao.CASES.items():
        module = ao.build(ref, name)
        inputs = ao.case_inputs(name)
        with torch.no_grad():
            if kind == "model":
                out = module(inputs["points"], inputs["features"], inputs.get("mask"))
            elif kind == "loss":
                res = module(inputs["pred"], inputs["target"], inputs["points"])
                out = torch.stack([res[k] for k in ao.LOSS_KEYS])
            elif kind == "perceiver":
                out = module(inputs["x"], inputs.get("attention_mask"))
            else:
                out = module(inputs["x"])
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed), meta=np.array(meta_of(name), dtype=np.int64),
                            out=out.numpy().astype(np.float32))
        if kind != "loss":
            tables[type(module).__name__ + ":" + name] = module
    tables["AuroraModel"] = ref.AuroraModel(3, 2, latent_dim=32, num_layers=2)
    tables["Swin3DEncoder"] = ref.Swin3DEncoder()
    tables["PerceiverProcessor"] = ref.PerceiverProcessor(ref.ProcessorConfig(input_dim=16, latent_dim=24, d_model=16,
                                                                              num_self_attention_layers=1, num_attention_heads=2))
    tables["Decoder3D"] = ref.Decoder3D()
    out = {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()}
    with open(os.path.join(GOLDEN, "aurora_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
