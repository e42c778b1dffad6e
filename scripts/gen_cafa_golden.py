"""Write tests/golden/cafa_*.npz and cafa_state_dict.json from the reference's own CaFA classes.

Run from the repository root, on the CPU, with the reference tree and einops present: ``python scripts/gen_cafa_golden.py``.
The reference's ``graph_weather/models/cafa`` files are loaded read-only by path under oracle.refload.REF_ROOT as a synthetic
package (they import each other relatively).  Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from
numpy.RandomState(seed): the fixtures hold the seed, the meta and the output - no weights, no inputs.
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

from tests import cafa_oracle as co  # noqa: E402
from oracle.refload import REF_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG = "_reference_cafa"


def _load_reference():
    base = os.path.join(REF_ROOT, "graph_weather", "models", "cafa")
    pkg = types.ModuleType(PKG)
    pkg.__path__ = [base]
    sys.modules[PKG] = pkg
    mods = {}
    for name in ("encoder", "decoder", "factorize", "processor", "model"):
        spec = importlib.util.spec_from_file_location(PKG + "." + name, os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[PKG + "." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def main():
    ref = _load_reference()
    tables = {}
    for name, (cfg, (b, h, w), seed) in co.CASES.items():
        model = co.fill_(ref["model"].CaFAForecaster(**cfg), seed).eval()
        with torch.no_grad():
            out = model(co.case_input(name))
        assert tuple(out.shape) == (b, cfg["output_channels"], h, w)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed),
                            meta=np.array([cfg[k] for k in co.META_KEYS] + [b, h, w], dtype=np.int64), out=out.numpy().astype(np.float32))
        tables["CaFAForecaster:" + name] = model
    fz = ref["factorize"]
    tables["CaFAEncoder"] = ref["encoder"].CaFAEncoder(3, 16, 2)
    tables["CaFADecoder"] = ref["decoder"].CaFADecoder(16, 3, 2)
    tables["CaFAProcessor"] = ref["processor"].CaFAProcessor(16, 2, 2, 8)
    tables["AxialAttention"] = fz.AxialAttention(16, 2, 8)
    tables["FactorizedAttention"] = fz.FactorizedAttention(16, 2, 8)
    tables["FactorizedTransformerBlock"] = fz.FactorizedTransformerBlock(16, 2, 8)
    out = {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()}
    with open(os.path.join(GOLDEN, "cafa_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
