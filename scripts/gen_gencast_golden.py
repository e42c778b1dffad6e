"""Write tests/golden/gencast_*.npz and gencast_state_dict.json from the reference's own GenCast layer classes.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_gencast_golden.py``.
The reference's four ``graph_weather/models/gencast/layers`` files are loaded read-only by path under oracle.refload.REF_ROOT
under their own module names (processor.py imports modules.py absolutely), with the stand-ins of tests/gencast_oracle.py
registered as ``torch_geometric.nn`` / ``torch_geometric.nn.conv`` (torch_geometric is not installed and not part of the
reference).  Weights come from tests/gencast_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed): the fixtures
hold the seed, the meta and the outputs - no weights, no inputs.  The JSON also records the constructors' signatures.
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

from tests import gencast_oracle as go  # noqa: E402
from oracle.refload import REF_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = "graph_weather.models.gencast.layers"
CLASSES = ("MLP", "InteractionNetwork", "FourierEmbedding", "ConditionalLayerNorm", "CondTransformerBlock", "Encoder", "Processor",
           "Decoder")


def _load_reference():
    for name in ("torch_geometric", "torch_geometric.nn", "torch_geometric.nn.conv"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torch_geometric.nn"].MessagePassing = go.MessagePassing
    sys.modules["torch_geometric.nn.conv"].TransformerConv = go.TransformerConv
    base = os.path.join(REF_ROOT, "graph_weather", "models", "gencast", "layers")
    saved = {k: v for k, v in sys.modules.items() if k == "graph_weather" or k.startswith("graph_weather.")}
    for k in saved:
        del sys.modules[k]
    parts = BASE.split(".")
    for i in range(1, len(parts) + 1):  # empty packages: nothing of this repository's alias tree is imported meanwhile
        pkg = types.ModuleType(".".join(parts[:i]))
        pkg.__path__ = []
        sys.modules[pkg.__name__] = pkg
    ns = types.SimpleNamespace()
    try:
        for name in ("modules", "encoder", "processor", "decoder"):
            spec = importlib.util.spec_from_file_location(BASE + "." + name, os.path.join(base, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[BASE + "." + name] = mod
            spec.loader.exec_module(mod)
            for attr in CLASSES:
                if hasattr(mod, attr):
                    setattr(ns, attr, getattr(mod, attr))
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return ns


def _signature(cls):
    out = []
    for name, prm in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = prm.default
        if d is inspect.Parameter.empty:
            out.append([name, "<required>"])
        else:
            out.append([name, d.__name__ if inspect.isclass(d) else d])
    return out


def main():
    ref = _load_reference()
    tables = {}
    for name, (kind, _, _, seed) in go.CASES.items():
        module = go.build(ref, name)
        with torch.no_grad():
            outs = go.call(module, name, go.case_inputs(name))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed), meta=np.array(go.meta_of(name), dtype=np.int64),
                            **{"out%d" % i: o.numpy().astype(np.float32) for i, o in enumerate(outs)})
        tables[go.CLASS_OF[kind] + ":" + name] = module
    tables["InteractionNetwork"] = ref.InteractionNetwork(sender_dim=5, receiver_dim=6, edge_attr_dim=3, hidden_dims=[9, 8], use_layer_norm=True)
    tables["ConditionalLayerNorm"] = ref.ConditionalLayerNorm(conditioning_dim=5, features_dim=12)
    tables["CondTransformerBlock"] = ref.CondTransformerBlock(input_dim=12, output_dim=4, num_heads=3, conditioning_dim=5, edges_dim=6)
    tables["CondTransformerBlock:mean"] = ref.CondTransformerBlock(input_dim=12, output_dim=12, num_heads=3, concat=False)
    out = {"state_dict": {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()},
           "signature": {c: _signature(getattr(ref, c)) for c in CLASSES}}
    with open(os.path.join(GOLDEN, "gencast_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
