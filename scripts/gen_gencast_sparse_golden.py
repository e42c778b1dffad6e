"""Write tests/golden/gencast_sparse_*.npz and gencast_sparse_state_dict.json from the reference's own sparse-processor classes.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_gencast_sparse_golden.py``.  The
reference's files - the GenCast graph, batching, noise and layer files that scripts/gen_gencast_model_golden.py loads, then
gencast/layers/experimental/sparse_transformer.py, both processor.py files, denoiser.py, genda/model.py and fgn/model.py - are loaded
read-only by path under oracle.refload.REF_ROOT under their own module names, with the stand-ins of tests/gencast_model_oracle.py
registered for the packages that are not installed and the torch-only stand-in of tests/gencast_sparse_oracle.py registered as
``dgl`` / ``dgl.sparse`` (DGL is not installed and not part of the reference): the reference's ``sparse=True`` branch then runs
its own ``SparseAttention`` and ``SparseTransformer`` on it.

Weights come from tests/cafa_oracle.fill_ (per-key seeded) and inputs from numpy.RandomState(seed).  Recorded per case: the seed,
the inputs, the eval output and the training-mode output (the classes hold no dropout: the generator asserts the two are bitwise
equal); for the GenDA case also ``guided_forward``.  The fixtures hold no weights and no program text.  The JSON records the
``state_dict`` key / shape tables of a sparse ``Processor`` (GenCast's and FGN's), ``Denoiser``, ``GenDA`` and FGN, the attributes
of the two classes and the constructors' signatures.
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
from tests import gencast_model_oracle as mo  # noqa: E402
from tests import gencast_sparse_oracle as so  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = "graph_weather.models"
FILES = ("gencast.graph.icosahedral_mesh", "gencast.graph.model_utils", "gencast.graph.grid_mesh_connectivity", "gencast.graph.graph_builder",
         "gencast.utils.batching", "gencast.utils.noise", "gencast.layers.modules", "gencast.layers.experimental.sparse_transformer",
         "gencast.layers.encoder", "gencast.layers.processor", "gencast.layers.decoder", "gencast.denoiser", "genda.model",
         "fgn.layers.processor", "fgn.model")
PACKAGES = ("graph_weather", MODELS, MODELS + ".gencast", MODELS + ".gencast.graph", MODELS + ".gencast.utils", MODELS + ".gencast.layers",
            MODELS + ".gencast.layers.experimental", MODELS + ".genda", MODELS + ".fgn", MODELS + ".fgn.layers")


def _load_reference():
    stand_ins = dict(mo.stand_in_modules(), **so.dgl_modules())
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
            if leaf == "sparse_transformer":  # what the package's __init__ exports: the processors import it from the package
                sys.modules[parent].SparseTransformer = mod.SparseTransformer
            mods[name] = mod
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods


def _both_modes(module, run):
    """(eval output, training-mode output) of ``run(module)``, asserted bitwise equal."""
    with torch.no_grad():
        out = run(module.eval())
        train = run(module.train())
    module.eval()
    assert torch.equal(out, train)
    return out.numpy().astype(np.float32), train.numpy().astype(np.float32)


def main():
    ref = _load_reference()
    st = ref["gencast.layers.experimental.sparse_transformer"]
    assert ref["gencast.layers.processor"].has_dgl and ref["fgn.layers.processor"].has_dgl
    classes = types.SimpleNamespace(SparseAttention=st.SparseAttention, SparseTransformer=st.SparseTransformer,
                                    Processor=ref["gencast.layers.processor"].Processor, FgnProcessor=ref["fgn.layers.processor"].Processor)
    tables, attrs = {}, {}
    for name, (kind, cfg, n, seed) in so.CASES.items():
        module = so.build(classes, name)
        inp = so.case_inputs(name)
        adj = so.spmatrix(inp["edge_index"], shape=(n, n)) if kind == "attention" else None
        out, train = _both_modes(module, lambda m: so.call(m, name, inp, adj))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed), out=out, train_out=train,
                            **{k: v.numpy() for k, v in inp.items()})
        tables[name] = {k: list(v.shape) for k, v in module.state_dict().items()}
        attrs[name] = sorted(k for k in list(module._modules) + [a for a in vars(module) if not a.startswith("_") and a != "training"])
        print(name, "out", out.shape, "entries", inp["edge_index"].shape[1], "tensors", len(tables[name]))

    shim = {"graph.grid_mesh_connectivity": ref["gencast.graph.grid_mesh_connectivity"]}
    model_cls = {"denoiser": ref["gencast.denoiser"].Denoiser, "genda": ref["genda.model"].GenDA,
                 "fgn": ref["fgn.model"].FunctionalGenerativeNetwork}
    for name, (kind, ckw, B, seed) in so.MODEL_CASES.items():
        kw = so.model_kwargs(name)
        model = fill_(model_cls[kind](**kw), seed).eval()
        gap = _check_gaps(model, kw["grid_lon"], kw["grid_lat"], shim)
        inputs = so.model_inputs(name)
        keep = dict(seed=np.int64(seed), min_gap=np.float64(gap), khop_entries=np.int64(model.khop_mesh_edge_index.shape[1]),
                    mesh_nodes=np.int64(model.khop_mesh_nodes.shape[0]))
        if kind == "fgn":
            x, noise = inputs
            with torch.no_grad():  # member by member through the reference's own stages, on the recorded noise vectors
                flat = x.reshape(x.shape[0], -1, x.shape[-1])
                members = []
                for m in range(noise.shape[1]):
                    latent_grid, latent_mesh = model._run_encoder(flat)
                    latent_mesh = model._run_processor(latent_mesh, noise_vectors=noise[:, m])
                    members.append(model._run_decoder(latent_mesh, latent_grid).reshape(x.shape[0], model.num_lon, model.num_lat, -1))
            keep.update(x=x.numpy(), noise=noise.numpy(), out=torch.stack(members, dim=1).numpy().astype(np.float32))
        else:
            names = ("z", "x", "sigma", "mask", "values")
            keep.update({k: v.numpy() for k, v in zip(names, inputs)})
            keep["out"], keep["train_out"] = _both_modes(model, lambda m: m(*inputs))
            if kind == "genda":
                with torch.no_grad():
                    keep["guided"] = model.guided_forward(*inputs, gamma=so.GAMMA).numpy().astype(np.float32)
                keep["gamma"] = np.float64(so.GAMMA)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **keep)
        tables[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        print(name, "out", keep["out"].shape, "min gap %.3e" % gap, "tensors", len(tables[name]), "khop entries", int(keep["khop_entries"]))
    out = {"state_dict": tables, "attributes": attrs,
           "signature": {"SparseAttention": _signature(st.SparseAttention), "SparseTransformer": _signature(st.SparseTransformer)}}
    with open(os.path.join(GOLDEN, "gencast_sparse_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
