"""Write tests/golden/modulation_*.npz and modulation_state_dict.json from the reference's own StochasticDecompositionLayer,
FiLMGenerator and FiLMApplier.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_modulation_golden.py``.  The
two reference files (they import only torch) are loaded read-only by path under oracle.refload.REF_ROOT.  Inputs are drawn from
numpy.RandomState(seed) and, during the reference call, torch.randn_like is replaced by a draw from
numpy.RandomState(seed + 1): the fixtures store the seed, not the inputs.  Weights come from tests/modulation_oracle.fill_
(per-key seeded; alpha nonzero), so the tests rebuild the same layers; no weights are stored.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from tests import modulation_oracle as mo  # noqa: E402
from oracle.refload import REF_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load(name):
    path = os.path.join(REF_ROOT, "graph_weather", "models", "layers", name + ".py")
    spec = importlib.util.spec_from_file_location("_reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _save(name, meta, out):
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), meta=np.array(meta, dtype=np.int64), out=out.numpy().astype(np.float32))


def main():
    film, sdl = _load("film"), _load("stochastic_decomposition")
    for name, (shape, latent, seed) in mo.SDL_CASES.items():
        layer = mo.fill_(sdl.StochasticDecompositionLayer(shape[1], latent), seed)
        x, z, noise = mo.sdl_inputs(shape, latent, seed)
        saved = torch.randn_like
        torch.randn_like = lambda a: noise.to(a.dtype)
        try:
            with torch.no_grad():
                out = layer(x, z)
        finally:
            torch.randn_like = saved
        _save(name, list(shape) + [latent, seed], out)
    for name, (n_lead, hidden, feat, batch, lead, seed) in mo.GENERATOR_CASES.items():
        gen = mo.fill_(film.FiLMGenerator(n_lead, hidden, feat), seed)
        with torch.no_grad():
            gamma, beta = gen(batch, lead)
        _save(name, [n_lead, hidden, feat, batch, lead, seed], torch.stack([gamma, beta]))
    for name, (shape, seed) in mo.APPLIER_CASES.items():
        x, gamma, beta = mo.applier_inputs(shape, seed)
        with torch.no_grad():
            out = film.FiLMApplier()(x, gamma, beta)
        _save(name, list(shape) + [seed], out)
    tables = {"StochasticDecompositionLayer(32, 16)": sdl.StochasticDecompositionLayer(32, 16),
              "StochasticDecompositionLayer(78, 32)": sdl.StochasticDecompositionLayer(78, 32),
              "FiLMGenerator(10, 8, 16)": film.FiLMGenerator(10, 8, 16), "FiLMGenerator(40, 64, 78)": film.FiLMGenerator(40, 64, 78),
              "FiLMApplier()": film.FiLMApplier()}
    out = {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()}
    with open(os.path.join(GOLDEN, "modulation_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
