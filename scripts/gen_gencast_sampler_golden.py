"""Write tests/golden/gencast_sampler_b.npz and gencast_sampler.json from the reference's own sampler.py, weighted_mse_loss.py and
utils/noise.py.

Run from the repository root, on the CPU, with the reference tree present: ``python scripts/gen_gencast_sampler_golden.py``.
The reference's files are loaded read-only by path as in scripts/gen_gencast_model_golden.py, with the stand-ins of
tests/gencast_model_oracle.py.  ``torch_harmonics`` is not installed: the stand-in module gets an ``InverseRealSHT`` that is the
restatement of tests/gencast_sampler_oracle.py in float32 (the precision torch_harmonics runs in) and records every coefficient
tensor it is given.  The reference draws those coefficients with ``torch.randn`` on the CPU and nothing else in the loop draws, so
the unscaled draws are regenerated from the seed and checked against the recorded (scaled) ones bit for bit.

The npz holds the Denoiser case's name and seeds (weights come from tests/cafa_oracle.fill_ by seed, inputs from the case), the
unscaled coefficient draws, the schedule and the reference's output; the JSON the gammas of ``Sampler()`` and
``Sampler(num_steps=5)``, the reference's loss values on the cases of the oracle module and the two constructors' signatures.
Data only: no weights and no program text.

Condition of the sampler fixture (asserted here and in the GPU test): the float32 restatement's own error against float64 is at
most 1e-3 of the result's maximum, so the trajectory is well enough conditioned for the tests' bar to mean something.
"""
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle.refload import REF_ROOT  # noqa: E402
from tests import gencast_model_oracle as mo  # noqa: E402
from tests import gencast_sampler_oracle as so  # noqa: E402
from tests.cafa_oracle import fill_, params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = "graph_weather.models.gencast"
FILES = ("graph.icosahedral_mesh", "graph.model_utils", "graph.grid_mesh_connectivity", "graph.graph_builder", "utils.batching",
         "utils.noise", "layers.modules", "layers.encoder", "layers.processor", "layers.decoder", "denoiser", "sampler",
         "weighted_mse_loss")

RECORDED = []  # every coefficient tensor the reference hands to InverseRealSHT


class InverseRealSHT:
    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular"):
        assert grid == "equiangular" and lmax == so.lmax_of(nlat, nlon) and mmax == lmax + 1
        self.nlat, self.nlon = nlat, nlon

    def __call__(self, coeffs):
        assert coeffs.dtype == torch.complex64
        RECORDED.append(coeffs.clone())
        return so.isht(coeffs, self.nlat, self.nlon, torch.float32)


def _load_reference():
    stand_ins = mo.stand_in_modules()
    stand_ins["torch_harmonics"].InverseRealSHT = InverseRealSHT
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
            setattr(sys.modules[parent], leaf, mod)
            if name == "denoiser":
                sys.modules[BASE].Denoiser = mod.Denoiser  # (sampler.py imports it from the package)
            mods[name] = mod
    finally:
        for k in [k for k in sys.modules if k == "graph_weather" or k.startswith("graph_weather.") or k in stand_ins]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods


def _signature(cls):
    import inspect

    out = []
    for name, prm in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = prm.default
        out.append([name, "<required>" if d is inspect.Parameter.empty else
                    (d if isinstance(d, (bool, int, float, list, type(None))) else str(d))])
    return out


def _gammas(sampler):
    """The churn decisions of sampler.py's loop, with its float32 CPU sigmas."""
    sigmas = sampler._sigmas_fn(torch.arange(0, sampler.num_steps) / (sampler.num_steps - 1))
    gammas = [min(sampler.S_churn / sampler.num_steps, math.sqrt(2) - 1) if sampler.S_tmin <= sigmas[i] <= sampler.S_tmax else 0.0
              for i in range(len(sigmas) - 1)]
    return sigmas, gammas


def main():
    ref = _load_reference()
    Sampler, Loss, Denoiser = ref["sampler"].Sampler, ref["weighted_mse_loss"].WeightedMSELoss, ref["denoiser"].Denoiser

    # ---- the sampler -----------------------------------------------------------------------------------------------------------
    name = so.SAMPLER_CASE
    kw = mo.case_kwargs(name)
    seed = mo.CASES[name][3]
    model = fill_(Denoiser(**kw), seed).eval()
    prev = so.sampler_prev_inputs()
    sampler = Sampler(**so.SAMPLER_KW)
    del RECORDED[:]
    torch.manual_seed(so.SAMPLER_SEED)
    out = sampler.sample(model, prev)
    num_lon, num_lat, feats = len(kw["grid_lon"]), len(kw["grid_lat"]), kw["output_features_dim"]
    lmax = so.lmax_of(num_lat, num_lon)
    assert len(RECORDED) == sampler.num_steps
    torch.manual_seed(so.SAMPLER_SEED)
    draws = [torch.randn(feats, lmax, lmax + 1, dtype=torch.complex64) for _ in range(sampler.num_steps)]
    for d, r in zip(draws, RECORDED):
        assert torch.equal(d / np.sqrt((num_lat ** 2) // 2), r), "the regenerated draws are not the reference's"
    sigmas, gammas = _gammas(sampler)
    s2, g2 = so.schedule(**so.SAMPLER_KW)
    assert torch.equal(sigmas, s2) and gammas == g2

    # the restatement on the same draws: float32 is what the reference ran, float64 the yardstick's reference
    graphs = mo.graph_tables(model)
    res = {}
    for dtype in (torch.float32, torch.float64):
        fn = so.denoiser_fn(params(model, dtype), mo.CASES[name][0], mo.cast_graphs(graphs, dtype))
        with torch.no_grad():
            res[dtype] = so.sampler_sample(fn, prev, draws, num_lon, num_lat, dtype, **so.SAMPLER_KW)
    scale = res[torch.float64].abs().max().item()
    yard = (res[torch.float32].double() - res[torch.float64]).abs().max().item()
    ref_err = (out.double() - res[torch.float64]).abs().max().item()
    print("sampler: out %s max %.3e; float32 restatement error %.3e (%.2e of the maximum); reference against float64 %.3e"
          % (tuple(out.shape), scale, yard, yard / scale, ref_err))
    assert yard <= 1e-3 * scale, "ill-conditioned trajectory: shorten num_steps or narrow sigma_max"
    np.savez_compressed(os.path.join(GOLDEN, "gencast_sampler_b.npz"), case=np.str_(name), seed=np.int64(seed),
                        torch_seed=np.int64(so.SAMPLER_SEED), num_steps=np.int64(sampler.num_steps),
                        draws=np.stack([torch.view_as_real(d).numpy() for d in draws]), sigmas=sigmas.numpy(),
                        gammas=np.array(gammas, dtype=np.float64), out=out.numpy().astype(np.float32),
                        restatement_error=np.float64(yard))

    # ---- schedules, losses, signatures -----------------------------------------------------------------------------------------
    table = {"gammas": {}, "sigmas": {}, "loss": {}, "signature": {"Sampler": _signature(Sampler), "WeightedMSELoss": _signature(Loss)}}
    for key, skw in (("default", {}), ("num_steps_5", dict(num_steps=5))):
        sg, gm = _gammas(Sampler(**skw))
        table["gammas"][key] = gm
        table["sigmas"][key] = [float(v) for v in sg]
    for case in so.LOSS_CASES:
        lkw, pred, sigma, target = so.loss_case(case)
        value = Loss(**lkw)(pred, sigma, target)
        aw, fw = so.loss_weights(**lkw)
        want = so.weighted_mse_loss(pred, sigma, target, aw, fw)
        print("loss %s: reference %.9g, float64 restatement %.9g" % (case, value.item(), want.item()))
        assert abs(value.item() - want.item()) <= 1e-5 * abs(want.item())
        table["loss"][case] = float(value.item())
    with open(os.path.join(GOLDEN, "gencast_sampler.json"), "w") as f:
        json.dump(table, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
