"""Write tests/golden/thermalizer_*.npz, thermalizer_state_dict.json and thermalizer_grid.json from the reference's own
ThermalizerLayer.

Run from the repository root with the reference tree present: ``python scripts/gen_thermalizer_golden.py``.  The reference
is loaded read-only through oracle.refload.  Inputs are drawn from numpy.RandomState(seed) and, during the reference call,
torch.randn_like is replaced by a draw from numpy.RandomState(seed + 1): the fixtures store the seed, not the noise.  Weights
come from tests/thermal_oracle.fill_ (per-key seeded), so the test rebuilds the same layer; no weights are stored.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from tests import thermal_oracle as to  # noqa: E402
from oracle.refload import load_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (B, H, W, F, t, seed): both branches, several timesteps
CASES = [(1, 1, 244, 3, 500, 1), (2, 2, 2, 32, 0, 2), (2, 4, 4, 3, 999, 3), (2, 5, 5, 3, 500, 4), (2, 6, 8, 32, 250, 5),
         (2, 13, 9, 3, 500, 6), (1, 6, 8, 256, 500, 7)]


def main():
    ns = load_reference()
    thermal = sys.modules["graph_weather.models.layers.thermalizer"]
    for B, H, W, F, t, seed in CASES:
        layer = to.fill_(thermal.ThermalizerLayer(F), seed)
        x = torch.from_numpy(np.random.RandomState(seed).standard_normal((B * H * W, F)).astype(np.float32))
        rs = np.random.RandomState(seed + 1)
        saved = torch.randn_like
        torch.randn_like = lambda a: torch.from_numpy(rs.standard_normal(tuple(a.shape)).astype(np.float32)).to(a.dtype)
        try:
            with torch.no_grad():
                out = layer(x, t, height=H, width=W, batch=B)
        finally:
            torch.randn_like = saved
        name = "thermalizer_b%d_%dx%d_f%d_t%d.npz" % (B, H, W, F, t)
        np.savez_compressed(os.path.join(GOLDEN, name), meta=np.array([B, H, W, F, t, seed], dtype=np.int64),
                            out=out.numpy().astype(np.float32))
    from graph_weather_amd.utils import regular_lat_lons

    tables = {"ThermalizerLayer(256)": thermal.ThermalizerLayer(256), "ThermalizerLayer(32)": thermal.ThermalizerLayer(32),
              "GraphWeatherForecaster(30deg, use_thermalizer=True)": ns.GraphWeatherForecaster(regular_lat_lons(30.0),
                                                                                               use_thermalizer=True)}
    out = {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()}
    with open(os.path.join(GOLDEN, "thermalizer_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)
    # the reference's _infer_grid_dimensions: every N up to 2 000 and the forecaster's B * M at mesh resolutions 0-2
    infer = thermal.ThermalizerLayer(3)._infer_grid_dimensions
    ns = sorted(set(range(1, 2001)) | {m * b for m in (122, 842, 5882) for b in range(1, 65)})
    with open(os.path.join(GOLDEN, "thermalizer_grid.json"), "w") as f:
        json.dump([[n, *infer(n)] for n in ns], f, separators=(",", ":"))


if __name__ == "__main__":
    main()
