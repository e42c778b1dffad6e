"""PhysicalConstraintLayer cost at 1 degree, B = 2 (csrc/gw_constraint.hip): the constrained vs unconstrained inference
forward (AutoGraph replay on), each constraint type's forward and backward kernels alone with their HBM bytes and the
fraction of 6.3 TB/s they reach, and one training step (forward, NormalizedMSELoss, backward, AdamW) with and without.

    python scripts/probes/constraint_probe.py [--iters 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd._lib import CONSTRAINT_TYPES  # noqa: E402
from graph_weather_amd.constraint import ConstraintFunction  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

STREAM_BW = 6.3e12  # bytes/s a streaming kernel reaches on MI355X


def _name(dtype):
    return str(dtype).replace("torch.", "")


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lat_lons = regular_lat_lons(1.0)
    B, G, C, F = 2, len(lat_lons), 78, 102
    feats = seeded_features(B, G, F, seed=1).to(dev)
    target = feats[..., :C].clone()
    models = {}
    for ct in ("none",) + tuple(CONSTRAINT_TYPES):
        m = gw.GraphWeatherForecaster(lat_lons, constraint_type=ct)
        deterministic_fill_(m, seed=1)
        models[ct] = m.to(dev)
    print(f"1 deg, B={B}, G={G}, C={C}; {args.iters} iterations per figure; times in us")
    for dtype in (torch.float32, "bf16x3"):
        base = None
        for ct, m in models.items():
            m.eval().set_compute_dtype(dtype)
            with torch.no_grad():
                t = timed(lambda: m(feats), args.iters)
            base = t if ct == "none" else base
            extra = "" if ct == "none" else f"  (+{t - base:8.1f} us, {100 * (t - base) / base:+.2f} %)"
            print(f"forward  {_name(dtype):8s} {ct:15s} {t:10.1f}{extra}")
    # kernels alone on the forecaster's operands: hr = decoder output rows, lr = the features' first 78 channels
    layer = models["additive"].constraint
    maps = layer.maps("pi", dev)
    hit = int((layer._host["hit"] > 0).sum())
    hr = torch.randn(B, G, C, device=dev) + 1.0
    g = torch.randn(B, G, C, device=dev)
    row = B * C * 4
    for ct, code in CONSTRAINT_TYPES.items():
        spec = (code, 1, *layer.grid_shape, 0, 1.0)
        with torch.no_grad():
            t = timed(lambda: ConstraintFunction.apply(hr, feats, spec, maps), args.iters)
        # statistics read the hit rows of hr (and lr); apply reads hr (and lr) rows per node and writes the output
        stats = {"additive": hit * row, "multiplicative": 2 * hit * row, "softmax": 0}[ct]
        apply = G * row * (3 if ct != "multiplicative" else 2)
        byt = stats + apply
        print(f"kernel   forward  {ct:15s} {t:10.1f} us  {byt / 1e6:7.1f} MB  {byt / (t * 1e-6) / 1e12:5.2f} TB/s "
              f"({100 * byt / (t * 1e-6) / STREAM_BW:5.1f} % of 6.3)")
        hrq, lrq = hr.clone().requires_grad_(True), feats.clone().requires_grad_(True)
        y = ConstraintFunction.apply(hrq, lrq, spec, maps)
        t = timed(lambda: torch.autograd.grad(y, (hrq, lrq), g, retain_graph=True), args.iters)
        # dlr is a zero-filled [B, G, 102] tensor (aux columns), then every path reads g through the CSR and writes dhr, dlr
        stats_b = {"additive": G * row, "multiplicative": G * row + 3 * hit * row, "softmax": 0}[ct]
        byt = B * G * F * 4 + stats_b + G * row * (3 if ct != "softmax" else 5)
        print(f"kernel   backward {ct:15s} {t:10.1f} us  {byt / 1e6:7.1f} MB  {byt / (t * 1e-6) / 1e12:5.2f} TB/s "
              f"({100 * byt / (t * 1e-6) / STREAM_BW:5.1f} % of 6.3)  (incl. zero fill of the features-shaped gradient)")
    for dtype in (torch.float32, "bf16x3"):
        base = None
        for ct, m in models.items():
            m.train().set_compute_dtype(dtype)
            crit = gw.NormalizedMSELoss(lat_lons=lat_lons, feature_variance=[1.0] * C)
            opt = gw.AdamW(m.parameters(), lr=1e-6)

            def step():
                opt.zero_grad()
                crit(m(feats), target).backward()
                opt.step()

            t = timed(step, max(3, args.iters // 4), warm=2)
            base = t if ct == "none" else base
            extra = "" if ct == "none" else f"  (+{t - base:8.1f} us, {100 * (t - base) / base:+.2f} %)"
            print(f"train    {_name(dtype):8s} {ct:15s} {t:10.1f}{extra}")


if __name__ == "__main__":
    main()
