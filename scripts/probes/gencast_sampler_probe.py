"""GenCast's ``Sampler().sample`` on the device, on the Denoiser configuration of scripts/probes/gencast_model_probe.py (splits 4,
3 hops, ``hidden_dims=[512, 512]``, 4 blocks, 4 heads, 8 features, a 2 degree grid 180 x 91), and one isotropic-noise draw at 1
degree (360 x 181) for a model's field count.

Wall time of one ``sample`` (20 steps: 39 Denoiser calls, 20 noise fields) between two host clock reads with the device
synchronised at both, beside 39 Denoiser calls alone on the loop's shapes, timed the same way: the difference is what the sampler
spends outside the Denoiser (noise draws, state updates, host work between the launches).  The noise draw is timed with HIP events
around single calls, the coefficient draw (``torch.randn``) and the transform apart.  ``--iters`` repeats reported as median
[minimum .. maximum] after a warm-up.  The log goes to profiles/gencast_sampler_probe.log (``--log`` to change it).  Nothing is
gated on these numbers.

    python scripts/probes/gencast_sampler_probe.py [--iters 5] [--batches 1 4] [--fields 83]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from graph_weather_amd import ops  # noqa: E402
from graph_weather_amd.gencast_model import Denoiser, generate_isotropic_noise  # noqa: E402
from graph_weather_amd.gencast_sampler import Sampler  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def repeat(timer, fn, iters, warm=2):
    for _ in range(warm):
        fn()
    return [timer(fn) for _ in range(iters)]


def fmt(ts):
    return "%9.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--fields", type=int, default=83, help="field count of the 1 degree noise draw (GenCast's output features)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gencast_sampler_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gencast_sampler_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lon, lat = np.arange(0.0, 360.0, 2.0), np.arange(-90.0, 90.0 + 1e-9, 2.0)
    feats = 8
    model = fill_(Denoiser(grid_lon=lon, grid_lat=lat, input_features_dim=feats, output_features_dim=feats, hidden_dims=[512, 512],
                           num_blocks=4, num_heads=4, splits=4, num_hops=3), 1).to(dev).eval()
    sampler = Sampler()
    calls = 2 * (sampler.num_steps - 1) - 1
    lines = ["gencast_sampler_probe: %s, grid %d x %d, mesh %d nodes, hidden 512, 4 blocks, %d features, Sampler() = %d steps, %d Denoiser "
             "calls, %d noise fields, median of %d [minimum .. maximum]"
             % (torch.cuda.get_device_name(0), len(lon), len(lat), model.mesh_nodes.shape[0], feats, sampler.num_steps, calls,
                sampler.num_steps, args.iters)]
    print(lines[0], flush=True)
    rs = np.random.RandomState(5)
    for B in args.batches:
        prev = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), 2 * feats)).astype(np.float32)).to(dev)
        x = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), feats)).astype(np.float32)).to(dev)
        s = torch.full((B, 1), 1.5, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)

        def denoiser_only():
            with torch.no_grad():
                for _ in range(calls):
                    model._forward_impl(x, prev, s)

        total = repeat(wall, lambda: sampler.sample(model, prev, generator=gen), args.iters)
        inner = repeat(wall, denoiser_only, args.iters)
        out = sampler.sample(model, prev, generator=gen)
        share = 1.0 - statistics.median(inner) / statistics.median(total)
        line = ("B %d sample %s  %d Denoiser calls alone %s  outside the Denoiser %.1f %%  (result finite: %s, largest |value| %.2f)"
                % (B, fmt(total), calls, fmt(inner), 100.0 * share, bool(torch.isfinite(out).all()), out.abs().max().item()))
        print(line, flush=True)
        lines.append(line)
    # one draw at 1 degree
    nlon, nlat = 360, 181
    gen = torch.Generator(device=dev).manual_seed(2)
    lmax = nlat - 1
    c = torch.randn(args.fields, lmax, lmax + 1, dtype=torch.complex64, device=dev, generator=gen)
    draw = repeat(event, lambda: generate_isotropic_noise(nlon, nlat, args.fields, device=dev, generator=gen, batch=1), args.iters)
    randn = repeat(event, lambda: torch.randn(args.fields, lmax, lmax + 1, dtype=torch.complex64, device=dev, generator=gen), args.iters)
    transform = repeat(event, lambda: ops.isht_forward(c, nlat, nlon, args.fields, 1.0), args.iters)
    flops = 2.0 * args.fields * (2 * nlat * lmax * (lmax + 1) / 2 + 2 * nlat * lmax * nlon)
    line = ("noise draw %d x %d, %d fields: %s  of it torch.randn %s  the transform alone %s (%.2f TFLOP/s on its %.2f GFLOP)"
            % (nlon, nlat, args.fields, fmt(draw), fmt(randn), fmt(transform), flops / statistics.median(transform) / 1e9, flops / 1e9))
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
