"""GenCast's Denoiser on the device: the batch-shared route (``Denoiser.forward``) beside the replicated route
(``gencast_model._forward_replicated``: the reference's ``hetero_batch`` / ``batch`` graphs through the layers' public forwards).

Default size: splits 4 (2 562 mesh nodes), 3 hops, ``hidden_dims=[512, 512]``, 4 blocks, 4 heads, a 2 degree grid (180 x 91), for
batch sizes 1 and 4; forward (eval, no_grad) and forward + backward (train).  Both routes run on the same device, same weights,
same inputs, alternating inside one loop after a warm-up; HIP events around single calls; ``--iters`` repeats reported as median
[minimum .. maximum]; the peak of ``torch.cuda.max_memory_allocated`` over one call of each route beside them.  The log goes to
profiles/gencast_model_probe.log (``--log`` to change it).  Nothing is gated on these numbers.

    python scripts/probes/gencast_model_probe.py [--iters 10] [--splits 4] [--hops 3] [--hidden 512] [--blocks 4] [--degrees 2]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from graph_weather_amd import gencast  # noqa: E402
from graph_weather_amd.gencast_model import Denoiser, _forward_replicated  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timings(fns, iters, warm=2):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            out[i].append(_time(fn))
    return out


def fmt(ts):
    return "%9.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def peak(fn):
    del gencast._PLANS[:]  # (neither route keeps the other's plans)
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--splits", type=int, default=4)
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--degrees", type=float, default=2.0)
    ap.add_argument("--features", type=int, default=8, help="input_features_dim and output_features_dim")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gencast_model_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gencast_model_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lon = np.arange(0.0, 360.0, args.degrees)
    lat = np.arange(-90.0, 90.0 + 1e-9, args.degrees)
    model = fill_(Denoiser(grid_lon=lon, grid_lat=lat, input_features_dim=args.features, output_features_dim=args.features,
                           hidden_dims=[args.hidden, args.hidden], num_blocks=args.blocks, num_heads=args.heads, splits=args.splits,
                           num_hops=args.hops), 1).to(dev)
    lines = ["gencast_model_probe: %s, grid %d x %d (%d nodes), mesh %d nodes, g2m %d / k-hop %d / m2g %d edges, hidden %d, %d blocks, "
             "%d heads, %d + 2 x %d features, median of %d [minimum .. maximum]"
             % (torch.cuda.get_device_name(0), len(lon), len(lat), len(lon) * len(lat), model.mesh_nodes.shape[0],
                model.g2m_edge_index.shape[1], model.khop_mesh_edge_index.shape[1], model.m2g_edge_index.shape[1], args.hidden,
                args.blocks, args.heads, args.features, args.features, args.iters)]
    print(lines[0], flush=True)
    rs = np.random.RandomState(5)
    for B in args.batches:
        z = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), args.features)).astype(np.float32)).to(dev)
        x = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), 2 * args.features)).astype(np.float32)).to(dev)
        s = torch.from_numpy(np.linspace(0.1, 10.0, B).astype(np.float32)[:, None]).to(dev)

        def fwd(route):
            def run():
                with torch.no_grad():
                    return model(z, x, s) if route == "shared" else _forward_replicated(model, z, x, s)
            return run

        def train(route):
            def run():
                model.zero_grad(set_to_none=True)
                zz, xx = z.clone().requires_grad_(True), x.clone().requires_grad_(True)
                out = model(zz, xx, s) if route == "shared" else _forward_replicated(model, zz, xx, s)
                out.square().mean().backward()
            return run

        model.eval()
        with torch.no_grad():
            diff = (fwd("shared")() - fwd("replicated")()).abs().max().item()
        for what, make in (("forward", fwd), ("forward + backward", train)):
            model.train(what != "forward")
            sh, rep = timings([make("shared"), make("replicated")], args.iters)
            m_sh, m_rep = peak(make("shared")), peak(make("replicated"))
            line = ("B %d %-18s shared %s  replicated %s  ratio %.2f  peak MiB shared %.0f replicated %.0f"
                    % (B, what, fmt(sh), fmt(rep), statistics.median(rep) / statistics.median(sh), m_sh, m_rep))
            print(line, flush=True)
            lines.append(line)
        lines.append("B %d max |shared - replicated| of the eval output: %.3e" % (B, diff))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
