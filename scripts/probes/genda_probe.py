"""GenDA on the device: ``forward``, the one-pass ``guided_forward`` beside the reference's composition (two ``forward`` calls and
the torch-op combine) and beside the replicated route at batch 2 B (``genda._forward_replicated`` on the doubled inputs and the
torch-op combine), the two kernels of csrc/gw_genda.hip against the bytes they move, and allocation peaks.

Default size: the Denoiser probe's - splits 4 (2 562 mesh nodes), 3 hops, ``hidden_dims=[512, 512]``, 4 blocks, 4 heads, a 2 degree
grid (180 x 91) - for batch sizes 1 and 4, eval mode (no conditioning dropout draw).  Routes run on the same device, same weights,
same inputs, alternating inside one loop after a warm-up; wall clock around single calls with the device synchronised at both ends;
``--iters`` repeats reported as median [minimum .. maximum]; the peak of ``torch.cuda.max_memory_allocated`` over one call of each
route.  The log goes to profiles/genda_probe.log (``--log`` to change it).  Nothing is gated on these numbers.

    python scripts/probes/genda_probe.py [--iters 10] [--splits 4] [--hops 3] [--hidden 512] [--blocks 4] [--degrees 2]
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

from graph_weather_amd import gencast, genda  # noqa: E402
from graph_weather_amd.genda import GenDA, _forward_replicated  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timings(fns, iters, warm=2):
    for _ in range(warm):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            out[i].append(_time(fn))
    return out


def fmt(ts):
    return "%9.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def peak(fn):
    del gencast._PLANS[:]  # (no route keeps another's plans)
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
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "genda_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("genda_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lon = np.arange(0.0, 360.0, args.degrees)
    lat = np.arange(-90.0, 90.0 + 1e-9, args.degrees)
    model = fill_(GenDA(grid_lon=lon, grid_lat=lat, input_features_dim=args.features, output_features_dim=args.features,
                        hidden_dims=[args.hidden, args.hidden], num_blocks=args.blocks, num_heads=args.heads, splits=args.splits,
                        num_hops=args.hops), 1).to(dev).eval()
    G, gamma = len(lon) * len(lat), args.gamma
    lines = ["genda_probe: %s, grid %d x %d (%d nodes), mesh %d nodes, g2m %d / k-hop %d / m2g %d edges, hidden %d, %d blocks, %d heads, "
             "%d + 2 x %d + 2 features, gamma %g, eval mode, wall clock with the device synchronised at both ends, median of %d "
             "[minimum .. maximum]"
             % (torch.cuda.get_device_name(0), len(lon), len(lat), G, model.mesh_nodes.shape[0], model.g2m_edge_index.shape[1],
                model.khop_mesh_edge_index.shape[1], model.m2g_edge_index.shape[1], args.hidden, args.blocks, args.heads, args.features,
                args.features, gamma, args.iters)]
    print(lines[0], flush=True)

    def say(line):
        print(line, flush=True)
        lines.append(line)

    rs = np.random.RandomState(5)
    for B in args.batches:
        z = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), args.features)).astype(np.float32)).to(dev)
        x = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), 2 * args.features)).astype(np.float32)).to(dev)
        s = torch.from_numpy(np.linspace(0.1, 10.0, B).astype(np.float32)[:, None]).to(dev)
        mask = torch.from_numpy((rs.random_sample((B, len(lon), len(lat), 1)) < 0.3).astype(np.float32)).to(dev)
        values = mask * torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), 1)).astype(np.float32)).to(dev)
        zero = torch.zeros_like(mask)

        def routes(zz, xx):
            def one_pass():
                return model.guided_forward(zz, xx, s, mask, values, gamma)

            def two_pass():
                cond = model(zz, xx, s, mask, values)
                uncond = model(zz, xx, s, torch.zeros_like(mask), torch.zeros_like(values))
                return uncond + gamma * (cond - uncond)

            def replicated():
                both = _forward_replicated(model, torch.cat([zz, zz]), torch.cat([xx, xx]), torch.cat([s, s]), torch.cat([mask, zero]),
                                           torch.cat([values, zero]))
                return both[B:] + gamma * (both[:B] - both[B:])

            return dict(one_pass=one_pass, two_pass=two_pass, replicated=replicated, forward=lambda: model(zz, xx, s, mask, values))

        def eval_(name):
            def run():
                with torch.no_grad():
                    return routes(z, x)[name]()
            return run

        def train(name):
            def run():
                model.zero_grad(set_to_none=True)
                zz, xx = z.clone().requires_grad_(True), x.clone().requires_grad_(True)
                routes(zz, xx)[name]().square().mean().backward()
            return run

        names = ("forward", "one_pass", "two_pass", "replicated")
        outs = {n: eval_(n)() for n in names}
        for what, make in (("forward", eval_), ("forward + backward", train)):
            ts = dict(zip(names, timings([make(n) for n in names], args.iters)))
            pk = {n: peak(make(n)) for n in names}
            med = {n: statistics.median(ts[n]) for n in names}
            say("B %d %-18s forward          %s  peak %.0f MiB" % (B, what, fmt(ts["forward"]), pk["forward"]))
            say("B %d %-18s guided one pass  %s  peak %.0f MiB" % (B, what, fmt(ts["one_pass"]), pk["one_pass"]))
            say("B %d %-18s two forwards     %s  peak %.0f MiB  time ratio to one pass %.2f" % (B, what, fmt(ts["two_pass"]), pk["two_pass"],
                                                                                                 med["two_pass"] / med["one_pass"]))
            say("B %d %-18s replicated 2 B   %s  peak %.0f MiB  time ratio to one pass %.2f" % (B, what, fmt(ts["replicated"]), pk["replicated"],
                                                                                                 med["replicated"] / med["one_pass"]))
        say("B %d max |one pass - two forwards| of the eval output: %.3e; |one pass - replicated|: %.3e (maximum %.3e)"
            % (B, (outs["one_pass"] - outs["two_pass"]).abs().max().item(), (outs["one_pass"] - outs["replicated"]).abs().max().item(),
               outs["one_pass"].abs().max().item()))
        # the two kernels alone: bytes read and written against the time of one call
        zf, xf = z.reshape(-1, args.features), x.reshape(-1, 2 * args.features)
        stat, w_s = model.g2m_grid_nodes, int(model.g2m_grid_nodes.shape[1])
        preds = torch.randn(2 * B * G, args.features, device=dev)
        w_in = 3 * args.features + 2
        in_bytes = 4 * (B * G * w_in + G * w_s + 2 * B * G * (w_in + w_s))
        out_bytes = 4 * B * G * args.features * 4
        t_in, t_out = timings([lambda: genda.genda_input_forward(zf, xf, s, stat, mask.reshape(-1, 1), values.reshape(-1, 1), 2, False),
                               lambda: genda.guided_output_forward(zf, preds, s, gamma)], args.iters)
        for what, ts, nbytes in (("input kernel, 2 copies", t_in, in_bytes), ("guided output kernel", t_out, out_bytes)):
            say("B %d %-24s %s  %.2f MB moved  %.0f GB/s at the median (one call, launch and synchronisation included)"
                % (B, what, fmt(ts), nbytes / 1e6, nbytes / 1e9 / (statistics.median(ts) * 1e-3)))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
