"""FGN on the device: the ensemble-shared route (``FunctionalGenerativeNetwork.forward``) beside the member loop
(``fgn._forward_member_loop``: the reference's route, one member at a time at batch B, on the same kernels).

Default size: the configuration of gencast_model_probe.py - splits 4 (2 562 mesh nodes), 3 hops, ``hidden_dims=[512, 512]``, 4
blocks, 4 heads, a 2 degree grid (180 x 91) - with noise dimension 32, at (B, N) = (1, 2), (2, 4) and (1, 1); forward (eval,
no_grad) and forward + backward (train).  Both routes run on the same device, same weights, same inputs and noise vectors,
alternating inside one loop after a warm-up; wall clock around single calls with the device synchronised at both ends;
``--iters`` repeats reported as median [minimum .. maximum]; the peak of ``torch.cuda.max_memory_allocated`` over one call of each
route beside them.  Then the fan-out ConditionalLayerNorm kernel beside repeat + the grouped kernel, forward and backward, with
the fan-out's algorithmic bytes (forward: x read once, N outputs written; backward: x and N dout read, dx written).  The log goes
to profiles/fgn_probe.log (``--log`` to change it).  Nothing is gated on these numbers.

    python scripts/probes/fgn_probe.py [--iters 10] [--splits 4] [--hops 3] [--hidden 512] [--blocks 4] [--degrees 2]
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

from graph_weather_amd import fgn, gencast  # noqa: E402
from graph_weather_amd.fgn import FunctionalGenerativeNetwork, _forward_member_loop  # noqa: E402
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
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            out[i].append(_time(fn))
    return out


def fmt(ts):
    return "%9.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def peak(fn):
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
    ap.add_argument("--noise", type=int, default=32, help="noise_dimension")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fgn_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fgn_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lon = np.arange(0.0, 360.0, args.degrees)
    lat = np.arange(-90.0, 90.0 + 1e-9, args.degrees)
    model = fill_(FunctionalGenerativeNetwork(grid_lon=lon, grid_lat=lat, input_features_dim=args.features,
                                              output_features_dim=args.features, noise_dimension=args.noise,
                                              hidden_dims=[args.hidden, args.hidden], num_blocks=args.blocks, num_heads=args.heads,
                                              splits=args.splits, num_hops=args.hops), 1).to(dev)
    M = int(model.mesh_nodes.shape[0])
    lines = ["fgn_probe: %s, grid %d x %d (%d nodes), mesh %d nodes, g2m %d / k-hop %d / m2g %d edges, hidden %d, %d blocks, %d heads, "
             "%d features, noise %d, wall clock with the device synchronised at both ends, median of %d [minimum .. maximum]"
             % (torch.cuda.get_device_name(0), len(lon), len(lat), len(lon) * len(lat), M, model.g2m_edge_index.shape[1],
                model.khop_mesh_edge_index.shape[1], model.m2g_edge_index.shape[1], args.hidden, args.blocks, args.heads, args.features,
                args.noise, args.iters)]
    print(lines[0], flush=True)
    rs = np.random.RandomState(5)
    for B, N in ((1, 2), (2, 4), (1, 1)):
        x = torch.from_numpy(rs.standard_normal((B, len(lon), len(lat), args.features)).astype(np.float32)).to(dev)
        noise = torch.from_numpy(rs.standard_normal((B, N, args.noise)).astype(np.float32)).to(dev)

        def call(route, xx):
            return model(xx, num_ensemble=N, noise_vectors=noise) if route == "shared" else _forward_member_loop(model, xx, noise)

        def fwd(route):
            def run():
                with torch.no_grad():
                    return call(route, x)
            return run

        def train(route):
            def run():
                model.zero_grad(set_to_none=True)
                call(route, x.clone().requires_grad_(True)).square().mean().backward()
            return run

        model.eval()
        with torch.no_grad():
            diff = (fwd("shared")() - fwd("loop")()).abs().max().item()
        for what, make in (("forward", fwd), ("forward + backward", train)):
            model.train(what != "forward")
            sh, lp = timings([make("shared"), make("loop")], args.iters)
            m_sh, m_lp = peak(make("shared")), peak(make("loop"))
            line = ("B %d N %d %-18s shared %s  member loop %s  ratio %.2f  peak MiB shared %.0f member loop %.0f"
                    % (B, N, what, fmt(sh), fmt(lp), statistics.median(lp) / statistics.median(sh), m_sh, m_lp))
            print(line, flush=True)
            lines.append(line)
        lines.append("B %d N %d max |shared - member loop| of the eval output: %.3e" % (B, N, diff))
        print(lines[-1], flush=True)

    # the fan-out kernel beside repeat + the grouped kernel, on the first block's rows
    W = args.hidden
    for B, N in ((1, 2), (2, 4), (1, 8)):
        xr = torch.from_numpy(rs.standard_normal((B * M, W)).astype(np.float32)).to(dev)
        sc, bi = (torch.from_numpy(rs.standard_normal((B * N, W)).astype(np.float32)).to(dev) for _ in range(2))
        dout = torch.from_numpy(rs.standard_normal((B * N * M, W)).astype(np.float32)).to(dev)

        def repeat():
            return xr.view(B, 1, M, W).expand(B, N, M, W).reshape(B * N * M, W)

        def bwd_repeat():
            dx = gencast.cond_layernorm_grouped_backward(repeat(), sc, bi, M, "silu", dout)[0]
            return dx.view(B, N, M, W).sum(1)

        f_fan, f_rep, b_fan, b_rep = timings([lambda: fgn.cond_layernorm_fanout_forward(xr, sc, bi, M, N, "silu"),
                                              lambda: gencast.cond_layernorm_grouped_forward(repeat(), sc, bi, M, "silu"),
                                              lambda: fgn.cond_layernorm_fanout_backward(xr, sc, bi, M, N, "silu", dout), bwd_repeat],
                                             args.iters, warm=3)
        fb, bb = 4.0 * M * W * B * (1 + N), 4.0 * M * W * B * (2 + N)
        line = ("fan-out norm B %d N %d [%d x %d]: forward fan-out %s (%.0f GB/s of %.1f MB) repeat + grouped %s; backward fan-out %s "
                "(%.0f GB/s of %.1f MB) repeat + grouped + member sum %s"
                % (B, N, B * M, W, fmt(f_fan), fb / statistics.median(f_fan) / 1e6, fb / 1e6, fmt(f_rep), fmt(b_fan),
                   bb / statistics.median(b_fan) / 1e6, bb / 1e6, fmt(b_rep)))
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
