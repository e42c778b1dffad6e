"""GenCast's sparse processor on the device: ``Processor(sparse="native")`` through the kernels of csrc/gw_sparse_attn.hip beside
(a) the same arithmetic as a torch-op composition (``index_select`` and a scatter softmax over the replicated mask, ``F.linear``,
``F.layer_norm``) and (b) the existing ``sparse=False`` processor without edge features on the same graph - a different model (the
reference says so), context and not a bar; the attention launch alone against its algorithmic bytes; allocation peaks.

Default size: the GenDA probe's mesh - splits 4 (2 562 mesh nodes), 3 hops, ``hidden_dims=[512, 512]``, 4 heads, 4 blocks - for batch
sizes 1 and 4, eval mode.  Routes run on the same device, same inputs, alternating inside one loop after a warm-up; wall clock around
single calls with the device synchronised at both ends; ``--iters`` repeats reported as median [minimum .. maximum]; the peak of
``torch.cuda.max_memory_allocated`` over one call of each route.  The attention launch is timed as 10 launches between two
synchronisations, divided by 10.  The log goes to profiles/gencast_sparse_probe.log (``--log`` to change it).  Nothing is gated on
these numbers.

    python scripts/probes/gencast_sparse_probe.py [--iters 10] [--splits 4] [--hops 3] [--hidden 512] [--blocks 4] [--heads 4]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from graph_weather_amd import gencast, gencast_sparse  # noqa: E402
from graph_weather_amd.gencast_graphs import GraphBuilder  # noqa: E402
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
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def torch_composition(proc, x, ei_rep, noise_rows, n_rows):
    """The sparse processor's forward as torch operations on the device (the reference's arithmetic, one replicated mask)."""
    fe = proc.fourier_embedder
    freqs = torch.exp(-np.log(fe.base_period) * torch.arange(0, fe.num_frequencies, dtype=torch.float32, device=x.device) / fe.num_frequencies)
    args = noise_rows * freqs[None, :]
    emb = fe.mlp(torch.cat([torch.cos(args), torch.sin(args)], dim=-1))
    row, col = ei_rep[0], ei_rep[1]

    def cln(norm, t):
        return norm.linear_scale(emb) * F.layer_norm(t, (t.shape[-1],), None, None, 1e-5) + norm.linear_bias(emb)

    for blk in proc.cond_transformers:
        att = blk.sparse_attention
        nh, dh = att.num_heads, att.head_dim
        x1 = cln(blk.cond_norm_1, x)
        q = (att.q_proj(x1) * att.scaling).reshape(n_rows, dh, nh)
        k, v = att.k_proj(x1).reshape(n_rows, dh, nh), att.v_proj(x1).reshape(n_rows, dh, nh)
        s = (q.index_select(0, row) * k.index_select(0, col)).sum(dim=1)  # [E, nh]
        idx = row[:, None].expand_as(s)
        smax = torch.full((n_rows, nh), -float("inf"), device=x.device).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
        ex = (s - smax.index_select(0, row)).exp()
        den = torch.zeros((n_rows, nh), device=x.device).index_add_(0, row, ex)
        p = ex / den.index_select(0, row)
        out = torch.zeros((n_rows, dh, nh), device=x.device).index_add_(0, row, p[:, None, :] * v.index_select(0, col))
        x = x + att.out_proj(out.reshape(n_rows, -1))
        x = x + blk.mlp(cln(blk.cond_norm_2, x))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--splits", type=int, default=4)
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gencast_sparse_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gencast_sparse_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    graphs = GraphBuilder(grid_lon=np.arange(0.0, 360.0, 30.0), grid_lat=np.arange(-75.0, 76.0, 30.0), splits=args.splits, num_hops=args.hops,
                          device=torch.device("cpu"), add_edge_features_to_khop=False)
    ei = graphs.khop_mesh_graph.edge_index.to(dev)
    M, E, D, nh = int(graphs.khop_mesh_graph.x.shape[0]), int(ei.shape[1]), args.hidden, args.heads
    kw = dict(latent_dim=D, hidden_dims=[D, D], num_blocks=args.blocks, num_heads=nh, num_frequencies=32, base_period=16, noise_emb_dim=16,
              activation_layer=torch.nn.SiLU)
    native = fill_(gencast.Processor(sparse="native", **kw), 1).to(dev).eval()
    dense = fill_(gencast.Processor(sparse=False, **kw), 1).to(dev).eval()
    deg = torch.bincount(ei[0], minlength=M)
    lines = ["gencast_sparse_probe: %s, mesh %d nodes, k-hop mask %d entries (per row: median %d, maximum %d), width %d, %d heads, %d blocks, "
             "eval mode, wall clock with the device synchronised at both ends, median of %d [minimum .. maximum]"
             % (torch.cuda.get_device_name(0), M, E, int(deg.median()), int(deg.max()), D, nh, args.blocks, args.iters)]
    print(lines[0], flush=True)

    def say(line):
        print(line, flush=True)
        lines.append(line)

    rs = np.random.RandomState(5)
    for B in args.batches:
        x = torch.from_numpy(rs.standard_normal((B * M, D)).astype(np.float32)).to(dev)
        noise = torch.from_numpy(np.linspace(-0.5, 0.5, B).astype(np.float32)[:, None]).to(dev)
        noise_rows = noise.repeat_interleave(M, 0)
        ei_rep = torch.cat([ei + b * M for b in range(B)], dim=1)

        def routes(xx):
            return dict(native=lambda: native._forward_shared(xx, ei, noise, None, B),
                        torch_ops=lambda: torch_composition(native, xx, ei_rep, noise_rows, B * M),
                        dense=lambda: dense._forward_shared(xx, ei, noise, None, B))

        def eval_(name):
            def run():
                with torch.no_grad():
                    return routes(x)[name]()
            return run

        def train(name):
            def run():
                (native if name != "dense" else dense).zero_grad(set_to_none=True)
                xx = x.clone().requires_grad_(True)
                routes(xx)[name]().square().mean().backward()
            return run

        names = ("native", "torch_ops", "dense")
        outs = {n: eval_(n)() for n in names}
        for what, make in (("forward", eval_), ("forward + backward", train)):
            ts = dict(zip(names, timings([make(n) for n in names], args.iters)))
            pk = {n: peak(make(n)) for n in names}
            med = {n: statistics.median(ts[n]) for n in names}
            say("B %d %-18s sparse, native kernels   %s  peak %.0f MiB" % (B, what, fmt(ts["native"]), pk["native"]))
            say("B %d %-18s sparse, torch ops        %s  peak %.0f MiB  time ratio to native %.2f"
                % (B, what, fmt(ts["torch_ops"]), pk["torch_ops"], med["torch_ops"] / med["native"]))
            say("B %d %-18s sparse=False, no edges   %s  peak %.0f MiB  time ratio to native %.2f (another model: context)"
                % (B, what, fmt(ts["dense"]), pk["dense"], med["dense"] / med["native"]))
        say("B %d max |native - torch ops| of the eval output: %.3e (maximum %.3e)"
            % (B, (outs["native"] - outs["torch_ops"]).abs().max().item(), outs["native"].abs().max().item()))
        # the attention launches alone, q / k / v read in place from one stacked table
        plan = gencast_sparse.sparse_plan(ei, M).plan
        qkv = torch.randn(B * M, 3 * D, device=dev)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        scale = (D // nh) ** -0.5
        out, lse = gencast_sparse.sparse_attention_forward(q, k, v, plan, nh, scale, B)
        dout = torch.randn_like(out)

        def fwd10():
            for _ in range(10):
                gencast_sparse.sparse_attention_forward(q, k, v, plan, nh, scale, B)

        def bwd10():
            for _ in range(10):
                gencast_sparse.sparse_attention_backward(q, k, v, plan, nh, scale, B, out, lse, dout, stacked=True)

        t_f, t_b = timings([fwd10, bwd10], args.iters)
        gather = B * E * 2 * 4 * D
        fwd_bytes = gather + B * M * (2 * 4 * D + 2 * 4 * nh)  # + q read, out written, the two planes
        bwd_bytes = 2 * gather + B * M * (7 * 4 * D + 3 * 4 * nh) + B * E * (2 * 4 * D + 3 * 4 * nh)  # both walks; dq, dk, dv written
        for what, ts, nbytes in (("attention forward", t_f, fwd_bytes), ("attention backward (2 launches)", t_b, bwd_bytes)):
            med = statistics.median(ts) / 10
            say("B %d %-32s %9.3f ms per call [%.3f .. %.3f]  %.1f MB algorithmic  %.2f TB/s (whole-row gathers measure 5.5-5.8 TB/s from HBM; "
                "this table of %.1f MB is cache resident)"
                % (B, what, med, min(ts) / 10, max(ts) / 10, nbytes / 1e6, nbytes / 1e12 / (med * 1e-3), B * M * 3 * D * 4 / 1e6))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
