"""GenCast's mesh processor on the device at the default size: 512 features, 4 heads, the 6-hop closure of the library's
resolution-3 mesh (41 162 nodes, built on the host with sparse products).

  (a) one CondTransformerBlock, forward and forward + backward, with and without edge features, for a concat=True block
      (4 heads of 128) and for the final concat=False block (4 heads of 512, head-mean);
  (b) the attention launch alone beside the torch-op composition on the same device (index_select, scatter softmax, index_add_:
      what PyG's TransformerConv does, tests/gencast_oracle.graph_attention), with the launch's algorithmic bytes - edges x bytes
      of the k, v (and e) rows it must read - over its time.  The composition materialises several [E, heads, C] temporaries
      (10.6 GB each for a concat=True block); where it does not fit the device the log says so.

HIP events around single calls after a warm-up; ``--iters`` repeats, reported as median [minimum .. maximum]; the routes of a
pair alternate inside one loop.  The log goes to profiles/gencast_probe.log (``--log`` to change it).  Nothing is gated on these
numbers.

    python scripts/probes/gencast_probe.py [--iters 10] [--hops 6] [--resolution 3]
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from graph_weather_amd import gencast, mesh  # noqa: E402
from tests import gencast_oracle as go  # noqa: E402


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


def khop_edges(resolution: int, hops: int) -> np.ndarray:
    """[2, E] int64: j -> i for every pair of mesh nodes within ``hops`` steps (self included), shuffled."""
    import scipy.sparse as sp

    m = mesh.get_mesh(resolution)
    ptr, idx = m.disk1_csr()
    a = sp.csr_matrix((np.ones(idx.size, dtype=np.float32), idx, ptr), shape=(m.num, m.num))
    r = a.copy()
    for _ in range(hops - 1):
        r = r @ a
        r.data[:] = 1.0
    r = r.tocoo()
    ei = np.stack([r.col, r.row]).astype(np.int64)
    return ei[:, np.random.RandomState(0).permutation(ei.shape[1])]


def composition(q, k, v, e, src, dst, n, heads, mean):
    """tests/gencast_oracle.graph_attention on the device."""
    C = q.shape[1] // heads
    qi, kj, vj = q.view(-1, heads, C).index_select(0, dst), k.view(-1, heads, C).index_select(0, src), v.view(-1, heads, C).index_select(0, src)
    if e is not None:
        ev = e.view(-1, heads, C)
        kj, vj = kj + ev, vj + ev
    s = (qi * kj).sum(-1) / math.sqrt(C)
    idx = dst[:, None].expand_as(s)
    smax = torch.full((n, heads), -math.inf, device=q.device).scatter_reduce(0, idx, s, "amax", include_self=True)
    ex = (s - smax.index_select(0, dst)).exp()
    den = torch.zeros((n, heads), device=q.device).index_add_(0, dst, ex) + 1e-16
    alpha = ex / den.index_select(0, dst)
    out = torch.zeros((n, heads, C), device=q.device).index_add_(0, dst, alpha[..., None] * vj)
    return out.mean(dim=1) if mean else out.reshape(n, heads * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hops", type=int, default=6)
    ap.add_argument("--resolution", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gencast_probe.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(args.log), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("device: %s" % torch.cuda.get_device_name(0))
    ei_np = khop_edges(args.resolution, args.hops)
    n, E = int(ei_np.max()) + 1, ei_np.shape[1]
    deg = np.bincount(ei_np[1], minlength=n)
    say("mesh resolution %d, %d-hop closure: %d nodes, %d edges, in-degree min %d / median %d / max %d"
        % (args.resolution, args.hops, n, E, deg.min(), int(np.median(deg)), deg.max()))
    ei = torch.from_numpy(ei_np).to(dev)
    plan = gencast.edge_plan(ei, n, n).plan
    rs = np.random.RandomState(1)
    f32 = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731
    latent, heads, cond_dim, edge_dim = 512, 4, 16, 512
    x, cond = f32(n, latent), f32(n, cond_dim)

    for concat in (True, False):
        C = latent // heads if concat else latent
        hc = heads * C
        kind = "concat=True (4 x %d)" % C if concat else "final concat=False (4 x %d, head-mean)" % C
        for with_e in (False, True):
            tag = "%s, %s" % (kind, "edge features" if with_e else "no edge features")
            torch.cuda.empty_cache()
            try:
                ea = f32(E, edge_dim) if with_e else None
                blk = go.fill_(gencast.CondTransformerBlock(latent, C, heads, conditioning_dim=cond_dim, edges_dim=edge_dim if with_e else None,
                                                            concat=concat, activation_layer=torch.nn.ReLU if concat else None), 3).to(dev)

                def fwd():
                    with torch.no_grad():
                        blk(x, ei, ea, cond)

                def fwd_bwd():
                    blk.zero_grad(set_to_none=True)
                    blk(x, ei, ea, cond).sum().backward()

                t_f, t_fb = timings([fwd, fwd_bwd], args.iters, warm=1)
                say("%-64s block forward %s   forward + backward %s" % (tag, fmt(t_f), fmt(t_fb)))
                del blk
                q, k, v = f32(n, hc), f32(n, hc), f32(n, hc)
                e = None
                if with_e:
                    del ea
                    torch.cuda.empty_cache()
                    e = f32(E, hc)
                (t_a,) = timings([lambda: gencast.graph_attention_forward(q, k, v, e, plan, heads, not concat, keep_heads=False)], args.iters, warm=1)
                gb = E * hc * 4 * (3 if with_e else 2) / 1e9
                ms = statistics.median(t_a)
                say("%-64s attention launch %s   %.1f GB of rows read: %.2f TB/s" % ("", fmt(t_a), gb, gb / ms))
                out, out_heads, lse = gencast.graph_attention_forward(q, k, v, e, plan, heads, not concat)
                dout = f32(n, C if not concat else hc)
                (t_b,) = timings([lambda: gencast.graph_attention_backward(q, k, v, e, plan, heads, not concat, out_heads, lse, dout)],
                                 args.iters, warm=1)
                say("%-64s attention backward (two launches) %s" % ("", fmt(t_b)))
                del out, out_heads, lse, dout
                try:
                    with torch.no_grad():
                        (t_c,) = timings([lambda: composition(q, k, v, e, ei[0], ei[1], n, heads, not concat)], max(3, args.iters // 3), warm=1)
                    say("%-64s torch-op composition, forward %s" % ("", fmt(t_c)))
                except torch.OutOfMemoryError:
                    say("%-64s torch-op composition, forward: out of device memory" % "")
                del q, k, v, e
            except torch.OutOfMemoryError:
                say("%-64s out of device memory" % tag)
            flush()
    flush()


if __name__ == "__main__":
    main()
