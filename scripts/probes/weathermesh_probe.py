"""WeatherMesh's processor on the device: the neighbourhood attention of csrc/gw_na3d.hip and a 10-layer ``WeatherMeshProcessor``
beside (a) the only earlier route to the same numbers - ``sparse_attention_forward`` / ``_backward`` of
graph_weather_amd/gencast_sparse.py on the explicit neighbourhood mask (one entry per (token, key): 245 per token at the default
kernel), plan and head-major rows prepared outside the timed region - and (b) a torch-op formulation: the keys and values of every
window gathered with ``index_select`` one depth plane of queries at a time, ``einsum``, ``softmax``, ``einsum`` (the gathered
tensors of a whole volume at the larger shape would be 2 x 57 GB).

Shapes (tokens B, D, H, W; channels; heads; kernel):
    small   (1, 6, 32, 64),   C = 64,  8 heads, kernel (5, 7, 7)
    large   (1, 14, 90, 180), C = 256, 8 heads, kernel (5, 7, 7)  - a 0.25 degree grid after three halvings; illustrative, the
                                                                    reference publishes no size
Routes run on the same device and inputs, alternating inside one loop after a warm-up; wall clock around single calls with the
device synchronised at both ends; ``--iters`` repeats reported as median [minimum .. maximum].  The 10-layer processor of route (b)
is timed at the small shape only.  Run one shape per invocation under a time limit of its own:

    timeout -k 10 300 python scripts/probes/weathermesh_probe.py --shape small
    timeout -k 10 900 python scripts/probes/weathermesh_probe.py --shape large --append

The log goes to profiles/weathermesh_probe.log (``--log`` to change it).  Nothing is gated on these numbers.
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

from graph_weather_amd import gencast_sparse, weathermesh  # noqa: E402
from graph_weather_amd.gencast import _Linear  # noqa: E402
from tests import weathermesh_oracle as wo  # noqa: E402
from tests.cafa_oracle import fill_  # noqa: E402

SHAPES = {"small": ((1, 6, 32, 64), 64, 8, (5, 7, 7)), "large": ((1, 14, 90, 180), 256, 8, (5, 7, 7))}


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
    return "%10.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def torch_na3d(qkv, idx, shape, nh, dh, scale):
    """Route (b): qkv [rows, 3 C] -> out [rows, C]; idx [rows, window] the neighbour table; one depth plane of queries at a time."""
    B, D, H, W = shape
    C, plane = nh * dh, H * W
    q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(-1, nh, dh) for i in range(3))
    outs = []
    for z in range(B * D):
        rows = slice(z * plane, (z + 1) * plane)
        nb = idx[rows].reshape(-1)
        kn = k.index_select(0, nb).view(plane, -1, nh, dh)
        vn = v.index_select(0, nb).view(plane, -1, nh, dh)
        p = torch.softmax(torch.einsum("nhd,nwhd->nhw", q[rows] * scale, kn), dim=-1)
        outs.append(torch.einsum("nhw,nwhd->nhd", p, vn).reshape(plane, C))
    return torch.cat(outs)


def torch_na3d_train(qkv, dout, idx, shape, nh, dh, scale):
    """Forward and backward of route (b), one plane of queries at a time so that one plane's gathered keys are alive at once."""
    B, D, H, W = shape
    C, plane = nh * dh, H * W
    leaf = qkv.detach().requires_grad_(True)
    q, k, v = (leaf[:, i * C:(i + 1) * C].reshape(-1, nh, dh) for i in range(3))
    for z in range(B * D):
        rows = slice(z * plane, (z + 1) * plane)
        nb = idx[rows].reshape(-1)
        kn = k.index_select(0, nb).view(plane, -1, nh, dh)
        vn = v.index_select(0, nb).view(plane, -1, nh, dh)
        p = torch.softmax(torch.einsum("nhd,nwhd->nhw", q[rows] * scale, kn), dim=-1)
        (torch.einsum("nhw,nwhd->nhd", p, vn).reshape(plane, C) * dout[rows]).sum().backward()
    return leaf.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="small")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "weathermesh_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weathermesh_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    shape, C, nh, kernel = SHAPES[args.shape]
    B, D, H, W = shape
    rows, dh, win = B * D * H * W, C // nh, kernel[0] * kernel[1] * kernel[2]
    scale = dh ** -0.5
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("weathermesh_probe: %s, tokens %s = %d, C %d, %d heads x %d, kernel %s (%d keys per token), wall clock with the device "
        "synchronised at both ends, median of %d [minimum .. maximum]" % (torch.cuda.get_device_name(0), shape, rows, C, nh, dh, kernel, win, args.iters))
    assert B == 1
    idx = wo.neighbour_table((D, H, W), kernel).to(dev)  # [rows, window]
    ei = torch.stack([torch.arange(rows, device=dev).repeat_interleave(win), idx.reshape(-1)])
    plan = gencast_sparse.sparse_plan(ei, rows).plan  # the mask's plan: built once, outside every timed region
    g = torch.Generator(device="cpu").manual_seed(1)
    qkv = torch.randn(rows, 3 * C, generator=g).to(dev)
    dout = torch.randn(rows, C, generator=g).to(dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]

    # ---- the attention alone ---------------------------------------------------------------------------------------------------
    out, lse = weathermesh.na3d_forward(q, k, v, shape, kernel, nh, scale)
    out_a, lse_a = gencast_sparse.sparse_attention_forward(q, k, v, plan, nh, scale, 1)
    out_b = torch_na3d(qkv, idx, shape, nh, dh, scale)
    top = out.abs().max().item()
    say("attention output, largest difference: to (a) %.3e, to (b) %.3e (maximum %.3e)"
        % ((out - out_a).abs().max().item(), (out - out_b).abs().max().item(), top))
    gr = weathermesh.na3d_backward(q, k, v, shape, kernel, nh, scale, out, lse, dout, stacked=True)[3]
    gr_a = gencast_sparse.sparse_attention_backward(q, k, v, plan, nh, scale, 1, out_a, lse_a, dout, stacked=True)[3]
    gr_b = torch_na3d_train(qkv, dout, idx, shape, nh, dh, scale)
    say("attention gradient [dq dk dv], largest difference: to (a) %.3e, to (b) %.3e (maximum %.3e)"
        % ((gr - gr_a).abs().max().item(), (gr - gr_b).abs().max().item(), gr.abs().max().item()))
    del out_b, gr_b
    fns = [lambda: weathermesh.na3d_forward(q, k, v, shape, kernel, nh, scale),
           lambda: gencast_sparse.sparse_attention_forward(q, k, v, plan, nh, scale, 1),
           lambda: torch_na3d(qkv, idx, shape, nh, dh, scale),
           lambda: weathermesh.na3d_backward(q, k, v, shape, kernel, nh, scale, out, lse, dout, stacked=True),
           lambda: gencast_sparse.sparse_attention_backward(q, k, v, plan, nh, scale, 1, out_a, lse_a, dout, stacked=True),
           lambda: torch_na3d_train(qkv, dout, idx, shape, nh, dh, scale)]
    ts = timings(fns, args.iters)
    med = [statistics.median(t) for t in ts]
    say("attention forward            gw_na3d              %s" % fmt(ts[0]))
    say("attention forward            (a) sparse kernels   %s  time ratio to gw_na3d %.2f" % (fmt(ts[1]), med[1] / med[0]))
    say("attention forward            (b) torch ops        %s  time ratio to gw_na3d %.2f" % (fmt(ts[2]), med[2] / med[0]))
    say("attention backward           gw_na3d              %s" % fmt(ts[3]))
    say("attention backward           (a) sparse kernels   %s  time ratio to gw_na3d %.2f" % (fmt(ts[4]), med[4] / med[3]))
    say("attention forward + backward (b) torch ops        %s  time ratio to gw_na3d forward + backward %.2f"
        % (fmt(ts[5]), med[5] / (med[0] + med[3])))
    flops = 4.0 * rows * win * C  # q . k and p v: 2 multiply-adds per (token, key, channel)
    say("attention forward: %.2f GFLOP algorithmic, %.2f TFLOP/s in gw_na3d (whole call)" % (flops / 1e9, flops / 1e12 / (med[0] * 1e-3)))

    # ---- the processor ---------------------------------------------------------------------------------------------------------
    proc = fill_(weathermesh.WeatherMeshProcessor(C, n_layers=args.layers, kernel=kernel, num_heads=nh), 2).to(dev).eval()
    x = torch.randn(B, D, H, W, C, generator=g).to(dev)

    def composed(attend):
        def run(xx):
            t = xx.reshape(-1, C)
            for layer in proc.layers:
                t = _Linear.apply(attend(_Linear.apply(t, layer.qkv.weight, layer.qkv.bias, False)), layer.proj.weight, layer.proj.bias, False)
            return t.view(xx.shape)
        return run

    routes = {"gw_na3d": proc,
              "(a) sparse kernels": composed(lambda t: gencast_sparse._SparseAttentionStacked.apply(t, plan, nh, scale, 1))}
    if args.shape == "small":
        routes["(b) torch ops"] = composed(lambda t: torch_na3d(t, idx, shape, nh, dh, scale))

    def eval_(fn):
        def run():
            with torch.no_grad():
                return fn(x)
        return run

    def train(fn):
        def run():
            proc.zero_grad(set_to_none=True)
            xx = x.clone().requires_grad_(True)
            fn(xx).square().mean().backward()
        return run

    outs = {n: eval_(fn)() for n, fn in routes.items()}
    for n in list(routes)[1:]:
        say("%d-layer processor output, largest difference of gw_na3d to %s: %.3e (maximum %.3e)"
            % (args.layers, n, (outs["gw_na3d"] - outs[n]).abs().max().item(), outs["gw_na3d"].abs().max().item()))
    for what, make in (("forward", eval_), ("forward + backward", train)):
        ts = dict(zip(routes, timings([make(fn) for fn in routes.values()], args.iters)))
        base = statistics.median(ts["gw_na3d"])
        for n in routes:
            say("%d-layer processor %-18s %-20s %s%s" % (args.layers, what, n, fmt(ts[n]),
                                                        "" if n == "gw_na3d" else "  time ratio to gw_na3d %.2f" % (statistics.median(ts[n]) / base)))
    if args.shape != "small":
        say("%d-layer processor, (b) torch ops: not measured at this shape" % args.layers)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
