"""WeatherMesh's convolution towers on the device: one 3-D ``ConvDownBlock``, one 3-D ``ConvUpBlock``, the encoder and the decoder
(csrc/gw_convnd.hip), forward and forward + backward in training mode, beside the BASELINE: the same modules' children called as
torch's own GPU operations (``nn.Conv2d/3d``, ``nn.BatchNorm2d/3d``, ``F.gelu``, ``F.interpolate``, ``torch.cat``) - the torch-only
restatement on the same card, not the code under test.  The attention layers of the encoder and decoder are this package's in
both routes (torch has no such operation).

Shape (illustrative; the reference publishes none): surface [1, 8, 128, 256], pressure [1, 6, 13, 128, 256], hidden_dim 32, three
blocks a side, latent [1, 14, 16, 32, 256], kernel (5, 7, 7), 8 heads.  The blocks are the second of the encoder's pressure path,
``ConvDownBlock(64, 128, stride=(1, 2, 2), is_3d=True)`` on [1, 64, 13, 64, 128], and the second of the decoder's,
``ConvUpBlock(128, 64, is_3d=True)`` on [1, 128, 13, 32, 64].

Routes alternate inside one loop after a warm-up (the first calls load code objects and let the convolution library pick
algorithms); wall clock around single calls with the device synchronised at both ends; medians of ``--iters`` (7) with minimum
and maximum; the peak allocation of one forward + backward per route.  Where a torch operation does not run on the machine the
probe says so and reports ours alone.  Run under a time limit of its own:

    timeout -k 10 900 python scripts/probes/weathermesh_model_probe.py

The log goes to profiles/weathermesh_model_probe.log (``--log`` to change it).  Nothing is gated on these numbers.
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from graph_weather_amd import weathermesh_model as wm  # noqa: E402
from tests.weathermesh_model_oracle import fill_model_  # noqa: E402

HIDDEN, BLOCKS, LATENT, KERNEL, HEADS = 32, 3, 256, (5, 7, 7), 8


def torch_block(block, x):
    """A block's children as torch operations."""
    up = isinstance(block, wm.ConvUpBlock)
    if up:
        x = F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear", align_corners=False) if block.is_3d else \
            F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    skip, bn_skip = (block.upsample, block.bn_up) if up else (block.downsample, block.bn_down)
    identity = bn_skip(skip(x))
    out = F.gelu(block.bn1(block.conv1(x)))
    return F.gelu(block.bn2(block.conv2(out)) + identity)


def torch_encoder(enc, surface, pressure):
    for block in enc.surface_path:
        surface = torch_block(block, surface)
    for block in enc.pressure_path:
        pressure = torch_block(block, pressure)
    latent = enc.to_latent(torch.cat([pressure, surface.unsqueeze(2)], dim=2)).permute(0, 2, 3, 4, 1).contiguous()
    for layer in enc.transformer_layers:
        latent = layer(latent)
    return latent


def torch_decoder(dec, latent):
    for layer in dec.transformer_layers:
        latent = layer(latent)
    features = dec.split(latent.permute(0, 4, 1, 2, 3))
    pressure, surface = features[:, :, :-1], features[:, :, -1]
    for block in dec.pressure_path:
        pressure = torch_block(block, pressure)
    for block in dec.surface_path:
        surface = torch_block(block, surface)
    return surface, pressure


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def probe(say, what, module, ours, theirs, inputs, iters):
    """ours / theirs: (module, *inputs) -> a tensor or a tuple of tensors."""
    base = copy.deepcopy(module)  # its own running buffers
    leaves = [t.clone().requires_grad_(True) for t in inputs]

    def total(out):
        return sum(o.sum() for o in out) if isinstance(out, tuple) else out.sum()

    def forward(fn, m):
        with torch.no_grad():
            return fn(m, *inputs)

    def both(fn, m):
        m.zero_grad(set_to_none=True)
        for t in leaves:
            t.grad = None
        total(fn(m, *leaves)).backward()

    routes = [("ours", ours, module)]
    try:
        both(theirs, base)
        torch.cuda.synchronize()
        routes.append(("torch", theirs, base))
    except Exception as e:  # the baseline is reported as absent, never silently replaced
        say("%s: the torch operations do not run here (%s: %s); ours alone" % (what, type(e).__name__, str(e).splitlines()[0][:120]))
    if len(routes) == 2:
        a, b = forward(ours, module), forward(theirs, base)
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        say("%s: largest difference of the outputs between the routes %.3e (maximum %.3e)"
            % (what, max((s - t).abs().max().item() for s, t in zip(a, b)), max(t.abs().max().item() for t in b)))
    fwd = timings([lambda f=f, m=m: forward(f, m) for _, f, m in routes], iters)
    bwd = timings([lambda f=f, m=m: both(f, m) for _, f, m in routes], iters)
    peaks = [peak(lambda f=f, m=m: both(f, m)) for _, f, m in routes]
    for (name, _, _), tf, tb, pk in zip(routes, fwd, bwd, peaks):
        say("%-28s %-6s forward %s   forward + backward %s   peak allocation %9.1f MiB" % (what, name, fmt(tf), fmt(tb), pk))
    if len(routes) == 2:
        say("%-28s ours / torch: forward %.2f, forward + backward %.2f, peak allocation %.2f"
            % (what, statistics.median(fwd[0]) / statistics.median(fwd[1]), statistics.median(bwd[0]) / statistics.median(bwd[1]),
               peaks[0] / peaks[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "weathermesh_model_probe.log"))
    ap.add_argument("--scale", type=int, default=1, help="divide height and width by this (rehearsals)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    log = open(args.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    H, W = 128 // args.scale, 256 // args.scale
    rs = np.random.RandomState(0)
    rand = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)  # noqa: E731
    say("device %s, torch %s, iters %d, surface [1, 8, %d, %d], pressure [1, 6, 13, %d, %d]" % (torch.cuda.get_device_name(0),
                                                                                              torch.__version__, args.iters, H, W, H, W))
    block = lambda m, x: m(x)  # noqa: E731
    down = fill_model_(wm.ConvDownBlock(2 * HIDDEN, 4 * HIDDEN, stride=(1, 2, 2), is_3d=True), 1).to(dev).train()
    probe(say, "ConvDownBlock 3-D 64->128", down, block, torch_block, [rand(1, 2 * HIDDEN, 13, H // 2, W // 2)], args.iters)
    up = fill_model_(wm.ConvUpBlock(4 * HIDDEN, 2 * HIDDEN, is_3d=True), 2).to(dev).train()
    probe(say, "ConvUpBlock 3-D 128->64", up, block, torch_block, [rand(1, 4 * HIDDEN, 13, H // 8, W // 8)], args.iters)
    enc = fill_model_(wm.WeatherMeshEncoder(8, 6, LATENT, 13, BLOCKS, HIDDEN, KERNEL, HEADS, 3), 3).to(dev).train()
    probe(say, "WeatherMeshEncoder", enc, lambda m, s, p: m(s, p), torch_encoder, [rand(1, 8, H, W), rand(1, 6, 13, H, W)], args.iters)
    dec = fill_model_(wm.WeatherMeshDecoder(LATENT, 8, 6, BLOCKS, HIDDEN, KERNEL, HEADS, 3), 4).to(dev).train()
    probe(say, "WeatherMeshDecoder", dec, lambda m, x: m(x), torch_decoder, [rand(1, 14, H // 8, W // 8, LATENT)], args.iters)
    log.close()


if __name__ == "__main__":
    main()
