"""StochasticDecompositionLayer and FiLMApplier cost (csrc/gw_modulate.hip) at the forecaster's two activation shapes,
(2, 78, 180, 360) and (2, 256, 5882): forward and forward + backward, each beside the reference's composition executed as
torch ops on the same device (randn_like, two broadcast multiplies and an add; a multiply and an add).  HIP events around
every call, median of --iters calls; before each timed call a 2 GB device copy runs, so that the call is enqueued while the
GPU is still busy (the events then bracket GPU work, not launch latency) and finds nothing of its operands in the caches.
Every line gives the time, the bytes the fused kernels have to move and the fraction of 6.3 TB/s that is.

    python scripts/probes/modulation_probe.py [--iters 20] [--out profiles/modulation_probe.log]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import graph_weather_amd as gw  # noqa: E402

STREAM_BW = 6.3e12  # bytes/s a streaming kernel reaches on MI355X
SHAPES = [(2, 78, 180, 360), (2, 256, 5882)]
LATENT_DIM, NUM_LEAD_TIMES, HIDDEN = 32, 40, 64


def timed(fn, iters, flush, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        flush[1].copy_(flush[0])
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)  # us


def reference_sdl(layer, x, z):
    """stochastic_decomposition.py:56-68 as torch ops."""
    epsilon = torch.randn_like(x)
    style = F.linear(z, layer.style_net.weight, layer.style_net.bias)
    shape = tuple(x.shape[:2]) + (1,) * (x.dim() - 2)
    return x + (layer.alpha.reshape((1, -1) + (1,) * (x.dim() - 2)) * style.reshape(shape) * epsilon)


def reference_film(x, gamma, beta):
    """film.py:72-75 as torch ops."""
    shape = tuple(x.shape[:2]) + (1,) * (x.dim() - 2)
    return x * gamma.reshape(shape) + beta.reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modulation_probe.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flush = (torch.empty(1 << 30, dtype=torch.uint8, device=dev), torch.empty(1 << 30, dtype=torch.uint8, device=dev))
    lines = [f"median of {args.iters} calls, HIP events, caches flushed before each call; times in us; bytes = what the fused kernels move"]

    def report(what, shape, t_hip, t_ref, byt):
        lines.append(f"{what:22s} {str(shape):20s} hip {t_hip:8.1f} us  {byt / 1e6:7.1f} MB  {byt / (t_hip * 1e-6) / 1e12:5.2f} TB/s "
                     f"({100 * byt / (t_hip * 1e-6) / STREAM_BW:5.1f} % of 6.3)   torch ops {t_ref:8.1f} us   ratio {t_hip / t_ref:5.2f}")
        print(lines[-1], flush=True)

    for shape in SHAPES:
        n = 1
        for s in shape:
            n *= s
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g).to(dev)
        dy = torch.randn(shape, generator=g).to(dev)
        z = torch.randn(shape[0], LATENT_DIM, generator=g).to(dev)
        layer = gw.StochasticDecompositionLayer(shape[1], LATENT_DIM).to(dev)
        with torch.no_grad():
            layer.alpha.fill_(0.5)
        params = tuple(layer.parameters())
        with torch.no_grad():
            t_hip = timed(lambda: layer(x, z), args.iters, flush)
            t_ref = timed(lambda: reference_sdl(layer, x, z), args.iters, flush)
        report("sdl forward", shape, t_hip, t_ref, 8 * n)
        xg, zg = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
        t_hip = timed(lambda: torch.autograd.grad(layer(xg, zg), (xg, zg) + params, dy), args.iters, flush)
        t_ref = timed(lambda: torch.autograd.grad(reference_sdl(layer, xg, zg), (xg, zg) + params, dy), args.iters, flush)
        report("sdl forward+backward", shape, t_hip, t_ref, 12 * n)  # the backward reads dy; dx is dy itself

        gen = gw.FiLMGenerator(NUM_LEAD_TIMES, HIDDEN, shape[1]).to(dev)
        with torch.no_grad():
            gamma, beta = (t.contiguous() for t in gen(shape[0], 3))
        film = gw.FiLMApplier()
        with torch.no_grad():
            t_hip = timed(lambda: film(x, gamma, beta), args.iters, flush)
            t_ref = timed(lambda: reference_film(x, gamma, beta), args.iters, flush)
        report("film forward", shape, t_hip, t_ref, 8 * n)
        gg, bg = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        t_hip = timed(lambda: torch.autograd.grad(film(xg, gg, bg), (xg, gg, bg), dy), args.iters, flush)
        t_ref = timed(lambda: torch.autograd.grad(reference_film(xg, gg, bg), (xg, gg, bg), dy), args.iters, flush)
        report("film forward+backward", shape, t_hip, t_ref, 20 * n)  # the backward reads dy and x and writes dx
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
