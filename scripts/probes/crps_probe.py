"""EnsembleCRPSLoss on the device beside the torch-op broadcasting composition ``(x[:, :, None] - x[:, None]).abs()``.

Shapes (B, N, lon, lat, C): (2, 4, 360, 181, 83) and (2, 16, 360, 181, 83) - 1 degree, 83 fields, members in registers - and
(2, 32, 360, 181, 83), which is above the register bound and takes the general kernels (a coverage path: the members are re-read
through the cache).  Forward (no_grad) and forward + backward of ``reduction="mean"`` with both weights; wall clock around single
calls with the device synchronised at both ends, ``--iters`` repeats reported as median [minimum .. maximum]; beside it the time
per call of ``--burst`` calls back to back between two device events (no host gap in it) and the algorithmic bytes over that time:
forward ``(B N + B) G C 4`` (every input read once), forward + backward ``(3 B N + 2 B) G C 4`` (both inputs read twice, dpred
written).  The composition runs on the same device and inputs with its allocation peak, and is skipped with a printed reason where
its temporaries would not fit.  Every shape is recorded, faster or not.  The log goes to profiles/crps_probe.log (``--log`` to
change it).  Nothing is gated on these numbers.

    python scripts/probes/crps_probe.py [--iters 10] [--burst 20]
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

from graph_weather_amd import EnsembleCRPSLoss, ops  # noqa: E402

SHAPES = [(2, 4, 360, 181, 83), (2, 16, 360, 181, 83), (2, 2 * ops.CRPS_REGISTER_MEMBERS, 360, 181, 83)]


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timings(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    return [_time(fn) for _ in range(iters)]


def burst(fn, calls):
    """ms per call of ``calls`` calls back to back between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def fmt(ts):
    return "%8.3f ms [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))


def peak(fn, clear):
    """MiB allocated at the highest point of one call above what was resident before it (``clear`` drops the last call's gradient)."""
    fn()
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    high = torch.cuda.max_memory_allocated()
    clear()
    return (high - base) / 2 ** 20


def composition(pred, target, aw, fw, alpha=1.0):
    n = pred.shape[1]
    c2 = alpha / (2.0 * n * (n - 1)) + (1.0 - alpha) / (2.0 * n * n)
    v = (pred - target[:, None]).abs().sum(1) / n - c2 * (pred[:, :, None] - pred[:, None]).abs().sum((1, 2))
    return (v * aw[None, None, :, None] * fw).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "crps_probe.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crps_probe: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = ["crps_probe: %s, EnsembleCRPSLoss(grid_lat, features_weights, alpha=1, reduction='mean'); wall clock with the device "
             "synchronised at both ends, median of %d [minimum .. maximum]; 'burst': ms per call of %d calls back to back between two "
             "device events, GB/s = algorithmic bytes over the burst time" % (torch.cuda.get_device_name(0), args.iters, args.burst)]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(5)
    for B, N, nlon, nlat, nvar in SHAPES:
        pred = torch.randn((B, N, nlon, nlat, nvar), device=dev, generator=gen)
        target = torch.randn((B, nlon, nlat, nvar), device=dev, generator=gen)
        lat = torch.linspace(-90.0, 90.0, nlat)
        fw = torch.from_numpy(np.random.RandomState(3).uniform(0.25, 2.0, nvar).astype(np.float32))
        crit = EnsembleCRPSLoss(grid_lat=lat, features_weights=fw).to(dev)
        leaf = pred.clone().requires_grad_(True)
        elements = B * nlon * nlat * nvar
        bytes_f, bytes_fb = 4.0 * elements * (N + 1), 4.0 * elements * (3 * N + 2)
        path = "registers" if N <= ops.CRPS_REGISTER_MEMBERS else "general kernels"

        def k_fwd():
            with torch.no_grad():
                return crit(pred, target)

        def k_train():
            leaf.grad = None
            crit(leaf, target).backward()

        def t_fwd():
            with torch.no_grad():
                return composition(pred, target, crit.area_weights, crit.features_weights)

        def t_train():
            leaf.grad = None
            composition(leaf, target, crit.area_weights, crit.features_weights).backward()

        def clear():
            leaf.grad = None

        head = "B %d N %d %d x %d x %d (%s)" % (B, N, nlon, nlat, nvar, path)
        free = torch.cuda.mem_get_info()[0]
        pairs = 4.0 * elements * N * N
        need = 4 * pairs  # the differences, their absolute values, and the two the backward keeps or forms beside them
        run_torch = need < 0.8 * free
        if not run_torch:
            lines.append("%s: torch-op composition skipped: its [B, N, N, lon, lat, C] temporaries are %.1f GB each and about four "
                         "are alive in forward + backward; %.1f GB are free" % (head, pairs / 1e9, free / 1e9))
            print(lines[-1], flush=True)
        for what, kern, comp, nbytes in (("forward", k_fwd, t_fwd, bytes_f), ("forward + backward", k_train, t_train, bytes_fb)):
            ts = timings(kern, args.iters)
            per = burst(kern, args.burst)
            line = ("%s %-18s kernels %s  burst %.3f ms = %.0f GB/s of %.1f MB  peak %.1f MiB"
                    % (head, what, fmt(ts), per, nbytes / per / 1e6, nbytes / 1e6, peak(kern, clear)))
            if run_torch:
                try:
                    tt = timings(comp, args.iters, warm=2)
                    ratio = statistics.median(tt) / statistics.median(ts)
                    line += ("  |  torch ops %s  peak %.1f MiB  torch / kernels %.2f (%s)"
                             % (fmt(tt), peak(comp, clear), ratio, "kernels faster" if ratio > 1.0 else "KERNELS NOT FASTER"))
                except torch.cuda.OutOfMemoryError:
                    leaf.grad = None
                    torch.cuda.empty_cache()
                    line += "  |  torch ops: out of memory (%.1f GB were free), not timed" % (free / 1e9)
            print(line, flush=True)
            lines.append(line)
        if run_torch:
            try:
                lines.append("%s: loss kernels %.7f, torch ops %.7f" % (head, k_fwd().item(), t_fwd().item()))
                print(lines[-1], flush=True)
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
        del pred, target, leaf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
