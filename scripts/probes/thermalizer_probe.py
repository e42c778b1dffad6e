"""Kernel time of the thermalizer (csrc/gw_thermal.hip), forward and backward, for the three cases of the issue:
1 degree B=2 (simple_net on a (1, 11 764) strip, F=256), B=5 (UNet, 170 x 173, F=256) and 181 x 360 (UNet, F=80; F=78 is refused
by GroupNorm(8, 78) as in the reference).  Run under ``rocprofv3 --kernel-trace --stats -d DIR -o thermal -- python
scripts/probes/thermalizer_probe.py``; the script itself prints wall times of the same calls."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import graph_weather_amd as gw  # noqa: E402
from tests import thermal_oracle as to  # noqa: E402

DEV = torch.device("cuda:0")
CASES = [("1deg_B2_simple", 1, 11764, 256), ("B5_unet_170x173", 170, 173, 256), ("181x360_unet_F80", 181, 360, 80)]


def main(reps: int = 5):
    for name, H, W, F in CASES:
        layer = to.fill_(gw.ThermalizerLayer(F), 1).to(DEV)
        x = torch.randn(H * W, F, device=DEV, requires_grad=True)
        g = torch.randn(H * W, F, device=DEV)
        for _ in range(2):
            layer(x, 500, height=H, width=W).backward(g)
        torch.cuda.synchronize()
        tf = tb = 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            y = layer(x, 500, height=H, width=W)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            y.backward(g)
            torch.cuda.synchronize()
            tf += t1 - t0
            tb += time.perf_counter() - t1
        print("%-18s forward %8.3f ms  backward %8.3f ms (wall, mean of %d)" % (name, 1e3 * tf / reps, 1e3 * tb / reps, reps),
              flush=True)


if __name__ == "__main__":
    main()
