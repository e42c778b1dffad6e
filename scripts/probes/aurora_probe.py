"""Aurora cost on the device, every new kernel beside the torch-op composition it replaces (tests/aurora_oracle.py: the
reference's own sequence of operations in float32 on the same device):

  (a) AuroraModel at N = 1024 points, latent 256, 4 layers (5 -> 3 features): forward, and forward + backward;
  (b) EarthSystemLoss at N = 1024 and N = 10000 with C = 3 on a 3 degree lattice: forward, and forward + backward.  The torch
      composition materialises [N, N, C] differences: 36 MB per temporary at N = 1024, 1.2 GB at N = 10000;
  (c) Swin3DEncoder(1, 96) and Decoder3D(1, 96, (16, 16, 16)) at 16^3 voxels, B = 1: forward, and the convolutions alone beside
      torch's conv3d / conv_transpose3d;
  (d) masked attention (B = 2, 8 heads of 32, n = 1024, a quarter of the keys dropped) beside the unmasked launch, and the token
      mean beside torch.mean.

HIP events around single calls after a warm-up; ``--iters`` repeats, reported as median [minimum .. maximum]; the two routes of
a pair alternate inside one loop.  The log goes to profiles/aurora_probe.log (``--log`` to change it).  Nothing is gated on
these numbers.

    python scripts/probes/aurora_probe.py [--iters 10]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import aurora  # noqa: E402
from graph_weather_amd import fengwu_ghr as fg  # noqa: E402
from tests import aurora_oracle as ao  # noqa: E402


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


def lattice(n_lon, n_lat, seed):
    rs = np.random.RandomState(seed)
    lon, lat = np.meshgrid((np.arange(n_lon) - (n_lon - 1) / 2) * 3.0, (np.arange(n_lat) - (n_lat - 1) / 2) * 1.5, indexing="ij")
    return (np.stack([lon.ravel(), lat.ravel()], axis=-1) + rs.uniform(-0.1, 0.1, (n_lon * n_lat, 2))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "aurora_probe.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def pair(what, ours, theirs):
        t_ours, t_theirs = timings([ours, theirs], args.iters)
        say("%-46s HIP %s   torch ops %s" % (what, fmt(t_ours), fmt(t_theirs)))

    rs = np.random.RandomState(1)
    f32 = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731
    say("device: %s" % torch.cuda.get_device_name(0))

    # (a) the point model
    n = 1024
    cfg = dict(input_features=5, output_features=3, latent_dim=256, num_layers=4)
    model = ao.fill_(gw.AuroraModel(**cfg), 1).to(dev).train()
    p32 = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    pts = torch.from_numpy(lattice(32, 32, 2)[None]).to(dev)
    feats = f32(1, n, 5)

    def ours_fb():
        model.zero_grad(set_to_none=True)
        model(pts, feats).sum().backward()

    def theirs_fb():
        for v in p32.values():
            v.grad = None
        ao.aurora_model(p32, pts, feats, None, cfg).sum().backward()

    with torch.no_grad():
        pair("AuroraModel N 1024 latent 256 x 4, forward", lambda: model(pts, feats), lambda: ao.aurora_model(p32, pts, feats, None, cfg))
    pair("AuroraModel, forward + backward", ours_fb, theirs_fb)

    # (b) the loss
    loss = gw.EarthSystemLoss()
    for n_lon, n_lat in ((32, 32), (100, 100)):
        n = n_lon * n_lat
        q = torch.from_numpy(lattice(n_lon, n_lat, 3)[None]).to(dev)
        pred = (250.0 + 200.0 * f32(1, n, 3)).requires_grad_(True)
        target = pred.detach() + 5.0 * f32(1, n, 3)

        def ours_f():
            with torch.no_grad():
                loss(pred, target, q)

        def ours_fb():
            pred.grad = None
            loss(pred, target, q)["total_loss"].backward()

        def theirs_f():
            with torch.no_grad():
                ao.earth_loss(pred, target, q, 0.5, 0.3, 0.2)

        def theirs_fb():
            pred.grad = None
            ao.earth_loss(pred, target, q, 0.5, 0.3, 0.2)["total_loss"].backward()

        pair("EarthSystemLoss N %d C 3, forward" % n, ours_f, theirs_f)
        pair("EarthSystemLoss N %d C 3, forward + backward" % n, ours_fb, theirs_fb)

    # (c) the volume models
    swin = ao.fill_(gw.Swin3DEncoder(1, 96), 4).to(dev).eval()
    sp = {k: v.detach().clone() for k, v in swin.state_dict().items()}
    vol = f32(1, 1, 16, 16, 16)
    dec = ao.fill_(gw.Decoder3D(1, 96, (16, 16, 16)), 5).to(dev).eval()
    dp = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    lat = f32(1, 4096, 96)
    with torch.no_grad():
        pair("Swin3DEncoder(1, 96) 16^3, forward", lambda: swin(vol), lambda: ao.swin_encoder(sp, vol))
        pair("  Conv3d 1 -> 96 alone (channels-last rows)", lambda: swin.convolution_rows(vol),
             lambda: F.conv3d(vol, sp["conv1.weight"], sp["conv1.bias"], padding=1).permute(0, 2, 3, 4, 1).contiguous())
        pair("Decoder3D(1, 96) 16^3, forward", lambda: dec(lat), lambda: ao.decoder3d(dp, lat, dict(embed_dim=96, target_shape=(16, 16, 16))))

    # (d) masked attention and the token mean
    B, heads, d, n = 2, 8, 32, 1024
    qkv = f32(B * n, 3 * heads * d)
    bias = torch.zeros(B, n, device=dev)
    bias[:, 3 * n // 4:] = float("-inf")
    t_m, t_u = timings([lambda: aurora.attention_masked_forward(qkv, bias, B, heads, n, d, d ** -0.5),
                        lambda: fg.attention_forward(qkv, B, heads, n, d, d ** -0.5)], args.iters)
    say("%-46s masked %s   unmasked %s" % ("attention forward B 2, 8 x 32, n 1024", fmt(t_m), fmt(t_u)))
    rows = f32(B * n, 512)
    pair("token mean [2 x 1024, 512]", lambda: aurora.token_mean_forward(rows, B, n), lambda: rows.reshape(B, n, 512).mean(dim=1))

    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
