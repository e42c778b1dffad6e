"""ImageMetaModel cost at the 1 degree shape (B = 2, 78 channels, 180 x 360, patch 4 -> 4 050 tokens of width 1 248; depth 5,
4 heads of 64; csrc/gw_fengwu.hip): the model forward and forward + backward, the attention launch alone (forward, and the
three backward launches), and beside them the restatement's torch-op composition (the reference's own sequence of operations:
LayerNorm, matmul, softmax on materialised scores, GELU) in float32 on the same device.  HIP events, warm-up, then the median of
``--iters`` single-call timings; the log goes to profiles/fengwu_probe.log.

    python scripts/probes/fengwu_probe.py [--iters 10]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import fengwu_ghr as fg  # noqa: E402
from tests import fengwu_oracle as fo  # noqa: E402

PEAK_F32 = 157.3e12  # FLOP/s of v_mfma_f32_16x16x4_f32 on MI355X
CFG = dict(image_size=(180, 360), patch_size=4, depth=5, heads=4, mlp_dim=5, channels=78, dim_head=64)
BATCH = 2


def median_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fengwu_probe.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = fo.fill_(gw.ImageMetaModel(**CFG), 1).to(dev)
    x = fo.image_input(CFG, BATCH, 2).to(dev)
    sd32 = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    n, heads, d = (180 // 4) * (360 // 4), CFG["heads"], CFG["dim_head"]
    inner = heads * d
    flop_attn = 4.0 * BATCH * heads * n * n * d  # the two products of one layer, forward
    say("ImageMetaModel %s, batch %d: %d tokens of width %d, %d (batch, head) pairs" % (CFG, BATCH, n, 78 * 16, BATCH * heads))

    def fwd():
        with torch.no_grad():
            return model(x)

    def fwd_bwd():
        model.zero_grad(set_to_none=True)
        model(x).sum().backward()

    def ref_fwd():
        with torch.no_grad():
            return fo.image_meta_model(sd32, CFG, x)

    def ref_fwd_bwd():
        for v in sd32.values():
            v.grad = None
        fo.image_meta_model(sd32, CFG, x).sum().backward()

    with torch.no_grad():
        a, b = fwd(), ref_fwd()
    say("kernels against the composition: max difference %.3e of the maximum" % ((a - b).abs().max() / b.abs().max()).item())
    t_f, t_fb = median_ms(fwd, args.iters), median_ms(fwd_bwd, args.iters)
    r_f, r_fb = median_ms(ref_fwd, args.iters), median_ms(ref_fwd_bwd, args.iters)
    say("model forward            : kernels %8.2f ms   torch composition %8.2f ms   ratio %.2f" % (t_f, r_f, r_f / t_f))
    say("model forward + backward : kernels %8.2f ms   torch composition %8.2f ms   ratio %.2f" % (t_fb, r_fb, r_fb / t_fb))

    rs = np.random.RandomState(3)
    qkv = torch.from_numpy(rs.standard_normal((BATCH * n, 3 * inner)).astype(np.float32)).to(dev)
    dout = torch.from_numpy(rs.standard_normal((BATCH * n, inner)).astype(np.float32)).to(dev)
    out, lse = fg.attention_forward(qkv, BATCH, heads, n, d, d ** -0.5)
    t_a = median_ms(lambda: fg.attention_forward(qkv, BATCH, heads, n, d, d ** -0.5), args.iters)
    t_ab = median_ms(lambda: fg.attention_backward(qkv, out, lse, dout, BATCH, heads, n, d, d ** -0.5), args.iters)

    def ref_attn(t):
        q, k, v = (c.reshape(BATCH, n, heads, d).permute(0, 2, 1, 3) for c in t.split(inner, dim=-1))
        return fo.attention_core(q, k, v, d ** -0.5).permute(0, 2, 1, 3).reshape(BATCH * n, inner)

    tq = qkv.clone().requires_grad_(True)

    def ref_attn_fb():
        tq.grad = None
        (ref_attn(tq) * dout).sum().backward()

    with torch.no_grad():
        r_a = median_ms(lambda: ref_attn(qkv), args.iters)
    r_afb = median_ms(ref_attn_fb, args.iters)
    say("attention forward        : kernel  %8.3f ms (%.1f TFLOP/s, %.0f%% of the fp32 MFMA peak)   torch composition %8.3f ms   ratio %.2f"
        % (t_a, flop_attn / t_a / 1e9, 100 * flop_attn / (t_a * 1e-3) / PEAK_F32, r_a, r_a / t_a))
    say("attention backward       : kernels %8.3f ms (7 products: %.1f TFLOP/s)   torch composition forward + backward %8.3f ms"
        % (t_ab, 3.5 * flop_attn / t_ab / 1e9, r_afb))
    say("attention fwd + bwd      : kernels %8.3f ms   torch composition %8.3f ms   ratio %.2f" % (t_a + t_ab, r_afb, r_afb / (t_a + t_ab)))
    # the wrappers' window attention: 9 tokens, tens of thousands of pairs
    nw, bw = 9, 2 * n
    qkvw = torch.from_numpy(rs.standard_normal((bw * nw, 3 * inner)).astype(np.float32)).to(dev)
    t_w = median_ms(lambda: fg.attention_forward(qkvw, bw, heads, nw, d, d ** -0.5), args.iters)
    say("window attention forward : kernel  %8.3f ms (%d pairs of %d tokens, %.1f MB read + written)"
        % (t_w, bw * heads, nw, qkvw.numel() * 4 / 3 * 4 / 1e6))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
