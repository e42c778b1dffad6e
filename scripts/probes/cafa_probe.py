"""CaFAForecaster cost at the 1 degree shape (B = 2, 78 -> 78 channels, 180 x 360, downsampling 2 -> 90 x 180 tokens of width
256; depth 6, 8 heads of 64; csrc/gw_cafa.hip and the axial addressing of csrc/gw_fengwu.hip):

  (a) the model forward and forward + backward, and beside them the restatement's torch-op composition (tests/cafa_oracle.py:
      the reference's own sequence of operations, rearranging copies included) in float32 on the same device;
  (b) the axial attention launch for each axis, and beside it the route it replaces: the existing ``attention_forward`` on a
      pre-transposed contiguous copy of the projection, plus the two copies that route needs (qkv in, the output back);
  (c) the patch embed and expand kernels against the bytes they must move.

HIP events around single calls after a warm-up; ``--iters`` repeats, reported as median [minimum .. maximum].  The two
attention routes are timed alternately in the same loop.  The log goes to profiles/cafa_probe.log (``--log`` to change it).

    python scripts/probes/cafa_probe.py [--iters 20]
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
from graph_weather_amd import cafa  # noqa: E402
from graph_weather_amd import fengwu_ghr as fg  # noqa: E402
from tests import cafa_oracle as co  # noqa: E402

PEAK_F32 = 157.3e12  # FLOP/s of v_mfma_f32_16x16x4_f32 on MI355X
PEAK_HBM = 8.0e12    # bytes/s
CFG = dict(input_channels=78, output_channels=78, model_dim=256, downsampling_factor=2, processor_depth=6, num_heads=8, dim_head=64,
           feedforward_multiplier=4)
B, H, W = 2, 180, 360


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timings(fns, iters, warm=3):
    """Per function the list of ``iters`` single-call times in ms; the functions alternate inside one loop."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "cafa_probe.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    f, dim, heads, d = CFG["downsampling_factor"], CFG["model_dim"], CFG["num_heads"], CFG["dim_head"]
    oh, ow = -(-H // f), -(-W // f)
    rows, inner = B * oh * ow, heads * d
    model = co.fill_(gw.CaFAForecaster(**CFG), 1).to(dev)
    x = torch.from_numpy(np.random.RandomState(2).standard_normal((B, CFG["input_channels"], H, W)).astype(np.float32)).to(dev)
    sd32 = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    flop_lin = 2.0 * rows * dim * (2 * (3 * inner + inner) + 2 * CFG["feedforward_multiplier"] * dim)
    flop_h, flop_w = 4.0 * B * ow * heads * oh * oh * d, 4.0 * B * oh * heads * ow * ow * d
    say("CaFAForecaster %s, input [%d, %d, %d, %d]: %d tokens (%d x %d per image) of width %d" % (CFG, B, CFG["input_channels"], H, W, rows, oh, ow, dim))
    say("FLOP per block, forward: Linear %.1f G, height attention %.1f G, width attention %.1f G" % (flop_lin / 1e9, flop_h / 1e9, flop_w / 1e9))

    # ---- (a) the model -------------------------------------------------------------------------------------------------
    def fwd():
        with torch.no_grad():
            return model(x)

    def fwd_bwd():
        model.zero_grad(set_to_none=True)
        model(x).sum().backward()

    def ref_fwd():
        with torch.no_grad():
            return co.forecaster(sd32, x, CFG)

    def ref_fwd_bwd():
        for v in sd32.values():
            v.grad = None
        co.forecaster(sd32, x, CFG).sum().backward()

    with torch.no_grad():
        a, b = fwd(), ref_fwd()
    say("kernels against the composition: max difference %.3e of the maximum" % ((a - b).abs().max() / b.abs().max()).item())
    del a, b
    t_f, r_f = timings([fwd, ref_fwd], args.iters)
    t_fb, r_fb = timings([fwd_bwd, ref_fwd_bwd], args.iters)
    total = CFG["processor_depth"] * (flop_lin + flop_h + flop_w)
    say("(a) model forward            : kernels %s   torch composition %s   ratio of medians %.2f"
        % (fmt(t_f), fmt(r_f), statistics.median(r_f) / statistics.median(t_f)))
    say("    %.0f GFLOP in the blocks -> %.1f TFLOP/s end to end (%.0f%% of the fp32 MFMA peak; a whole-program rate)"
        % (total / 1e9, total / statistics.median(t_f) / 1e9, 100 * total / (statistics.median(t_f) * 1e-3) / PEAK_F32))
    say("(a) model forward + backward : kernels %s   torch composition %s   ratio of medians %.2f"
        % (fmt(t_fb), fmt(r_fb), statistics.median(r_fb) / statistics.median(t_fb)))

    # ---- (b) attention along each axis ---------------------------------------------------------------------------------
    rs = np.random.RandomState(3)
    qkv = torch.from_numpy(rs.standard_normal((rows, 3 * inner)).astype(np.float32)).to(dev)
    dout = torch.from_numpy(rs.standard_normal((rows, inner)).astype(np.float32)).to(dev)
    scale = d ** -0.5
    for axis, name, flop in ((1, "height", flop_h), (2, "width", flop_w)):
        seqs, n = (B * ow, oh) if axis == 1 else (B * oh, ow)

        def axial():
            return cafa.attention_axial_forward(qkv, B, oh, ow, axis, heads, d, scale)

        def copy_route():
            if axis == 1:
                t = qkv.reshape(B, oh, ow, 3 * inner).permute(0, 2, 1, 3).contiguous().reshape(rows, 3 * inner)
                o, _ = fg.attention_forward(t, seqs, heads, n, d, scale)
                return o.reshape(B, ow, oh, inner).permute(0, 2, 1, 3).contiguous()
            return fg.attention_forward(qkv, seqs, heads, n, d, scale)[0]

        def copies_only():
            if axis == 1:
                qkv.reshape(B, oh, ow, 3 * inner).permute(0, 2, 1, 3).contiguous()
                dout.reshape(B, ow, oh, inner).permute(0, 2, 1, 3).contiguous()

        o1, o2 = axial()[0], copy_route().reshape(rows, inner)
        same = torch.equal(o1, o2)
        out, lse = axial()
        t_ax, t_cp, t_c = timings([axial, copy_route, copies_only], args.iters)
        t_b, = timings([lambda: cafa.attention_axial_backward(qkv, out, lse, dout, B, oh, ow, axis, heads, d, scale)], args.iters)
        say("(b) %-6s attention forward : axial launch %s (%.1f TFLOP/s)   existing kernel on a transposed copy + its copies %s"
            "   the copies alone %s   bitwise equal: %s" % (name, fmt(t_ax), flop / statistics.median(t_ax) / 1e9, fmt(t_cp), fmt(t_c), same))
        say("    %-6s attention backward: axial launches %s (7 products: %.1f TFLOP/s); %d sequences of %d tokens, %d heads"
            % (name, fmt(t_b), 3.5 * flop / statistics.median(t_b) / 1e9, seqs, n, heads))

    # ---- (c) the patch kernels -----------------------------------------------------------------------------------------
    enc, dec = model.encoder.encoder, model.decoder.decoder
    C = CFG["input_channels"]
    k = C * f * f
    r2 = torch.from_numpy(rs.standard_normal((rows, dim)).astype(np.float32)).to(dev)
    g_img = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32)).to(dev)
    with torch.no_grad():
        w_e, b_e, w_x, b_x = enc.weight.detach(), enc.bias.detach(), dec.weight.detach(), dec.bias.detach()
        img_bytes, row_bytes, w_bytes = 4.0 * B * C * H * W, 4.0 * rows * dim, 4.0 * dim * k
        flop_p = 2.0 * rows * dim * k
        for name, fn, nbytes, nflop in (
            ("patch embed forward ", lambda: cafa.patch_embed_forward(x, w_e, b_e, f), img_bytes + row_bytes + w_bytes, flop_p),
            ("patch embed backward", lambda: cafa.patch_embed_backward(x, w_e, r2, f), 2 * img_bytes + 2 * row_bytes + 2 * w_bytes, 2 * flop_p),
            ("patch expand forward", lambda: cafa.patch_expand_forward(r2, w_x, b_x, B, H, W, f), img_bytes + row_bytes + w_bytes, flop_p),
            ("patch expand backward", lambda: cafa.patch_expand_backward(r2, w_x, g_img, f), 2 * img_bytes + 2 * row_bytes + 2 * w_bytes,
             2 * flop_p),
        ):
            t, = timings([fn], args.iters)
            med = statistics.median(t) * 1e-3
            say("(c) %s: %s   %.1f MB to move (%.3f ms at the HBM peak), %.1f GFLOP (%.3f ms at the fp32 MFMA peak) -> %.0f GB/s, %.1f TFLOP/s"
                % (name, fmt(t), nbytes / 1e6, nbytes / PEAK_HBM * 1e3, nflop / 1e9, nflop / PEAK_F32 * 1e3, nbytes / med / 1e9,
                   nflop / med / 1e12))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
