"""The forward bench.py times, at the size and on the path it times, against the fp64 oracle on the device.

``c2`` (the headline): 1 degree, batch 2, one input buffer passed call after call - from the third call on
``graphed.AutoGraph`` pins that buffer and replays one HIP graph whose mesh stack runs on two streams (``routes.mesh_streams``).
``c4``'s per-GPU shard: 1 degree, batch 8 (211 MB of input, above ``AutoGraph.MAX_INPUT_BYTES``): eager.  Compared on the polar +
random row sample of tests/test_gpu_split.py, as the delta of the forecast from its input (the decoder residual), at the fp32
tests' bar (2e-4 of the delta scale) in fp32 and in bf16x3."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import routes  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

from . import oracle_gpu  # noqa: E402
from .test_gpu_split import X3_REL, _row_sample  # noqa: E402

DEV = "cuda:0"
FP32_REL = 2e-4  # of the decoder-delta scale (tests/test_gpu_round2.py)
BARS = {"fp32": FP32_REL, "bf16x3": X3_REL}


def _model(precision, seed=0):
    lat_lons = regular_lat_lons(1.0)
    model = gw.GraphWeatherForecaster(lat_lons, resolution=2)  # bench.py build_model(CONFIGS["c2"])
    deterministic_fill_(model, seed=seed)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = model.encoder.graphs.as_oracle_dict()
    model = model.to(DEV).eval()
    if precision != "fp32":
        model.set_compute_dtype(gw.BF16X3)
    return model, lat_lons, sd, g


class Oracle:
    """fp64 oracle forecasts on the device, kept as [B, rows, 78] on the host for the row sample only."""

    def __init__(self, sd, g, rows):
        self.sd, self.g, self.rows = sd, g, rows

    def __call__(self, feats):
        y = oracle_gpu.forecast(self.sd, self.g, feats, DEV)[:, self.rows.to(DEV)].cpu()
        torch.cuda.empty_cache()
        return y


def _err(y, ref, feats, rows):
    """max |y - ref| / max |ref - x| on the sampled rows (the decoder-delta scale), y on the device, ref on the host."""
    start = feats[:, rows, :78].double().cpu()
    ys = y[:, rows.to(y.device)].double().cpu()
    return ((ys - ref.double()).abs().max() / (ref.double() - start).abs().max()).item()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_bench_loop_replays_one_pinned_graph_against_the_oracle(precision):
    """bench.py time_forward on c2, exactly: five calls of model(buf) on one buffer - calls 3 to 5 replay ONE capture that reads
    the buffer in place.  Then the buffer's contents change under the pinned graph, then five fresh tensors (the path where the
    graph copies each input into its own buffer): every output against the oracle for its own input."""
    t0 = time.perf_counter()
    model, lat_lons, sd, g = _model(precision)
    G = len(lat_lons)
    rows = _row_sample(lat_lons, 1500, seed=1)
    oracle = Oracle(sd, g, rows)
    bar = BARS[precision]
    feats = seeded_features(2, G, 102, seed=42)  # the bench's input
    other = seeded_features(2, G, 102, seed=7)
    fresh = [seeded_features(2, G, 102, seed=100 + i) for i in range(5)]
    refs = [oracle(x) for x in [feats, other] + fresh]
    assert routes.mesh_streams(0, [torch.float32 if precision == "fp32" else gw.BF16X3], 2) == 2  # two-stream mesh stack

    buf = feats.to(DEV)
    with torch.no_grad():
        outs = [model(buf) for _ in range(5)]
        auto = model._auto
        fg = auto._fg
        assert fg is not None and fg.captures == 1 and fg.pinned, "calls 3-5 must replay one capture on the pinned buffer"
        assert fg.input.data_ptr() == buf.data_ptr()
        e5 = _err(outs[4], refs[0], feats, rows)
        e_first = _err(outs[0], refs[0], feats, rows)  # the eager call, same bar
        # the buffer's contents change under the pinned graph
        buf.copy_(other.to(DEV))
        y6 = model(buf)
        assert fg.captures == 1 and fg.pinned
        e6 = _err(y6, refs[1], other, rows)
        moved = _err(outs[4], refs[1], other, rows)  # the previous output, judged as a forecast of the new input
        # fresh tensors, all kept alive (no two share an address): the graph goes back to its own buffer and copies each in
        xs = [x.to(DEV) for x in fresh]
        assert len({x.data_ptr() for x in xs} | {buf.data_ptr()}) == 6
        ys = [model(x) for x in xs]
        assert fg.captures == 2 and not fg.pinned
        e_fresh = [_err(y, r, x, rows) for y, r, x in zip(ys, refs[2:], fresh)]
    torch.cuda.synchronize()
    print(f"[bench forward {precision}] c2 1deg B=2, {rows.numel()} rows: call 1 (eager) {e_first:.2e}, call 5 (pinned replay) "
          f"{e5:.2e}; buffer rewritten: {e6:.2e} (previous output vs the new oracle {moved:.2e}); fresh tensors "
          f"{', '.join(f'{e:.2e}' for e in e_fresh)}; bar {bar:.0e}; peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB, "
          f"{time.perf_counter() - t0:.0f} s")
    assert e_first <= bar and e5 <= bar
    assert e6 <= bar
    assert moved > 100 * bar, "the rewritten buffer must change the forecast by far more than the bar"
    assert max(e_fresh) <= bar


def test_deterministic_replay_equals_the_eager_forward_bitwise():
    """set_deterministic(True), fp32, c2: the replayed forecast (mesh stack on two streams) is bitwise the eager forward's."""
    model, lat_lons, sd, g = _model("fp32")
    model.set_deterministic(True)
    buf = seeded_features(2, len(lat_lons), 102, seed=42).to(DEV)
    with torch.no_grad():
        for _ in range(5):
            y = model(buf)
        fg = model._auto._fg
        assert fg is not None and fg.captures == 1 and fg.pinned
        y_eager = model._forward_eager(buf)
    torch.cuda.synchronize()
    n_diff = (y != y_eager).sum().item()
    print(f"[bench forward deterministic] replay vs eager: {n_diff} elements differ")
    assert torch.equal(y, y_eager)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_c4_shard_batch8_stays_eager_against_the_oracle(precision):
    """c4's per-GPU shard (1 degree, batch 8): input above AutoGraph.MAX_INPUT_BYTES, so every call is eager; samples 0 and 7 (the
    two ends of every batch walk) against the oracle."""
    t0 = time.perf_counter()
    model, lat_lons, sd, g = _model(precision)
    rows = _row_sample(lat_lons, 1500, seed=1)
    feats = seeded_features(8, len(lat_lons), 102, seed=42)
    ref = Oracle(sd, g, rows)(feats[[0, 7]])
    fd = feats.to(DEV)
    with torch.no_grad():
        for _ in range(3):
            y = model(fd)
        auto = model.__dict__.get("_auto")
        assert auto is not None and not auto.usable(fd) and auto._fg is None, "batch 8 at 1 degree must stay eager"
    e = _err(y[[0, 7]], ref, feats[[0, 7]], rows)
    print(f"[bench forward c4 shard {precision}] 1deg B=8, samples 0 and 7: {e:.2e} (bar {BARS[precision]:.0e}); input "
          f"{fd.numel() * 4 / 2**20:.0f} MiB; {time.perf_counter() - t0:.0f} s")
    assert e <= BARS[precision]
