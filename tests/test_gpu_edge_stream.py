"""The decoder form of the fp32 edge update (csrc/gw_edge_stream.hip: constants in LDS, no residual stream) against ``edge_kernel`` (csrc/gw_edge.hip) on the same operands - bit for bit: it keeps the weight ring,
the MFMA order and every arithmetic expression - against a float64 restatement, and behind ``AssimilatorDecoder.decode``."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import ops  # noqa: E402
from graph_weather_amd.ops import Operand, PackedMLP  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

DEV = "cuda:0"
FP32_REL = 2e-4  # the bar tests/test_gpu_round2.py applies to edge_kernel's rows against the float64 oracle
ATOMICS_REL = 1e-5  # ... and to atomics against deterministic segment sums (test_deterministic_forward_*)


def _rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


def _mlp(rs):
    dims = [768, 256, 256, 256]
    ws = [torch.from_numpy((rs.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)) for i in range(3)]
    bs = [torch.from_numpy((0.1 * rs.standard_normal(dims[i + 1])).astype(np.float32)) for i in range(3)]
    ln = (torch.from_numpy((1 + 0.1 * rs.standard_normal(256)).astype(np.float32)),
          torch.from_numpy((0.1 * rs.standard_normal(256)).astype(np.float32)))
    return ws, bs, ln


def _tile_local_dst(rs, B, E):
    """Sorted destinations in which no run of equal ids crosses a multiple of 64 of the column index b * E + k of any sample b:
    every destination's edges then fall inside one tile, each aggregate row receives ONE add (onto the zero fill) and the
    result does not depend on the order of atomics.  Ids are skipped at random: destinations without an edge."""
    cuts = {k for b in range(B) for k in range(E) if (b * E + k) % 64 == 0}
    dst, d, left = [], 0, 0
    for k in range(E):
        if left == 0 or k in cuts:
            d += 1 + int(rs.rand() < 0.2)
            left = int(rs.randint(1, 10))
        dst.append(d)
        left -= 1
    return np.asarray(dst, dtype=np.int32)


# name: (batch, edges per sample, projected operands (1: the gathered node products; 2: + the per-edge product, the decoder's
# form), hub)
CASES = {
    "b2_e100": (2, 100, 2, False),            # a tile straddles the sample boundary
    "t3_r0": (1, 64 * 3, 2, False),           # identity tile order
    "t3_r1": (1, 64 * 3 + 1, 1, False),
    "t3_r63": (1, 64 * 3 + 63, 2, False),
    "t67_r0": (1, 64 * 67, 1, False),         # the XCD map is active, with a remainder
    "t67_r1": (1, 64 * 67 + 1, 2, False),
    "t67_r63": (1, 64 * 67 + 63, 2, False),
    "t21": (1, 64 * 21 - 5, 2, False),        # a ragged last tile
    "t600": (2, 64 * 300 - 7, 2, False),      # more tiles than the 512 workgroup slots: the anti-phase start is on
    "hub": (2, 400, 2, True),                 # a destination with 150 edges: partial sums of three tiles meet in atomics
}
BITWISE = [n for n, c in CASES.items() if not c[3]]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the float64 reference and edge_kernel's aggregate (all-zero residual table) of a case; made once."""
    B, E, n_proj, hub = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    ws, bs, ln = _mlp(rs)
    n_src = 37
    if hub:
        dst = np.sort(np.concatenate([np.full(150, 11), rs.randint(0, 60, size=E - 150)])).astype(np.int32)
    else:
        dst = _tile_local_dst(rs, B, E)
    n_dst = int(dst.max()) + 3  # the last rows have no edge either
    src = rs.randint(0, n_src, size=E).astype(np.int32)
    src[0] = n_src - 1
    ps = torch.from_numpy(rs.standard_normal((B * n_src, 256)).astype(np.float32))
    pe = torch.from_numpy(rs.standard_normal((E, 256)).astype(np.float32))  # per-edge product, shared by the batch
    # float64: gather-add -> ReLU -> two layers -> LayerNorm -> segment sum
    st, dt = torch.from_numpy(src).long(), torch.from_numpy(dst).long()
    z = bs[0].double() + ps.double().reshape(B, n_src, 256)[:, st]
    if n_proj == 2:
        z = z + pe.double()[None]
    h = torch.relu(torch.relu(z) @ ws[1].double().T + bs[1].double())
    y = torch.nn.functional.layer_norm(h @ ws[2].double().T + bs[2].double(), (256,), ln[0].double(), ln[1].double(), 1e-5)
    ref = torch.zeros(B, n_dst, 256, dtype=torch.float64)
    ref.index_add_(1, dt, y)
    pm = PackedMLP([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], (ln[0].to(DEV), ln[1].to(DEV)),
                   ((0, 256), (256, 512), (512, 768)), torch.float32)
    args = (pm, B, torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), Operand(ps.to(DEV), n_src, 256, projected=True),
            ops.ZERO, Operand(pe.to(DEV), 0, 256, projected=True) if n_proj == 2 else ops.ZERO)
    agg_old = torch.zeros(B * n_dst, 256, device=DEV)
    ops.edge_update_forward(*args, Operand(torch.zeros(E, 256, device=DEV), 0, 256), n_dst, agg_old, None)
    torch.cuda.synchronize()
    return args, n_dst, ref.reshape(B * n_dst, 256), agg_old.cpu(), dst


def _run_new(name):
    args, n_dst, ref, agg_old, dst = _case(name)
    agg = torch.zeros(args[1] * n_dst, 256, device=DEV)
    ops.edge_update_forward(*args, ops.ZERO, n_dst, agg, None)
    torch.cuda.synchronize()
    return agg.cpu()


@pytest.mark.parametrize("name", BITWISE)
def test_no_residual_kernel_equals_edge_kernel_bit_for_bit(name):
    """Same projected operands and weights; edge_kernel adds an all-zero residual (LN + 0.0 is the same value), the new
    kernel gets none.  Every destination's edges lie inside one tile, so no sum depends on the order of atomics."""
    agg = _run_new(name)
    _, n_dst, _, agg_old, dst = _case(name)
    delta = (agg - agg_old).abs().max().item()
    print(f"{name}: max |new - old| = {delta:.3e}")
    assert delta == 0.0
    rows = agg.reshape(-1, n_dst, 256)
    empty = torch.from_numpy(np.setdiff1d(np.arange(n_dst), dst)).long()
    assert len(empty) >= 2 and bool((rows[:, empty] == 0).all())  # destinations without an edge stay as zero-filled
    assert bool((rows[:, torch.from_numpy(np.unique(dst)).long()].abs().amax(dim=2) > 0).all())  # ... and every other row was written


def test_no_residual_kernel_with_a_hub_spanning_three_tiles():
    """150 edges of one destination: partial sums of three tiles meet in atomics.  Bar: what atomics against deterministic sums
    get in tests/test_gpu_round2.py."""
    agg = _run_new("hub")
    r = _rel(agg, _case("hub")[3])
    print(f"hub: rel(new, old) = {r:.3e}")
    assert r <= ATOMICS_REL


@pytest.mark.parametrize("name", list(CASES))
def test_no_residual_kernel_against_float64(name):
    agg = _run_new(name)
    r = _rel(agg, _case(name)[2])
    print(f"{name}: rel(new, float64) = {r:.3e}")
    assert r <= FP32_REL


def test_launches_the_no_residual_kernel_does_not_take_are_refused():
    """No residual with e' requested, or in deterministic mode: no kernel exists - a loud error, never another route."""
    args, n_dst, _, _, _ = _case("t3_r1")
    B, E = args[1], int(args[2].shape[0])
    agg = torch.zeros(B * n_dst, 256, device=DEV)
    with pytest.raises(RuntimeError, match="without residual"):
        ops.edge_update_forward(*args, ops.ZERO, n_dst, agg, torch.empty(B * E, 256, device=DEV))
    with pytest.raises(RuntimeError, match="without residual"):
        ops.edge_update_forward(*args, ops.ZERO, n_dst, agg, None, deterministic=True)


# ---- behind AssimilatorDecoder.decode -------------------------------------------------------------------------------------


def _forecaster(deg=10.0, seed=0):
    lat_lons = regular_lat_lons(deg)
    model = gw.GraphWeatherForecaster(lat_lons)
    deterministic_fill_(model, seed=seed)
    model = model.to(DEV).eval()
    model.auto_graph = False
    return model, lat_lons


@pytest.fixture
def old_route():
    def force(flag):
        ops.EDGE_STREAM = not flag

    yield force
    ops.EDGE_STREAM = True


def test_decode_with_the_cached_residual_sums_matches_the_per_edge_residual_route(old_route):
    model, lat_lons = _forecaster()
    feats = seeded_features(2, len(lat_lons), 102, seed=4).to(DEV)
    dec = model.decoder
    with torch.no_grad():  # (under autograd the differentiable path keeps the per-edge residual)
        assert dec.stream_path()
        y_new = model(feats)
        assert "dec_e_sum" in dec._cache
        old_route(True)
        assert not dec.stream_path()
        y_old = model(feats)
        old_route(False)
    r = _rel(y_new - feats[..., :78], y_old - feats[..., :78])
    print(f"decode: rel(delta new, delta old) = {r:.3e}")
    assert r <= ATOMICS_REL
    with torch.no_grad():
        model.set_deterministic(True)  # deterministic mode keeps the per-edge residual
        assert not dec.stream_path()
        y_det = model(feats)
    assert _rel(y_new - feats[..., :78], y_det - feats[..., :78]) <= ATOMICS_REL


def test_a_weight_update_rebuilds_the_residual_sum_table():
    """Cold forward (tables rebuilt on the side stream) == warm forward, bitwise: the decoder's sums meet at most two partial
    sums per row (7 edges per grid node), and deterministic mesh blocks fix the rest."""
    model, lat_lons = _forecaster()
    for blk in list(model.encoder.graph_processor.blocks) + list(model.processor.graph_processor.blocks):
        blk.deterministic = True
    feats = seeded_features(2, len(lat_lons), 102, seed=5).to(DEV)
    dec = model.decoder
    with torch.no_grad():
        y0 = model(feats)
        t0 = dec._cache._entries["dec_e_sum"][1]
        for p in dec.parameters():
            p.mul_(1.01)
        y_cold = model(feats)
        t1 = dec._cache._entries["dec_e_sum"][1]
        y_warm = model(feats)
        assert dec._cache._entries["dec_e_sum"][1] is t1
    assert t1 is not t0 and not torch.equal(t1, t0)
    assert not torch.equal(y_cold, y0)
    assert torch.equal(y_cold, y_warm)


def test_hip_graph_replay_of_the_new_route_equals_eager():
    """Fourth call of a shape = second replay of the captured forward.  Mesh blocks deterministic, decoder on the no-residual
    kernel in atomics mode (at most two partial sums per row: order independent) - so equality is bitwise."""
    model, lat_lons = _forecaster()
    for blk in list(model.encoder.graph_processor.blocks) + list(model.processor.graph_processor.blocks):
        blk.deterministic = True
    model.auto_graph = True
    feats = seeded_features(2, len(lat_lons), 102, seed=6).to(DEV)
    with torch.no_grad():
        assert model.decoder.stream_path()
        ref = model._forward_eager(feats)
        ys = [model(feats) for _ in range(4)]
        auto = model.__dict__["_auto"]
        assert auto._fg is not None and auto._fg.captures == 1
    assert torch.equal(ys[3], ref)
