"""The fp32 encoder stage in one launch (csrc/gw_encoder_fused.hip: ``encfused_kernel``) against the two launches it replaces
on the same operands - ``ops.mlp_forward`` (node encoder, ``chain_kernel``) followed by ``ops.edge_update_forward``
(``elds_kernel``) - bit for bit: it keeps their summation order and every arithmetic expression; against a float64
restatement; and behind ``Encoder.encode``."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import ops  # noqa: E402
from graph_weather_amd.ops import Operand, PackedMLP, SavedActivations  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

DEV = "cuda:0"
FP32_REL = 2e-4  # the project's bar for fp32 kernels against float64 (tests/test_gpu_edge_lds.py)
ATOMICS_REL = 1e-5  # ... and for sums whose order differs (atomics against deterministic segment sums)
SPLITS = ((0, 256), (256, 512), (512, 768))
LD = 320  # leading dimension of the product tables that are wider than their 256 features
K_FEAT = 102
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


def _mlp(rs, k_in):
    """Biases, gamma - 1 and beta of size 0.1: a constant read from the wrong LDS slot is far outside every bar."""
    dims = [k_in, 256, 256, 256]
    ws = [torch.from_numpy((rs.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)) for i in range(3)]
    bs = [torch.from_numpy((0.1 * rs.standard_normal(256)).astype(np.float32)) for _ in range(3)]
    ln = (torch.from_numpy((1 + 0.1 * rs.standard_normal(256)).astype(np.float32)),
          torch.from_numpy((0.1 * rs.standard_normal(256)).astype(np.float32)))
    return ws, bs, ln


def _tile_local_dst(rs, B, E):
    """Sorted destinations in which no run of equal ids crosses a multiple of 64 of the column index b * E + k of any sample b:
    each aggregate row then receives ONE add onto its zero fill.  Ids are skipped at random: destinations without an edge."""
    cuts = {k for b in range(B) for k in range(E) if (b * E + k) % 64 == 0}
    dst, d, left = [], 0, 0
    for k in range(E):
        if left == 0 or k in cuts:
            d += 1 + int(rs.rand() < 0.2)
            left = int(rs.randint(1, 10))
        dst.append(d)
        left -= 1
    return np.asarray(dst, dtype=np.int32)


def _table(rs, rows, ld=256, k=256):
    """[rows, ld] with k features per row; the padding columns of a wider table hold 1e3 (never to be read)."""
    t = torch.full((rows, ld), 1e3, dtype=torch.float32)
    t[:, :k] = torch.from_numpy(rs.standard_normal((rows, k)).astype(np.float32))
    return t


def _f64_mlp(x, ws, bs, ln):
    h = torch.relu(x @ ws[0].double().T + bs[0].double())
    h = torch.relu(h @ ws[1].double().T + bs[1].double())
    return torch.nn.functional.layer_norm(h @ ws[2].double().T + bs[2].double(), (256,), ln[0].double(), ln[1].double(), 1e-5)


# (batch, grid rows = edges per sample)
SHAPES = {
    "b2_e100": (2, 100),             # a tile straddles the sample boundary
    "t3_r0": (1, 192),               # identity tile order
    "t3_r1": (1, 193),               # ... ragged last tile
    "t3_r63": (1, 255),
    "t67_r1": (1, 64 * 67 + 1),      # the XCD map is active, with a remainder
    "t600": (2, 64 * 300 - 7),       # more tiles than the 512 workgroup slots: the anti-phase start is on
}
HUB = (2, 400)  # a destination with 150 edges: partial sums of three tiles meet in atomics


@functools.lru_cache(maxsize=None)
def _case(nproj, B, G, feat_ld, hub=False, src_kind="perm"):
    """Operands of one stage (on the device, never changed) and the float64 restatement of its aggregate with and without
    residual.  nproj 2: P_d[dst] (shared by the batch, 256 wide) and the per-edge product (ld 320); nproj 1: the latter alone."""
    rs = np.random.RandomState(1000 * nproj + 7 * B + G + feat_ld + 3 * hub + len(src_kind))
    nw, nb, nln = _mlp(rs, K_FEAT)
    ew, eb, eln = _mlp(rs, 768)
    if hub:
        dst = np.sort(np.concatenate([np.full(150, 11), rs.randint(0, 60, size=G - 150)])).astype(np.int32)
    else:
        dst = _tile_local_dst(rs, B, G)
    n_dst = int(dst.max()) + 3  # the last rows have no edge either
    src = rs.permutation(G).astype(np.int32)
    if src_kind == "repeat":  # a grid row read by several edges (and rows read by none)
        src[5:9] = src[4]
    feats = _table(rs, B * G, feat_ld, K_FEAT)
    pd = _table(rs, n_dst) if nproj == 2 else None
    pe = _table(rs, G, LD)
    res = _table(rs, G)
    st, dt = torch.from_numpy(src).long(), torch.from_numpy(dst).long()
    xg = _f64_mlp(feats[:, :K_FEAT].double(), nw, nb, nln).reshape(B, G, 256)[:, st]
    z = eb[0].double() + xg @ ew[0][:, :256].double().T + pe[:, :256].double()[None]
    if nproj == 2:
        z = z + pd.double()[dt][None]
    h = torch.relu(z)
    h = torch.relu(h @ ew[1].double().T + eb[1].double())
    y = torch.nn.functional.layer_norm(h @ ew[2].double().T + eb[2].double(), (256,), eln[0].double(), eln[1].double(), 1e-5)
    ref_nores = torch.zeros(B, n_dst, 256, dtype=torch.float64).index_add_(1, dt, y).reshape(B * n_dst, 256)
    ref_res = torch.zeros(B, n_dst, 256, dtype=torch.float64).index_add_(1, dt, y + res.double()[None]).reshape(B * n_dst, 256)
    pm_n = PackedMLP([w.to(DEV) for w in nw], [b.to(DEV) for b in nb], (nln[0].to(DEV), nln[1].to(DEV)), ((0, K_FEAT),), torch.float32)
    pm_e = PackedMLP([w.to(DEV) for w in ew], [b.to(DEV) for b in eb], (eln[0].to(DEV), eln[1].to(DEV)), SPLITS, torch.float32)
    assert pm_n.w1[0].numel() == 28 * 1024  # the first layer is packed in 28 K-steps: what the kernel's short chunk reads
    dev = dict(src=torch.from_numpy(src).to(DEV), dst=torch.from_numpy(dst).to(DEV), feats=feats.to(DEV),
               pd=None if pd is None else pd.to(DEV), pe=pe.to(DEV), res=res.to(DEV), zero_res=torch.zeros(G, 256, device=DEV))
    return dict(pm_n=pm_n, pm_e=pm_e, B=B, G=G, n_dst=n_dst, dst_np=dst, ref_nores=ref_nores, ref_res=ref_res, **dev)


def _operands(c):
    feats = Operand(c["feats"], c["G"], K_FEAT)
    x_dst = ops.ZERO if c["pd"] is None else Operand(c["pd"], 0, 256, projected=True)
    return feats, x_dst, Operand(c["pe"], 0, 256, projected=True)


def _fused(c, res, **kw):
    feats, x_dst, e_in = _operands(c)
    agg = torch.zeros(c["B"] * c["n_dst"], 256, device=DEV)
    ops.encoder_fused_forward(c["pm_n"], c["pm_e"], c["B"], c["src"], c["dst"], feats, x_dst, e_in,
                              Operand(c["res"], 0, 256) if res else ops.ZERO, c["n_dst"], agg, **kw)
    torch.cuda.synchronize()
    return agg.cpu()


def _two_launches(c, res_table, node_save=None, **kw):
    feats, x_dst, e_in = _operands(c)
    B, G = c["B"], c["G"]
    xg = ops.mlp_forward(c["pm_n"], feats, B * G, G, save=node_save)
    agg = torch.zeros(B * c["n_dst"], 256, device=DEV)
    ops.edge_update_forward(c["pm_e"], B, c["src"], c["dst"], Operand(xg, G, 256), x_dst, e_in, Operand(res_table, 0, 256),
                            c["n_dst"], agg, None, **kw)
    torch.cuda.synchronize()
    return agg.cpu()


CASES = [(n, s, ld) for n in (2, 1) for s in SHAPES for ld in (K_FEAT, 107)]


@pytest.mark.parametrize("nproj,shape,feat_ld", CASES, ids=[f"p{n}-{s}-ld{ld}" for n, s, ld in CASES])
def test_one_launch_equals_the_two_launches_bit_for_bit(nproj, shape, feat_ld):
    """Every destination's edges lie inside one tile, so no sum depends on the order of atomics.  With the residual the
    aggregate is the two launches' bits; without it, their bits on an all-zero residual table.  Rows without an edge stay zero.
    (ld 102: 8-byte pairs; ld 107: rows at odd addresses, single floats.)"""
    c = _case(nproj, *SHAPES[shape], feat_ld)
    for res in (True, False):
        agg = _fused(c, res)
        old = _two_launches(c, c["res"] if res else c["zero_res"])
        d = (agg - old).abs().max().item()
        r = _rel(agg, c["ref_res" if res else "ref_nores"])
        print(f"p{nproj} {shape} ld{feat_ld} res={res}: max |new - old| = {d:.3e}, rel(new, float64) = {r:.3e}")
        assert torch.equal(agg, old)
        assert r <= FP32_REL
        rows = agg.reshape(c["B"], c["n_dst"], 256)
        empty = torch.from_numpy(np.setdiff1d(np.arange(c["n_dst"]), c["dst_np"])).long()
        assert len(empty) >= 2 and bool((rows[:, empty] == 0).all())
        assert bool((rows[:, torch.from_numpy(np.unique(c["dst_np"])).long()].abs().amax(dim=2) > 0).all())


@pytest.mark.parametrize("nproj", [2, 1])
def test_one_launch_with_a_hub_spanning_three_tiles(nproj):
    """150 edges of one destination: partial sums of three tiles meet in atomics - against deterministic segment sums."""
    c = _case(nproj, *HUB, K_FEAT, True)
    for res in (True, False):
        agg = _fused(c, res)
        det = _two_launches(c, c["res"] if res else c["zero_res"], deterministic=True)
        r, r64 = _rel(agg, det), _rel(agg, c["ref_res" if res else "ref_nores"])
        print(f"p{nproj} hub res={res}: rel(new, deterministic) = {r:.3e}, rel(new, float64) = {r64:.3e}")
        assert r <= ATOMICS_REL
        assert r64 <= FP32_REL


def test_a_repeated_source_row_is_encoded_per_edge():
    """The result does not depend on src being a permutation."""
    c = _case(2, 2, 100, K_FEAT, False, "repeat")
    for res in (True, False):
        agg = _fused(c, res)
        assert torch.equal(agg, _two_launches(c, c["res"] if res else c["zero_res"]))
        assert _rel(agg, c["ref_res" if res else "ref_nores"]) <= FP32_REL


@pytest.mark.parametrize("route", ["save", "deterministic"])
def test_launches_the_fused_kernel_refuses_keep_the_two_launches(route):
    """Activation saving and deterministic segment sums are not the fused kernel's: the entry point refuses them loudly, and
    the two launches take them as before."""
    c = _case(2, 2, 100, K_FEAT)
    n = c["B"] * c["G"]
    with pytest.raises(RuntimeError, match="inference in atomics mode"):
        if route == "save":
            _fused(c, True, save=SavedActivations(c["pm_e"], n, DEV))
        else:
            _fused(c, True, deterministic=True)
    if route == "save":
        agg = _two_launches(c, c["res"], node_save=SavedActivations(c["pm_n"], n, DEV), save=SavedActivations(c["pm_e"], n, DEV))
    else:
        agg = _two_launches(c, c["res"], deterministic=True)
    r = _rel(agg, c["ref_res"])
    print(f"{route}: rel(two launches, float64) = {r:.3e}")
    assert r <= FP32_REL


# ---- behind Encoder.encode ------------------------------------------------------------------------------------------------


def _forecaster(deg=10.0, seed=0):
    lat_lons = regular_lat_lons(deg)
    model = gw.GraphWeatherForecaster(lat_lons)
    deterministic_fill_(model, seed=seed)
    model = model.to(DEV).eval()
    model.auto_graph = False
    return model, lat_lons


@pytest.fixture
def two_launches():
    def force(flag):
        ops.ENCODER_FUSED = not flag

    yield force
    ops.ENCODER_FUSED = True


def _count_fused(monkeypatch):
    calls = []
    real = ops.encoder_fused_forward
    monkeypatch.setattr(ops, "encoder_fused_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_encode_on_the_fused_route_matches_the_two_launches_and_the_golden(two_launches, monkeypatch):
    model, lat_lons = _forecaster()
    enc = model.encoder
    feats = seeded_features(2, len(lat_lons), 102, seed=42).to(DEV)  # (the inputs of tests/golden/forecaster_10deg_b2.npz)
    first = model.processor.graph_processor.blocks[0].edge_model.edge_mlp.packed()
    post_w = [first.w1[0], first.w1[1]]
    calls = _count_fused(monkeypatch)
    with torch.no_grad():
        assert enc.fused_path(feats)
        x_new = enc.encode(feats)
        xp_new, posts_new, agg0_new = enc.encode(feats, post_w=post_w)
        assert len(calls) == 2 and "enc_proj_team" in enc._cache
        two_launches(True)
        assert not enc.fused_path(feats)
        x_old = enc.encode(feats)
        xp_old, posts_old, agg0_old = enc.encode(feats, post_w=post_w)
        assert len(calls) == 2
        two_launches(False)
        enc.graph_processor.blocks[0].deterministic = True  # deterministic mode keeps the two launches
        assert not enc.fused_path(feats)
        x_det = enc.encode(feats)
        assert len(calls) == 2
    torch.cuda.synchronize()
    assert torch.equal(x_new, xp_new) and torch.equal(x_old, xp_old)
    for name, a, b in (("mesh rows", x_new, x_old), ("mesh rows (deterministic)", x_new, x_det), ("post product 0", posts_new[0], posts_old[0]),
                       ("post product 1", posts_new[1], posts_old[1])):
        r = _rel(a, b)
        print(f"encode: rel({name} new, old) = {r:.3e}")
        assert r <= ATOMICS_REL
    assert bool((agg0_new == 0).all()) and bool((agg0_old == 0).all()) and agg0_new.shape == agg0_old.shape
    g = np.load(os.path.join(GOLDEN, "forecaster_10deg_b2.npz"))
    r = _rel(x_new[::37], torch.from_numpy(g["enc_x_rows"]))
    print(f"encode: rel(mesh rows, golden) = {r:.3e}")
    assert r <= FP32_REL
    with torch.enable_grad():  # under autograd the differentiable path keeps the two launches
        model.train()
        assert not enc.fused_path(feats)


def test_hip_graph_replay_of_the_fused_route_equals_eager(two_launches):
    """Fourth call of a shape = second replay of the captured forward = the first call, bit for bit: every block but the
    encoder's is deterministic, and on the 10 degree grid (648 edges onto 5 882 mesh rows) at most two partial sums meet in an
    aggregate row of the encoder, so the order of its atomics does not show.  And the forecast is the two-launch route's."""
    model, lat_lons = _forecaster()
    for blk in list(model.processor.graph_processor.blocks) + list(model.decoder.graph_processor.blocks):
        blk.deterministic = True
    model.auto_graph = True
    feats = seeded_features(2, len(lat_lons), 102, seed=6).to(DEV)
    with torch.no_grad():
        assert model.encoder.fused_path(feats)
        ys = [model(feats).clone() for _ in range(4)]
        auto = model.__dict__["_auto"]
        assert auto._fg is not None and auto._fg.captures == 1
        two_launches(True)
        y_old = model._forward_eager(feats)
        two_launches(False)
    assert torch.equal(ys[3], ys[0])
    r = _rel(ys[3] - feats[..., :78], y_old - feats[..., :78])
    print(f"replay: rel(delta fused, delta two launches) = {r:.3e}")
    assert r <= ATOMICS_REL


def test_a_weight_update_rebuilds_the_cached_residual_sum_product(two_launches):
    """... and the forward after it matches a fresh model with the same weights, on the fused route and on the two launches."""
    from graph_weather_amd.optim import _bump_versions

    model, lat_lons = _forecaster()
    enc = model.encoder
    feats = seeded_features(2, len(lat_lons), 102, seed=5).to(DEV)
    with torch.no_grad():
        x0 = enc.encode(feats)
        t0 = enc._cache._entries["enc_proj_team"][1]
        for p in enc.parameters():
            p.mul_(1.01)
        _bump_versions(list(enc.parameters()))
        x1 = enc.encode(feats)
        t1 = enc._cache._entries["enc_proj_team"][1]
        fresh, _ = _forecaster()
        fresh.encoder.load_state_dict(enc.state_dict())
        x_fresh = fresh.encoder.encode(feats)
        two_launches(True)
        x_fresh_old = fresh.encoder.encode(feats)
        two_launches(False)
    assert t1 is not t0 and not torch.equal(t1, t0)
    assert not torch.equal(x1, x0)
    r, r_old = _rel(x1, x_fresh), _rel(x1, x_fresh_old)
    print(f"after the update: rel(model, fresh model) = {r:.3e}, rel(model, fresh model on two launches) = {r_old:.3e}")
    assert r <= ATOMICS_REL and r_old <= ATOMICS_REL
