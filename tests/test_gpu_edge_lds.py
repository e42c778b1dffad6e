"""The inference form of the fp32 edge update with the constants in LDS (csrc/gw_edge_lds.hip: ``elds_kernel``) against
``edge_kernel`` (csrc/gw_edge.hip) on the same operands - bit for bit: it keeps the tile map, the weight ring, the MFMA order and
every arithmetic expression - and against a float64 restatement.  ``edge_kernel`` is reached through ``deterministic=True``, a
route the new kernel does not take."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from graph_weather_amd import ops  # noqa: E402
from graph_weather_amd.ops import Operand, PackedMLP, SavedActivations  # noqa: E402

DEV = "cuda:0"
FP32_REL = 2e-4  # the bar tests/test_gpu_round2.py applies to edge_kernel's rows against the float64 oracle
ATOMICS_REL = 1e-5  # ... and to atomics against deterministic segment sums (test_deterministic_forward_*)
SPLITS = ((0, 256), (256, 512), (512, 768))
LD = 320  # leading dimension of the tables that are wider than their 256 features
N_SRC = 37


def _rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


def _mlp(rs, n_mid=1):
    """Biases, gamma - 1 and beta of size 0.1: a constant read from the wrong LDS offset is far outside every bar."""
    dims = [768] + [256] * (n_mid + 2)
    n = len(dims) - 1
    ws = [torch.from_numpy((rs.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)) for i in range(n)]
    bs = [torch.from_numpy((0.1 * rs.standard_normal(dims[i + 1])).astype(np.float32)) for i in range(n)]
    ln = (torch.from_numpy((1 + 0.1 * rs.standard_normal(256)).astype(np.float32)),
          torch.from_numpy((0.1 * rs.standard_normal(256)).astype(np.float32)))
    return ws, bs, ln


def _tile_local_dst(rs, B, E):
    """Sorted destinations in which no run of equal ids crosses a multiple of 64 of the column index b * E + k of any sample b:
    every destination's edges then fall inside one tile, each aggregate row receives ONE add onto its zero fill in atomics mode
    and one plain store in deterministic mode.  Ids are skipped at random: destinations without an edge."""
    cuts = {k for b in range(B) for k in range(E) if (b * E + k) % 64 == 0}
    dst, d, left = [], 0, 0
    for k in range(E):
        if left == 0 or k in cuts:
            d += 1 + int(rs.rand() < 0.2)
            left = int(rs.randint(1, 10))
        dst.append(d)
        left -= 1
    return np.asarray(dst, dtype=np.int32)


def _table(rs, rows, ld=256):
    """[rows, ld] with 256 features per row; the padding columns of a wider table hold 1e3 (never to be read)."""
    t = torch.full((rows, ld), 1e3, dtype=torch.float32)
    t[:, :256] = torch.from_numpy(rs.standard_normal((rows, 256)).astype(np.float32))
    return t


def _rows(t, B, per_batch, index):
    """float64 [B, len(index), 256]: rows ``index`` of every sample's part of a table (per_batch == 0: shared by the batch)."""
    t = t[:, :256].double()
    if per_batch == 0:
        return t[index][None].expand(B, -1, -1)
    return t.reshape(B, per_batch, 256)[:, index]


# form: which operand is raw (None: none) and which operands are present, as (x_src, x_dst, e_in)
FORMS = {
    "processor": (2, (True, True, True)),   # elds_kernel<true, 2>: raw e (row k, per sample), P_s[src], P_d[dst]; residual = e
    "encoder2": (0, (True, True, True)),    # elds_kernel<true, 2>: raw x_src[src], P_d[dst], a per-edge product shared by the batch
    "encoder1": (0, (True, False, True)),   # elds_kernel<true, 1>: raw x_src[src], the per-edge product
    "block0": (None, (True, True, True)),   # elds_kernel<false, 3>: three products, per-sample residual
}
# (batch, edges per sample)
SHAPES = {
    "b2_e100": (2, 100),             # a tile straddles the sample boundary
    "t3_r0": (1, 192),               # identity tile order
    "t3_r1": (1, 193),               # ... ragged last tile
    "t3_r63": (1, 255),
    "t67_r1": (1, 64 * 67 + 1),      # the XCD map is active, with a remainder
    "t600": (2, 64 * 300 - 7),       # more tiles than the 512 workgroup slots: the anti-phase start is on
}
HUB = (2, 400)  # a destination with 150 edges: partial sums of three tiles meet in atomics


def _build(form, B, E, hub, seed, n_mid=1):
    """Operands of one launch (on the device) and the float64 restatement of e' and of its segment sums."""
    raw_pos, present = FORMS[form]
    rs = np.random.RandomState(seed)
    ws, bs, ln = _mlp(rs, n_mid)
    if hub:
        dst = np.sort(np.concatenate([np.full(150, 11), rs.randint(0, 60, size=E - 150)])).astype(np.int32)
    else:
        dst = _tile_local_dst(rs, B, E)
    n_dst = int(dst.max()) + 3  # the last rows have no edge either
    src = rs.randint(0, N_SRC, size=E).astype(np.int32)
    src[0] = N_SRC - 1
    st, dt, kt = torch.from_numpy(src).long(), torch.from_numpy(dst).long(), torch.arange(E)
    index = (st, dt, kt)
    # tables: node tables per sample; the per-edge table per sample in the processor (it is the residual too), else batch-shared
    per_batch = [N_SRC, n_dst, E if form == "processor" else 0]
    lds_ = [256, 256, LD]
    if form == "encoder1":
        lds_[0] = LD
    tabs = [_table(rs, B * per_batch[i] if per_batch[i] else E, lds_[i]) if present[i] else None for i in range(3)]
    if form == "processor":
        res, res_pb = tabs[2], E
    elif form == "block0":
        res, res_pb = _table(rs, B * E, LD), E
    else:
        res, res_pb = _table(rs, E), 0
    # float64: layer 1 (the raw product + the gathered products), the further layers, LayerNorm, residual, index_add_
    z = bs[0].double()[None, None].expand(B, E, 256).clone()
    for i in range(3):
        if not present[i]:
            continue
        rows = _rows(tabs[i], B, per_batch[i], index[i])
        z = z + (rows @ ws[0][:, SPLITS[i][0]:SPLITS[i][1]].double().T if i == raw_pos else rows)
    h = torch.relu(z)
    for l in range(1, n_mid + 1):
        h = torch.relu(h @ ws[l].double().T + bs[l].double())
    y = torch.nn.functional.layer_norm(h @ ws[-1].double().T + bs[-1].double(), (256,), ln[0].double(), ln[1].double(), 1e-5)
    e_ref = y + _rows(res, B, res_pb, kt)
    agg_ref = torch.zeros(B, n_dst, 256, dtype=torch.float64)
    agg_ref.index_add_(1, dt, e_ref)
    pm = PackedMLP([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], (ln[0].to(DEV), ln[1].to(DEV)), SPLITS, torch.float32)
    dev_tabs = {id(t): t.to(DEV) for t in tabs + [res] if t is not None}  # (the processor's residual IS its raw table)
    opnds = [Operand(dev_tabs[id(tabs[i])], per_batch[i], 256, projected=i != raw_pos) if present[i] else ops.ZERO for i in range(3)]
    args = (pm, B, torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), *opnds, Operand(dev_tabs[id(res)], res_pb, 256), n_dst)
    return args, dst, e_ref.reshape(B * E, 256), agg_ref.reshape(B * n_dst, 256)


def _run(args, with_e_out=True, **kw):
    B, E, n_dst = args[1], int(args[2].shape[0]), args[-1]
    agg = torch.zeros(B * n_dst, 256, device=DEV)
    e_out = torch.full((B * E, 256), float("nan"), device=DEV) if with_e_out else None
    ops.edge_update_forward(*args, agg, e_out, **kw)
    torch.cuda.synchronize()
    return agg.cpu(), None if e_out is None else e_out.cpu()


def _seed(*names):
    return sum(map(ord, "".join(names)))


CASES = [(f, s, True) for f in FORMS for s in SHAPES] + [(f, s, False) for f in FORMS for s in ("b2_e100", "t3_r1")]


@pytest.mark.parametrize("form,shape,with_e_out", CASES, ids=[f"{f}-{s}-{'e' if w else 'noe'}" for f, s, w in CASES])
def test_constants_in_lds_kernel_equals_edge_kernel_bit_for_bit(form, shape, with_e_out):
    """Every destination's edges lie inside one tile, so no sum depends on the order of atomics: agg and e' are edge_kernel's
    bits (deterministic route), rows without an edge stay zero, and both agree with float64."""
    B, E = SHAPES[shape]
    args, dst, e_ref, agg_ref = _build(form, B, E, False, _seed(form, shape))
    n_dst = args[-1]
    agg_old, e_old = _run(args, deterministic=True)
    agg, e_out = _run(args, with_e_out)
    d_agg = (agg - agg_old).abs().max().item()
    print(f"{form} {shape}: max |agg new - old| = {d_agg:.3e}")
    assert d_agg == 0.0
    if with_e_out:
        d_e = (e_out - e_old).abs().max().item()
        print(f"{form} {shape}: max |e' new - old| = {d_e:.3e}")
        assert d_e == 0.0
    rows = agg.reshape(B, n_dst, 256)
    empty = torch.from_numpy(np.setdiff1d(np.arange(n_dst), dst)).long()
    assert len(empty) >= 2 and bool((rows[:, empty] == 0).all())  # destinations without an edge stay as zero-filled
    assert bool((rows[:, torch.from_numpy(np.unique(dst)).long()].abs().amax(dim=2) > 0).all())  # ... and every other row was written
    r_agg = _rel(agg, agg_ref)
    print(f"{form} {shape}: rel(agg, float64) = {r_agg:.3e}")
    assert r_agg <= FP32_REL
    if with_e_out:
        r_e = _rel(e_out, e_ref)
        print(f"{form} {shape}: rel(e', float64) = {r_e:.3e}")
        assert r_e <= FP32_REL


@pytest.mark.parametrize("form", list(FORMS))
def test_constants_in_lds_kernel_with_a_hub_spanning_three_tiles(form):
    """150 edges of one destination: partial sums of three tiles meet in atomics.  e' is bitwise; the sums get the bar atomics
    against deterministic sums get in tests/test_gpu_round2.py."""
    args, _, e_ref, agg_ref = _build(form, *HUB, True, _seed(form, "hub"))
    agg_old, e_old = _run(args, deterministic=True)
    agg, e_out = _run(args)
    d_e = (e_out - e_old).abs().max().item()
    r = _rel(agg, agg_old)
    print(f"{form} hub: max |e' new - old| = {d_e:.3e}, rel(agg new, old) = {r:.3e}")
    assert d_e == 0.0
    assert r <= ATOMICS_REL
    r_agg, r_e = _rel(agg, agg_ref), _rel(e_out, e_ref)
    print(f"{form} hub: rel(agg, float64) = {r_agg:.3e}, rel(e', float64) = {r_e:.3e}")
    assert r_agg <= FP32_REL and r_e <= FP32_REL


@functools.lru_cache(maxsize=None)
def _fallthrough_case(n_mid):
    return _build("processor", 2, 100, False, _seed("fall", str(n_mid)), n_mid)


@pytest.mark.parametrize("route", ["save", "deterministic", "two_middle_layers"])
def test_launches_the_new_kernel_refuses_still_run_on_edge_kernel(route):
    """Activation saving, deterministic segment sums and a deeper MLP are not the new kernel's: they reach edge_kernel as before."""
    args, _, e_ref, agg_ref = _fallthrough_case(2 if route == "two_middle_layers" else 1)
    kw = {}
    if route == "save":
        kw["save"] = SavedActivations(args[0], args[1] * int(args[2].shape[0]), DEV)
    elif route == "deterministic":
        kw["deterministic"] = True
    agg, e_out = _run(args, **kw)
    r_agg, r_e = _rel(agg, agg_ref), _rel(e_out, e_ref)
    print(f"{route}: rel(agg, float64) = {r_agg:.3e}, rel(e', float64) = {r_e:.3e}")
    assert r_agg <= FP32_REL and r_e <= FP32_REL
