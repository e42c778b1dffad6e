"""The training autograd nodes of graph_weather_amd/autograd.py without a GPU, over the case tables of tests/autograd_oracle.py.

1. The oracle against autograd: ``backward_from_saves`` fed the float64 forward's own saves equals torch's float64 autograd of the
   reference form to 1e-10, for every case.  That proves the reference tests/test_gpu_autograd_nodes.py holds the kernels to.
2. Preconditions of the cases: the route each edge case names is the one the restated dispatch gives, fewer than 0.1 % of the
   float64 pre-activations lie under the margin inside which a ReLU gate may differ between precisions, and the graphs have the
   hub, the empty destinations and the unused source they claim.
3. Host logic: ``EdgeUpdateFunction``, ``NodeUpdateFunction``, ``ProjectFunction`` and ``MLPRowsFunction`` themselves run on the
   CPU - every C-ABI call replaced by a torch restatement (tests/backward_restated.py for the backward primitives; the four
   forward entry points below, which fill the ``SavedActivations``), ``MLP.packed`` by a stand-in - and their outputs and
   gradients are compared with the float64 oracle at 2e-5, the bar of tests/test_backward_host_logic.py.  Which operand gets which
   slice, which table is summed over the batch and when the residual's gradient joins is thereby checked here."""
import types

import pytest
import torch

from graph_weather_amd import autograd as ag
from graph_weather_amd import layers, ops, routes

from . import autograd_oracle as ao
from .backward_restated import install

F64 = torch.float64


def _rel(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _all_ops():
    for c, g in ao.EDGE_PARAMS:
        yield "edge-%s-%s" % (c.name, g), ao.edge_op(c, g)
    for c, n in ao.NODE_PARAMS:
        yield "node-%s-%d" % (c.name, n), ao.node_op(c, n)
    for c, n in ao.ROWS_PARAMS:
        yield "rows-%s-%d" % (c.name, n), ao.rows_op(c, n)


ALL_OPS = [k for k, _ in _all_ops()]


@pytest.fixture(scope="module")
def all_ops():
    return dict(_all_ops())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the oracle against autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_OPS)
def test_backward_from_saves_equals_float64_autograd(all_ops, key):
    op, (dout, dagg) = all_ops[key]
    _, _, hidden, pre_norm, _ = ao.forward(op, *ao.leaves(op, F64))
    got = ao.joined(ao.backward_from_saves(op, hidden, pre_norm, dout, dagg), op)
    want = ao.autograd64(op, dout, dagg)
    assert set(got) == set(want)
    for k in want:
        assert _rel(got[k], want[k]) <= 1e-10, (k, _rel(got[k], want[k]))


@pytest.mark.parametrize("case,n", ao.PROJECT_PARAMS, ids=ao.PROJECT_IDS)
def test_project_backward_equals_float64_autograd(case, n):
    x, W0, douts, dpass = ao.project_operands(case, n)
    got = ao.project_backward(case, x, W0, douts, dpass)
    want = ao.project_autograd64(case, x, W0, douts, dpass)
    assert set(got) == set(want)
    for k in want:
        assert _rel(got[k], want[k]) <= 1e-10, (k, _rel(got[k], want[k]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. preconditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_OPS)
def test_fewer_than_a_thousandth_of_the_pre_activations_lie_under_the_margin(all_ops, key):
    op, _ = all_ops[key]
    total, inside = ao.margin_counts(ao.forward(op, *ao.leaves(op, F64))[4])
    print("%s: %d of %d pre-activations under the margin" % (key, inside, total))
    assert inside < 1e-3 * total


@pytest.mark.parametrize("case", ao.EDGE_CASES, ids=[c.name for c in ao.EDGE_CASES])
def test_edge_cases_reach_the_route_they_name(case):
    wid, hidden_layers, norm = ao.MLPS[case.mlp]
    got = ao.edge_training_route(torch.float32, case.modes, hidden_layers - 1, norm, wid)
    print("%s: fp32 %s, bf16x3 %s" % (case.name, got, ao.CHAINX3))
    assert got == case.route
    assert ao.edge_training_route(ao.BF16X3, case.modes, hidden_layers - 1, norm, wid) == ao.CHAINX3
    # the project's own facts the restatement leans on: what edge_fast_eligible reads of the packed MLP
    mlp = layers.EdgeProcessor(wid, wid, wid, hidden_layers, "LayerNorm" if norm else None).edge_mlp
    assert mlp.native_splits() == ((0, 256), (256, 512), (512, 768))
    assert len(mlp._linears()) - 2 == hidden_layers - 1 and (mlp._norm() is not None) == norm and mlp.out_dim == wid


def test_routes_cover_both_fp32_kernels_and_the_three_raw_operand_form():
    assert {c.route for c in ao.EDGE_CASES} == {ao.EDGE_KERNEL, ao.CHAIN_EDGE}
    assert any(c.modes == ("raw", "raw", "raw") and c.res == "e_in" for c in ao.EDGE_CASES)


def test_graphs_have_what_they_claim():
    g1, g2, g3 = ao.graph("G1"), ao.graph("G2"), ao.graph("G3")
    assert (g1.B, g1.E, g2.B, g2.E, g3.B, g3.E) == (2, 100, 1, 64 * 3 + 1, 3, 5)
    for g in (g1, g2, g3):
        assert g.n_src == 37 and (g.dst[1:] >= g.dst[:-1]).all() and g.src.max() == g.n_src - 1
        assert g.unused_src not in g.src  # a source row without an edge
        empty = sorted(set(range(g.n_dst)) - set(g.dst.tolist()))
        assert len(empty) >= 2 and empty[-2:] == [g.n_dst - 2, g.n_dst - 1]  # destinations without an edge, the last rows included
    # G1: a tile of 64 columns straddles the sample boundary, the last tile is ragged, and the hub's run crosses a tile boundary
    assert g1.E % 64 != 0 and (g1.B * g1.E) % 64 != 0
    run = [k for k in range(g1.E) if g1.dst[k] == g1.hub]
    assert len(run) == 70 and run == list(range(run[0], run[0] + 70))
    assert any((b * g1.E + run[0]) // 64 != (b * g1.E + run[-1]) // 64 for b in range(g1.B))
    assert g3.B * g3.E <= 64  # everything inside one tile


def test_node_form_with_saves_is_cols64():
    case = next(c for c in ao.NODE_CASES if c.name == "b1_form")
    n = case.sizes[0]
    assert routes.node_update_row_split_groups(case.B * n) > 0  # (the inference form of this size IS the row split ...)
    assert routes.node_update_form(torch.float32, case.B * n, True, "raw", 1, 0, saves=False).startswith("row_split")
    form = routes.node_update_form(torch.float32, case.B * n, True, "raw", 1, 0, saves=True)  # ... and saves exclude it
    print("node update, B = %d, %d rows, saves on: %s" % (case.B, n, form))
    assert form == routes.NODE_COLS64


# ---------------------------------------------------------------------------------------------------------------------
# 3. host logic: the Functions themselves on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _feed_of(o: ops.Operand, idx: torch.Tensor) -> ao.Feed:
    if o is None or o.k == 0 or o.tensor is None:
        return ao.Feed("zero", None, idx, 0, grad=False)
    width = min(int(o.k), int(o.tensor.shape[1]))
    return ao.Feed("proj" if o.projected else "raw", o.tensor.detach(), idx, int(o.rows_per_batch), width=width, k=width)


def _fill(save, hidden, y, pm):
    for l, h in enumerate(hidden):
        save.hidden[l].copy_(h.float())
    if save.pre_norm is not None:
        save.pre_norm.zero_()
        save.pre_norm[:, :pm.n_out].copy_(y.float())


def _run(pm, B, n, feeds, res, out_width, dst=None, n_dst=0):
    op = ao.Op(B, n, feeds, list(pm.splits), pm.params, pm.gamma is not None, res, None, out_width, dst, n_dst, ln_width=pm.ln_width)
    return ao.forward(op, *ao.leaves(op, F64))


@pytest.fixture
def host(monkeypatch):
    """Every C-ABI call of the four nodes as a float64 torch restatement (results rounded to float32 where the kernels store)."""
    calls = install(monkeypatch)

    def packed(self):
        with torch.no_grad():
            ps = [p.detach() for p in self.native_params()]
        norm = self._norm() is not None
        n_lin = (len(ps) - (2 if norm else 0)) // 2
        W0 = ps[0]
        return types.SimpleNamespace(params=ps, splits=self.native_splits(), n_mid=n_lin - 2, hidden=int(W0.shape[0]),
                                     n_out=int(ps[2 * n_lin - 2].shape[0]), gamma=ps[-2] if norm else None,
                                     ln_width=self.out_dim if (norm and self.out_dim < int(ps[2 * n_lin - 2].shape[0])) else 0,
                                     w1=[W0[:, lo:hi] for lo, hi in self.native_splits()])

    def edge_update_forward(pm, batch, src, dst, x_src, x_dst, e_in, e_res, n_dst, agg, e_out, tag=None, save=None, **kw):
        E = int(src.shape[0])
        idx = (src.long(), dst.long(), torch.arange(E))
        feeds = [_feed_of(o, i) for o, i in zip((x_src, x_dst, e_in), idx)]
        out, a, hidden, y, _ = _run(pm, batch, E, feeds, _feed_of(e_res, idx[2]), 256, idx[1], n_dst)
        agg.add_(a.float())
        if e_out is not None:
            e_out.copy_(out.float())
        _fill(save, hidden, y, pm)

    def node_update_forward(pm, n_rows, rows_per_batch, x, x_res, agg, out=None, save=None, **kw):
        ar = torch.arange(rows_per_batch)
        res = _feed_of(x_res, ar)
        o, _, hidden, y, _ = _run(pm, n_rows // rows_per_batch, rows_per_batch, [_feed_of(x, ar), _feed_of(agg, ar)],
                                  None if res.mode == "zero" else res, 256)
        _fill(save, hidden, y, pm)
        return o.float()

    def mlp_forward(pm, x, n_rows, rows_per_batch, residual=None, out=None, save=None):
        ar = torch.arange(rows_per_batch)
        res = None
        if residual is not None:
            res = ao.Feed("raw", residual.tensor.detach(), ar, int(residual.rows_per_batch), width=int(residual.tensor.shape[1]))
        o, _, hidden, y, _ = _run(pm, n_rows // rows_per_batch, rows_per_batch, [_feed_of(x, ar)], res, pm.n_out)
        _fill(save, hidden, y, pm)
        return o.float()

    def project_forward(w_slices, x, n_rows, rows_per_batch, **kw):
        return [(x.tensor.detach()[:, :256].double() @ w.double().t()).float() for w in w_slices]

    monkeypatch.setattr(layers.MLP, "packed", packed)
    for name, fn in (("edge_update_forward", edge_update_forward), ("node_update_forward", node_update_forward),
                     ("mlp_forward", mlp_forward), ("project_forward", project_forward)):
        monkeypatch.setattr(ops, name, fn)
    return calls


BAR = 2e-5  # the bar of tests/test_backward_host_logic.py


def _check(kind, op, douts, outs, inputs, fn, mlp, raw_slots):
    """Outputs and every gradient against the float64 oracle; ``raw_slots``: {input name: position in backward's result}."""
    P, T, R = ao.leaves(op, F64)
    out64, agg64, _, _, _ = ao.forward(op, P, T, R)
    if outs.get("rows") is not None:
        assert _rel(outs["rows"], out64) <= BAR
    if outs.get("agg") is not None:
        assert _rel(outs["agg"], agg64) <= BAR
    dout, dagg = douts
    if outs.get("rows") is None:
        dout = None
    got = ao.node_grads(outs, (dout, dagg), mlp, op, inputs)
    want = ao.autograd64(op, dout, dagg)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, ref in want.items():
        assert got[k] is not None, k
        g = got[k]
        assert tuple(g.shape) == tuple(ref.shape), (k, g.shape, ref.shape)
        r = _rel(g, ref)
        assert r <= BAR, (k, r)
    raw = ao.raw_backward(fn, *[d for d in ((dagg, dout if dout is not None else torch.zeros(0)) if kind == "edge" else (dout,))])
    for name, slot in raw_slots.items():
        needs = name in inputs and inputs[name].requires_grad
        if not needs:
            assert raw[slot] is None, (name, "an input that needs no gradient gets None")
    return raw


@pytest.mark.parametrize("case,gname", ao.EDGE_PARAMS, ids=ao.EDGE_IDS)
def test_edge_update_function_on_the_host(host, case, gname):
    op, douts = ao.edge_op(case, gname)
    mlp = ao.module_for("edge", op, case.mlp)
    outs, inputs, fn = ao.call_edge(case, gname, op, mlp, "cpu")
    assert (outs["rows"] is not None) == case.want_edges
    raw = _check("edge", op, douts, outs, inputs, fn, mlp, {"op0": 5, "op1": 6, "op2": 7})
    if op.res_is is not None and case.grads != "params" and case.mlp == "std":
        # the gradient of e is ONE tensor carrying both uses: the residual's slot is empty, the join happened in the launch
        assert raw[8] is None and raw[7] is not None
        assert any(c.startswith("chain") for c in host.names)
    if case.grads == "params":
        assert raw[8] is None


@pytest.mark.parametrize("case,n", ao.NODE_PARAMS, ids=ao.NODE_IDS)
def test_node_update_function_on_the_host(host, case, n):
    op, douts = ao.node_op(case, n)
    mlp = ao.module_for("node", op, case.mlp)
    outs, inputs, fn = ao.call_node(case, op, mlp, "cpu")
    _check("node", op, douts, outs, inputs, fn, mlp, {"op0": 5, "res": 6, "op1": 7})


@pytest.mark.parametrize("case,n", ao.ROWS_PARAMS, ids=ao.ROWS_IDS)
def test_mlp_rows_function_on_the_host(host, case, n):
    op, douts = ao.rows_op(case, n)
    mlp = ao.module_for("rows", op, rows_case=case)
    outs, inputs, fn = ao.call_rows(case, op, mlp, "cpu")
    _check("rows", op, douts, outs, inputs, fn, mlp, {"op0": 1, "res": 2})


def test_mlp_rows_refuses_the_gradient_of_a_residual_shared_by_the_batch(host):
    case = next(c for c in ao.ROWS_CASES if c.name == "head256_res78_ln")
    op, _ = ao.rows_op(case, 63)
    mlp = ao.module_for("rows", op, rows_case=case)
    x = torch.zeros(2 * 63, 256)
    res = op.res.table.clone().requires_grad_(True)  # 63 rows for 2 x 63: shared by the batch
    with pytest.raises(NotImplementedError, match="gradient of a residual table shared by the batch is not implemented"):
        ag.mlp_rows(mlp, x, 2 * 63, 63, residual_op=ops.Operand(res, 0, 78))


@pytest.mark.parametrize("case,n", ao.PROJECT_PARAMS, ids=ao.PROJECT_IDS)
def test_project_function_on_the_host(host, case, n):
    got, want, raw = ao.run_project(case, n, "cpu", torch.float32)
    for k, ref in want.items():
        assert _rel(got[k], ref) <= BAR, (k, _rel(got[k], ref))
    if not case.x_grad:
        assert raw[3] is None
