"""The four training autograd nodes of graph_weather_amd/autograd.py - ``EdgeUpdateFunction``, ``NodeUpdateFunction``,
``ProjectFunction``, ``MLPRowsFunction`` - and the activation saves their forward kernels write, against float64, over the case
tables of tests/autograd_oracle.py (tests/test_autograd_nodes_host.py proves that oracle and the cases' preconditions on the CPU).
Every case runs in fp32 and in bf16x3 and has three parts, each failing for its own reason only:

A. Forward and saves by value.  The node is called through ``ag.edge_update`` / ``ag.node_update`` / ``ag.project`` /
   ``ag.mlp_rows``; the ``SavedActivations`` its forward filled is read through ``out.grad_fn.save``.  ``agg``, ``e'`` / ``x'``,
   every ``hidden[l]`` and ``pre_norm`` are compared with the float64 restatement over all rows and columns at the bar the project
   applies to these kernels' rows (2e-4 of the tensor's maximum: FP32_REL of tests/test_gpu_edge_lds.py, X3_REL of
   tests/test_gpu_split.py); padded columns of narrow and head forms are exactly 0, rows of ``agg`` without an edge exactly 0.  The
   ReLU masks agree wherever the float64 pre-activation is at least 1e-4 of its layer's maximum; the entries under that margin
   and the disagreements among them are printed.
B. Backward against the float64 backward evaluated ON THE SAVES THE KERNEL WROTE (``backward_from_saves``): error = max
   |got - ref64|, yardstick = the same formulas in float32 on the CPU on the same saves, bar = max(4 x yardstick, floor x max
   |ref64|), floor = max(1e-6, 2^-24 sqrt(K)) for fp32 with K the terms of the longest sum (``longest_sums``) and 5e-5 for bf16x3
   (the figure tests/test_gpu_round6.py holds the same split products to).  Printed as ratio = error / max(yardstick, floor x
   max |ref64| / 4): the bar reads as ratio 4.  Exact: the W0 block of a projected or absent operand is 0, the gradient row of a
   source or destination without an edge is 0, an input that needs no gradient gets None, and where e is operand and residual
   its gradient is ONE tensor equal to the reference's sum of the two.
C. End to end: the same gradients against float64 autograd of the reference form (gates from float64) at the bar of
   tests/test_gpu_backward.py, 2e-3 of each tensor's maximum - coarse; a save and a backward wrong in the same way cannot pass
   A and B together and this.  One amendment, without which C is not well posed at these sizes: where part A found an entry under
   the margin whose gate differs from float64's (z is zero to working precision there and either derivative of ReLU is right),
   the float64 autograd takes the kernel's gate on THAT entry; every other gate is float64's.  With a few dozen rows behind a
   weight gradient one such entry moves the tensor by far more than 2e-3: in the run below 13 entries differed, in 12 of the 192
   cases (11 bf16x3, 1 fp32), never more than one per layer, and with float64's gate on them the worst figures were 0.27 (node
   proj_per-2x100 bf16x3, W1), 0.20 (rows in256-63, W0, fp32 and bf16x3 alike) and 0.09 (edge encoder_inputs_frozen-G1 bf16x3,
   W0); that figure is printed, not asserted, whenever an entry differs.  With the kernel's gate on them the worst C figure of
   the file is 1.3e-5.

Measured on an MI355X (the 192 tests of this file: 5.7 s alone with start-up, the slowest 1.4 s - the first, which loads the
library - and none of the others above 0.1 s).  Worst figure per node, forward route and dtype, with its case:

    node     forward kernel              dtype   A rel (bar 2e-4)                  B ratio (bar 4)            C rel (bar 2e-3)
    edge     edge_kernel+save            fp32    6.2e-7  encoder_edges-G3 pre_norm  2.86  raw_dst-G1 W0        7.2e-7
    edge     chain_kernel EPI_EDGE+save  fp32    1.1e-6  all_raw-G1 hidden[0]       2.35  deep-G1 W3           6.2e-7
    edge     chainx3+save                bf16x3  8.8e-6  narrow-G1 pre_norm         0.83  deep-G1 W0           1.0e-5
    node     cols64 (chain_kernel)       fp32    8.8e-7  frozen_strided_per hidden  2.61  deep-2x100 W3        7.4e-7
    node     cols64 (chainx3_kernel)     bf16x3  9.6e-6  zero-2x37 pre_norm         0.77  proj_shared-2x37 W0  1.1e-5
    rows     chain_kernel EPI_ROWS / DEC fp32    7.5e-7  head256_res78_nonorm-130   1.65  in256-63 dx          7.2e-7
    rows     chainx3_kernel              bf16x3  1.2e-5  in2-130 pre_norm           1.11  in102-1 W0           1.3e-5
    project  gw_project_forward          fp32    (outputs under B)                  2.13  s0-1 out0            -
    project  gw_project_forward          bf16x3                                     0.97  s01-1 W0             -

No bf16x3 form was refused by an entry point.

Found with this file's cases on the CPU (tests/test_autograd_nodes_host.py) and mended in autograd.py: the backward took a
table that is wider than its 256 features (a leading dimension above 256, which the forward reads through the row stride) as it
was - the weight-gradient product of a raw e, agg, x or projected x wrote 320 columns into a 256-column block of W0's gradient
(past its end for the last block), and gw_gather_rows read a raw node table as packed rows.  Cases
processor_inputs_frozen, encoder_inputs_frozen, frozen_strided_per, frozen_strided_shared and s2_x_frozen_strided.
"""
import pytest
import torch

from graph_weather_amd import autograd as ag
from graph_weather_amd import ops, routes

from . import autograd_oracle as ao

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
FP32_REL = 2e-4  # tests/test_gpu_edge_lds.py
X3_REL = 2e-4  # tests/test_gpu_split.py
X3_FLOOR = 5e-5  # tests/test_gpu_round6.py: test_chain_backward_on_split_operands_against_torch_and_the_single_products
REL = 2e-3  # tests/test_gpu_backward.py
DTYPES = [torch.float32, ao.BF16X3]
DTYPE_IDS = ["fp32", "bf16x3"]


def _maxabs(t):
    return max(t.abs().max().item(), 1e-30) if t.numel() else 1e-30


def _value(tag, name, got, ref, bar):
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref.shape), (tag, name, tuple(got.shape), tuple(ref.shape))
    rel = (got - ref).abs().max().item() / _maxabs(ref)
    print("%s A %-9s rel %.3e (bar %.0e)" % (tag, name, rel, bar))
    assert rel <= bar, (tag, name, rel)


def check_forward(tag, op, outs, save, dtype):
    """Part A.  Returns the kernel's saves in the parameters' own widths (float32, CPU) and, per layer, the entries under the
    margin whose gate differs from float64's: (hidden, pre_norm, flips)."""
    bar = FP32_REL if dtype == torch.float32 else X3_REL
    out64, agg64, hidden64, y64, pre64 = ao.forward(op, *ao.leaves(op, F64))
    n_out = int(op.params[2 * op.n_lin - 2].shape[0])
    if outs.get("agg") is not None:
        agg = outs["agg"].detach().cpu()
        _value(tag, "agg", agg, agg64, bar)
        empty = sorted(set(range(op.n_dst)) - set(op.dst.tolist()))
        assert len(empty) >= 2 and bool((agg.reshape(op.B, op.n_dst, -1)[:, empty] == 0).all()), (tag, "agg rows without an edge")
    if outs.get("rows") is not None:
        rows = outs["rows"].detach().cpu()
        _value(tag, "rows", rows, out64, bar)
        if n_out < op.out_width:  # zero-padded narrow outputs (the residual's padding is zero too)
            assert bool((rows[:, n_out:] == 0).all()), (tag, "padded output columns")
    hid = save.hidden.detach().cpu()
    assert hid.shape[0] == len(hidden64) and hid.shape[1] == op.rows
    hidden, flips = [], []
    for l, h64 in enumerate(hidden64):
        w = int(h64.shape[1])
        got = hid[l][:, :w]
        assert bool((hid[l][:, w:] == 0).all()), (tag, "padded hidden columns of layer %d" % l)
        _value(tag, "hidden[%d]" % l, got, h64, bar)
        z = pre64[l]
        strong = z.abs() >= ao.MARGIN * z.abs().max()
        differ = (got > 0) != (h64 > 0)
        print("%s A mask[%d]   %d of %d entries under the margin, %d of them differ" % (tag, l, int((~strong).sum()), z.numel(),
                                                                                 int((differ & ~strong).sum())))
        assert not bool((differ & strong).any()), (tag, "relu mask of layer %d" % l, int((differ & strong).sum()))
        hidden.append(got)
        flips.append(differ & ~strong)
    pre_norm = None
    if op.norm:
        pn = save.pre_norm.detach().cpu()
        assert pn.shape[0] == op.rows and bool((pn[:, n_out:] == 0).all()), (tag, "padded pre_norm columns")
        pre_norm = pn[:, :n_out]
        _value(tag, "pre_norm", pre_norm, y64, bar)
    else:
        assert save.pre_norm is None
    return hidden, pre_norm, flips


def check_backward(tag, op, got, hidden, pre_norm, flips, douts, dtype):
    """Parts B and C on the gradients ``got`` ({name: tensor}); returns the worst ratio of part B."""
    dout, dagg = douts
    ref = ao.joined(ao.backward_from_saves(op, hidden, pre_norm, dout, dagg, F64), op)
    yard = ao.joined(ao.backward_from_saves(op, hidden, pre_norm, dout, dagg, F32), op)
    K = ao.longest_sums(op)
    assert set(got) == set(ref), (tag, sorted(got), sorted(ref))
    worst = 0.0
    for k, r in ref.items():
        assert got[k] is not None, (tag, k)
        g = got[k].detach().cpu().double()
        assert tuple(g.shape) == tuple(r.shape), (tag, k, tuple(g.shape), tuple(r.shape))
        err = (g - r).abs().max().item()
        y = (yard[k].double() - r).abs().max().item()
        floor = (ao.fp32_floor(K[k]) if dtype == torch.float32 else X3_FLOOR) * _maxabs(r)
        bar = max(4 * y, floor)
        ratio = err / max(y, floor / 4)
        worst = max(worst, ratio)
        print("%s B %-6s err %.3e yardstick %.3e bar %.3e ratio %.2f" % (tag, k, err, y, bar, ratio))
        assert err <= bar, (tag, k, err, bar)
    print("%s B worst ratio %.2f" % (tag, worst))
    n_flips = sum(int(f.sum()) for f in flips)
    if n_flips:  # measured, not asserted: what the gates of float64 alone give (see the docstring: one such entry moves a tensor by > REL)
        for k, r in ao.autograd64(op, dout, dagg).items():
            rel = (got[k].detach().cpu().double() - r).abs().max().item() / _maxabs(r)
            print("%s C %-6s rel %.3e with float64's gate on the %d entries under the margin that differ" % (tag, k, rel, n_flips))
    end = ao.autograd64(op, dout, dagg, flips if n_flips else None)
    assert set(end) == set(got)
    for k, r in end.items():
        rel = (got[k].detach().cpu().double() - r).abs().max().item() / _maxabs(r)
        print("%s C %-6s rel %.3e (bar %.0e)" % (tag, k, rel, REL))
        assert rel <= REL, (tag, k, rel)
    # exact: the W0 block of an operand that is projected or absent (its gradient arrives through ProjectFunction)
    if op.param_grad:
        for i, f in enumerate(op.feeds):
            if f.mode != "raw":
                lo, hi = op.splits[i]
                assert bool((got["W0"][:, lo:hi] == 0).all()), (tag, "W0 block of operand %d" % i)
    return worst


def exact_rows_without_an_edge(tag, op, got, g):
    """The gradient row of a source / destination no edge touches is exactly 0."""
    empty_dst = sorted(set(range(g.n_dst)) - set(g.dst.tolist()))
    for key, rows, n_tab in (("op0", [g.unused_src], g.n_src), ("op1", empty_dst, g.n_dst)):
        if key in got:
            t = got[key].detach().cpu().reshape(-1, n_tab, 256)
            assert bool((t[:, rows] == 0).all()), (tag, key, "rows without an edge")


def _to_dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case,gname", ao.EDGE_PARAMS, ids=ao.EDGE_IDS)
def test_edge_update(case, gname, dtype):
    op, douts = ao.edge_op(case, gname)
    wid, hidden_layers, norm = ao.MLPS[case.mlp]
    route = ao.edge_training_route(dtype, case.modes, hidden_layers - 1, norm, wid)
    tag = "edge %s-%s %s [%s]" % (case.name, gname, DTYPE_IDS[DTYPES.index(dtype)], route)
    print(tag)
    assert route == (case.route if dtype == torch.float32 else ao.CHAINX3)
    mlp = ao.module_for("edge", op, case.mlp, device=DEV, dtype=dtype)
    outs, inputs, fn = ao.call_edge(case, gname, op, mlp, DEV)
    assert (outs["rows"] is not None) == case.want_edges
    hidden, pre_norm, flips = check_forward(tag, op, outs, fn.save, dtype)
    got = ao.node_grads(outs, douts, mlp, op, inputs)
    check_backward(tag, op, got, hidden, pre_norm, flips, douts, dtype)
    exact_rows_without_an_edge(tag, op, got, ao.graph(gname))
    de_out, dagg = douts
    raw = ao.raw_backward(fn, dagg.to(DEV), de_out.to(DEV) if de_out is not None else torch.zeros(0, device=DEV))
    for i in range(3):
        name = "op%d" % i
        if not (name in inputs and inputs[name].requires_grad):
            assert raw[5 + i] is None, (tag, name, "an input that needs no gradient gets None")
    if case.grads == "params":
        assert raw[8] is None
    if (case.name.startswith("processor") or case.name == "all_raw") and case.grads != "params":
        # e is operand and residual: ONE tensor carries both uses (checked against the reference's sum in part B)
        assert raw[8] is None and raw[7] is not None and torch.equal(raw[7], got["op2"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case,n", ao.NODE_PARAMS, ids=ao.NODE_IDS)
def test_node_update(case, n, dtype):
    op, douts = ao.node_op(case, n)
    tag = "node %s-%dx%d %s [cols64]" % (case.name, case.B, n, DTYPE_IDS[DTYPES.index(dtype)])
    print(tag)
    if case.name == "b1_form":  # a mesh-sized launch: without saves it is the row split; with saves on it must be the 64-column kernels
        form = routes.node_update_form(dtype, op.rows, True, case.x_mode, op.n_lin - 2, 0, saves=True)
        print("%s node_update_form with saves: %s (without: %s)" % (tag, form, routes.node_update_form(dtype, op.rows, True, case.x_mode,
                                                                                                    op.n_lin - 2, 0, saves=False)))
        assert form == routes.NODE_COLS64
    mlp = ao.module_for("node", op, case.mlp, device=DEV, dtype=dtype)
    outs, inputs, fn = ao.call_node(case, op, mlp, DEV)
    hidden, pre_norm, flips = check_forward(tag, op, outs, fn.save, dtype)
    got = ao.node_grads(outs, douts, mlp, op, inputs)
    check_backward(tag, op, got, hidden, pre_norm, flips, douts, dtype)
    raw = ao.raw_backward(fn, douts[0].to(DEV))
    for name, slot in (("op0", 5), ("res", 6), ("op1", 7)):
        if not (name in inputs and inputs[name].requires_grad):
            assert raw[slot] is None, (tag, name, "an input that needs no gradient gets None")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case,n", ao.ROWS_PARAMS, ids=ao.ROWS_IDS)
def test_mlp_rows(case, n, dtype):
    op, douts = ao.rows_op(case, n)
    tag = "rows %s-%d %s" % (case.name, n, DTYPE_IDS[DTYPES.index(dtype)])
    print(tag)
    mlp = ao.module_for("rows", op, rows_case=case, device=DEV, dtype=dtype)
    outs, inputs, fn = ao.call_rows(case, op, mlp, DEV)
    hidden, pre_norm, flips = check_forward(tag, op, outs, fn.save, dtype)
    got = ao.node_grads(outs, douts, mlp, op, inputs)
    check_backward(tag, op, got, hidden, pre_norm, flips, douts, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_mlp_rows_refuses_the_gradient_of_a_residual_shared_by_the_batch(dtype):
    case = next(c for c in ao.ROWS_CASES if c.name == "head256_res78_ln")
    op, _ = ao.rows_op(case, 63)
    mlp = ao.module_for("rows", op, rows_case=case, device=DEV, dtype=dtype)
    x = torch.zeros(2 * 63, 256, device=DEV)
    res = op.res.table.to(DEV).requires_grad_(True)  # 63 rows for 2 x 63: shared by the batch
    with pytest.raises(NotImplementedError, match="gradient of a residual table shared by the batch is not implemented"):
        ag.mlp_rows(mlp, x, 2 * 63, 63, residual_op=ops.Operand(res, 0, 78))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case,n", ao.PROJECT_PARAMS, ids=ao.PROJECT_IDS)
def test_project(case, n, dtype):
    tag = "project %s-%d %s" % (case.name, n, DTYPE_IDS[DTYPES.index(dtype)])
    print(tag)
    got, want, raw = ao.run_project(case, n, DEV, dtype)
    x, W0, douts, dpass = ao.project_operands(case, n)
    yard = ao.project_backward(case, x, W0, douts, dpass, F32)
    fwd32 = ao.project_forward(case, x, W0)
    worst = 0.0
    for k, r in want.items():
        g = got[k].detach().cpu().double()
        assert tuple(g.shape) == tuple(r.shape)
        y32 = yard[k] if k in yard else fwd32[int(k[3:])]
        err, y = (g - r).abs().max().item(), (y32.double() - r).abs().max().item()
        terms = n if k == "W0" else 256 * max(1, len(case.slices))  # rows of a weight gradient; a row product (per slice joined)
        floor = (ao.fp32_floor(terms) if dtype == torch.float32 else X3_FLOOR) * _maxabs(r)
        bar, ratio = max(4 * y, floor), err / max(y, floor / 4)
        worst = max(worst, ratio)
        print("%s B %-6s err %.3e yardstick %.3e bar %.3e ratio %.2f" % (tag, k, err, y, bar, ratio))
        assert err <= bar, (tag, k, err, bar)
    print("%s B worst ratio %.2f" % (tag, worst))
    used = {s for s, d in zip(case.slices, douts) if d is not None}
    for s in range(3):
        if s not in used:  # the block of a slice that is absent or unused in the loss: exactly 0
            lo, hi = ao.PROJECT_SPLITS[s]
            assert bool((got["W0"][:, lo:hi] == 0).all()), (tag, "W0 block of slice %d" % s)
    if not case.x_grad:
        assert raw[3] is None
