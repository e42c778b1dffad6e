"""Plain-torch oracle of the four training autograd nodes of graph_weather_amd/autograd.py (``EdgeUpdateFunction``,
``NodeUpdateFunction``, ``ProjectFunction``, ``MLPRowsFunction``): the case tables, the graphs, a forward restatement in a chosen
dtype that also returns the activation saves it implies, a backward evaluated FROM GIVEN SAVES, and the restated dispatch of the
training edge update.  Importable without a GPU: tests/test_autograd_nodes_host.py proves it against torch's float64 autograd and
tests/test_gpu_autograd_nodes.py holds the kernels to it.

One description serves the three MLP nodes (``Op``): operands ("feeds") are row tables read through an index, either raw (they
enter Linear_0 through their column block of W0 - the reference's ``cat`` -> Linear, graph_net_block.py:131-134) or projected
(rows already multiplied by that block: gather-added to the pre-activation) or absent; then the Linear / ReLU chain, an optional
LayerNorm (eps 1e-5), a residual, and for the edge update ``index_add_`` by destination (graph_net_block.py:188).  Everything is in
the parameters' own widths: a narrow (128) model is computed 128 wide and compared with the first 128 columns of the kernels'
zero-padded tables.

``backward_from_saves`` is linear in the output gradients once ``hidden`` and ``pre_norm`` are given: fed the saves a kernel wrote,
it is the reference for that kernel's backward without a ReLU gate that flipped between precisions entering the comparison."""
import dataclasses
import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
LD = 320  # leading dimension of the tables that are wider than their 256 features; the padding holds PAD_VALUE
PAD_VALUE = 1e3
MARGIN = 1e-4  # |pre-activation| below MARGIN * max |pre-activation| of its layer: the sign may differ between precisions
BF16X3 = "bf16x3"


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Graph:
    name: str
    B: int
    E: int
    n_src: int
    n_dst: int
    src: np.ndarray  # int32 [E]
    dst: np.ndarray  # int32 [E], sorted
    hub: Optional[int]  # destination with the long run
    unused_src: int  # a source row no edge starts from


@functools.lru_cache(maxsize=None)
def graph(name: str) -> Graph:
    rs = np.random.RandomState(sum(map(ord, name)))
    n_src = 37
    if name == "G1":
        # B = 2, E = 100: the tile of columns 64..127 straddles the sample boundary (column 100) and the last tile is ragged; the
        # hub's 70 edges are k = 20..89: its run crosses column 64 in sample 0 and columns 128 (k = 28) in sample 1
        B, E, hub = 2, 100, 11
        head = np.sort(rs.choice(np.arange(0, 10), size=20))  # (some of 0..9 get no edge)
        tail = np.sort(rs.choice(np.arange(12, 17), size=10))
        dst = np.concatenate([head, np.full(70, hub), tail]).astype(np.int32)
    elif name == "G2":
        B, E, hub = 1, 64 * 3 + 1, None
        dst = np.sort(rs.randint(0, 60, size=E)).astype(np.int32)
    elif name == "G3":
        B, E, hub = 3, 5, None
        dst = np.asarray([0, 0, 2, 2, 3], dtype=np.int32)
    else:
        raise KeyError(name)
    n_dst = int(dst.max()) + 3  # the last rows have no edge
    unused = 5
    src = rs.choice(np.setdiff1d(np.arange(n_src), [unused]), size=E).astype(np.int32)
    src[0] = n_src - 1
    return Graph(name, B, E, n_src, n_dst, src, dst, hub, unused)


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
MLPS = {  # name: (feature width of tables and hidden units, hidden_layers, LayerNorm)
    "std": (256, 2, True),
    "deep": (256, 3, True),      # n_mid = 2: three saved layers, the general chain kernel
    "no_norm": (256, 2, False),  # norm_type=None: no pre_norm, the bias routes of _mlp_chain_backward
    "narrow": (128, 2, True),    # zero-padded tables, ln_width = 128, gradients through the differentiable pads of native_params
}

EDGE_KERNEL, CHAIN_EDGE, CHAINX3 = "edge_kernel+save", "chain_kernel EPI_EDGE+save", "chainx3+save"


@dataclasses.dataclass(frozen=True)
class EdgeCase:
    name: str
    modes: Tuple[str, str, str]  # (x_src, x_dst, e_in): "zero" | "raw" | "proj"
    shared: Tuple[bool, bool, bool]  # the operand's table is shared by the batch (rows_pb == 0)
    res: str  # "e_in" (the same tensor as e_in) | "per" (its own per-sample table) | "shared"
    want_edges: bool
    grads: str = "all"  # "all" | "params" (inputs detached) | "inputs" (parameters frozen)
    mlp: str = "std"
    route: str = EDGE_KERNEL  # the fp32 forward kernel the case is there for (bf16x3: always chainx3)
    graphs: Tuple[str, ...] = ("G1",)
    strided: Tuple[int, ...] = ()  # operands (3: the residual) whose table has leading dimension LD
    seed: int = 0
    note: str = ""


_PROC = dict(modes=("proj", "proj", "raw"), shared=(False, False, False), res="e_in")
EDGE_CASES = [
    EdgeCase("processor", **_PROC, want_edges=True, graphs=("G1", "G2"), note="the same_e join"),
    EdgeCase("processor_last", **_PROC, want_edges=False),
    # (tables that need no gradient may be strided: both products, and e, which is the residual too.  Regression: the weight-
    # gradient product of a raw e wider than its features wrote 320 columns into the 256-column block of W0's gradient)
    EdgeCase("processor_inputs_frozen", **_PROC, want_edges=True, grads="params", strided=(0, 1, 2)),
    EdgeCase("processor_params_frozen", **_PROC, want_edges=True, grads="inputs"),
    EdgeCase("encoder", ("raw", "zero", "proj"), (False, False, True), "shared", False, graphs=("G1", "G3"),
             note="the gather-of-batch-sum branch of de_res"),
    EdgeCase("encoder_inputs_frozen", ("raw", "zero", "proj"), (False, False, True), "shared", False, grads="params",
             strided=(0, 2, 3), note="regression: a raw table wider than its 256 features went to gw_gather_rows as packed rows"),
    EdgeCase("encoder_edges", ("raw", "zero", "proj"), (False, False, True), "shared", True, graphs=("G1", "G3"),
             note="de_out present: the segment_sum_rows(dn.rows(), ...) branch"),
    EdgeCase("decoder", ("proj", "proj", "proj"), (False, True, True), "per", False, graphs=("G1", "G3"),
             note="no raw operand: bias0_in_chain"),
    EdgeCase("raw_dst", ("zero", "raw", "proj"), (False, False, False), "per", True),
    EdgeCase("raw_shared", ("raw", "proj", "zero"), (True, False, False), "per", True, graphs=("G1", "G3"),
             note="a raw table shared by the batch: gather_rows with rows_pb == 0, its gradient summed over the batch"),
    EdgeCase("all_raw", ("raw", "raw", "raw"), (False, False, False), "e_in", True, route=CHAIN_EDGE, graphs=("G1", "G2"),
             note="general chain kernel, three fan products, same_e on that route"),
    EdgeCase("two_raw", ("raw", "raw", "zero"), (False, False, False), "per", True, route=CHAIN_EDGE),
    EdgeCase("deep", **_PROC, want_edges=True, mlp="deep", route=CHAIN_EDGE),
    EdgeCase("no_norm", **_PROC, want_edges=True, mlp="no_norm", route=CHAIN_EDGE),
    EdgeCase("narrow", **_PROC, want_edges=True, mlp="narrow", route=CHAIN_EDGE),
]
EDGE_PARAMS = [(c, g) for c in EDGE_CASES for g in c.graphs]
EDGE_IDS = ["%s-%s" % (c.name, g) for c, g in EDGE_PARAMS]


@dataclasses.dataclass(frozen=True)
class NodeCase:
    name: str
    x_mode: str
    x_shared: bool
    res: Optional[str]  # "per" | "shared" | None
    agg_grad: bool = True
    mlp: str = "std"
    B: int = 2
    sizes: Tuple[int, ...] = (37, 100)  # rows per sample
    seed: int = 0
    frozen_strided: bool = False  # no input needs a gradient and every table has leading dimension LD


NODE_CASES = [
    NodeCase("raw_per", "raw", False, "per"),
    NodeCase("raw_shared", "raw", True, "per"),
    NodeCase("proj_per", "proj", False, "shared"),
    NodeCase("proj_shared", "proj", True, "per", agg_grad=False),
    NodeCase("zero", "zero", False, None),
    NodeCase("deep", "raw", False, "per", mlp="deep"),
    NodeCase("no_norm", "raw", False, "per", mlp="no_norm"),
    NodeCase("narrow", "raw", False, "per", mlp="narrow"),
    # regression: tables wider than their 256 features reached the weight-gradient products and gw_gather_rows as they were
    NodeCase("frozen_strided_per", "raw", False, "per", agg_grad=False, frozen_strided=True, sizes=(37,)),
    NodeCase("frozen_strided_shared", "raw", True, "shared", agg_grad=False, frozen_strided=True, sizes=(37,)),
    NodeCase("b1_form", "raw", False, "per", B=1, sizes=(37,)),  # records the node form taken with saves on (cols64)
    NodeCase("b3_shared_res", "raw", True, "shared", B=3, sizes=(37,)),  # a batch above 2 in the shared-table sums
]
NODE_PARAMS = [(c, n) for c in NODE_CASES for n in c.sizes]
NODE_IDS = ["%s-%dx%d" % (c.name, c.B, n) for c, n in NODE_PARAMS]


@dataclasses.dataclass(frozen=True)
class ProjectCase:
    name: str
    slices: Tuple[int, ...]
    passthrough: bool = False
    unused: Tuple[int, ...] = ()  # outputs (positions in ``slices``) that do not enter the loss: their dout is None
    x_grad: bool = True
    ld: int = 256  # leading dimension of x (above 256: padding never to be read; only where x needs no gradient)


PROJECT_CASES = [
    ProjectCase("s0", (0,)),
    ProjectCase("s01", (0, 1)),
    ProjectCase("s2", (2,)),
    ProjectCase("s2_passthrough", (2,), passthrough=True),
    ProjectCase("s01_one_unused", (0, 1), unused=(1,)),
    ProjectCase("s01_x_frozen", (0, 1), x_grad=False),
    # regression: the weight-gradient product took all 320 columns of x into the 256-column block of W0's gradient
    ProjectCase("s2_x_frozen_strided", (2,), x_grad=False, ld=LD),
]
PROJECT_ROWS = (1, 37, 130)
PROJECT_PARAMS = [(c, n) for c in PROJECT_CASES for n in PROJECT_ROWS]
PROJECT_IDS = ["%s-%d" % (c.name, n) for c, n in PROJECT_PARAMS]


@dataclasses.dataclass(frozen=True)
class RowsCase:
    name: str
    in_dim: int
    hidden: int
    out: int
    norm: bool
    res_width: Optional[int] = None  # 78: dres is dy itself; 102: the zero-padded dres branch
    seed: int = 0


# (in2: seed 4 - with seed 0 the 130-row case has 0.105 % of its pre-activations under the margin, the precondition is < 0.1 %)
ROWS_CASES = ([RowsCase("in%d" % k, k, 256, 256, True, seed=4 if k == 2 else 0) for k in (2, 102, 256)]
              + [RowsCase("head%d_res%d_%s" % (h, r, "ln" if n else "nonorm"), 256, h, 78, n, r)
                 for h in (128, 256) for r in (78, 102) for n in (True, False)])
ROWS_ROWS = (1, 63, 130)
# (case, rows) whose seed was changed for the margin precondition: the one row of this case has 1 of its 512 pre-activations under it
ROWS_SEED_SHIFT = {("head256_res102_ln", 1): 1}
ROWS_PARAMS = [(c, n) for c in ROWS_CASES for n in ROWS_ROWS]
ROWS_IDS = ["%s-%d" % (c.name, n) for c, n in ROWS_PARAMS]


# ---------------------------------------------------------------------------------------------------------------------
# restated dispatch (csrc/gw_kernels.hip: gw_edge_update_forward with a save; csrc/gw_edge.hip: edge_fast_eligible)
# ---------------------------------------------------------------------------------------------------------------------
def edge_training_route(dtype, modes: Sequence[str], n_mid: int, has_norm: bool, ln_width: int) -> str:
    """Forward kernel of a training edge update.  ``ln_width``: features the LayerNorm spans (256, or fewer in a narrow model)."""
    if dtype == BF16X3:
        return CHAINX3
    n_raw = sum(m == "raw" for m in modes)
    n_proj = sum(m == "proj" for m in modes)
    if n_raw <= 1 and n_proj >= 1 and n_mid == 1 and has_norm and ln_width == 256:
        return EDGE_KERNEL
    return CHAIN_EDGE


# ---------------------------------------------------------------------------------------------------------------------
# one fused op
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Feed:
    mode: str  # "zero" | "raw" | "proj"
    table: Optional[torch.Tensor]  # float32 [table rows, ld >= width]
    idx: Optional[torch.Tensor]  # int64 [n]: row of the sample's part of the table read by row k of the op
    rows_pb: int  # table rows per sample; 0 = one table shared by the batch
    width: int = 256  # feature columns of the table (ld above it: padding never to be read)
    k: int = 256  # leading columns that carry values (narrow models: 128; the rest is zero)
    grad: bool = True

    def features(self, dtype) -> torch.Tensor:
        return self.table[:, :self.width].to(dtype)


@dataclasses.dataclass
class Op:
    B: int
    n: int  # rows per sample
    feeds: List[Feed]
    splits: List[Tuple[int, int]]  # column block of W0 of every feed
    params: List[torch.Tensor]  # float32, model.parameters() order: W0, b0, ..., [gamma, beta]
    norm: bool
    res: Optional[Feed]
    res_is: Optional[int]  # the residual is the same tensor as this feed
    out_width: int  # columns of an output row (256 for tables: narrow outputs are zero padded; n_out for row MLPs)
    dst: Optional[torch.Tensor] = None  # int64 [n]: the edge update's segment sums
    n_dst: int = 0
    param_grad: bool = True
    ln_width: int = 0  # 0: LayerNorm over all outputs; else over the first ln_width (zero-padded parameters)

    @property
    def rows(self) -> int:
        return self.B * self.n

    @property
    def n_lin(self) -> int:
        return (len(self.params) - (2 if self.norm else 0)) // 2

    def names(self) -> List[str]:
        out = []
        for l in range(self.n_lin):
            out += ["W%d" % l, "b%d" % l]
        return out + (["gamma", "beta"] if self.norm else [])


def _gather(t: torch.Tensor, rows_pb: int, idx: torch.Tensor, B: int) -> torch.Tensor:
    """[B * n, w]: row idx[k] of every sample's part of a table (rows_pb == 0: of the one shared table)."""
    if rows_pb == 0:
        return t[idx].repeat(B, 1)
    return t.reshape(B, rows_pb, t.shape[1])[:, idx].reshape(B * idx.numel(), t.shape[1])


def _scatter(rows: torch.Tensor, feed: Feed, B: int) -> torch.Tensor:
    """Dual of ``_gather``: [table rows, w]; a shared table gets the sum over the batch."""
    n, w = feed.idx.numel(), rows.shape[1]
    n_tab = feed.rows_pb if feed.rows_pb else int(feed.table.shape[0])
    out = torch.zeros(B, n_tab, w, dtype=rows.dtype)
    out.index_add_(1, feed.idx, rows.reshape(B, n, w))
    return out.reshape(B * n_tab, w) if feed.rows_pb else out.sum(0)


def _pad(t: torch.Tensor, width: int) -> torch.Tensor:
    return t if t.shape[1] == width else torch.nn.functional.pad(t, (0, width - t.shape[1]))


def leaves(op: Op, dtype):
    """(parameters, feed tables, residual table) of the op in ``dtype``; the residual IS its feed's tensor where they are one."""
    P = [p.to(dtype) for p in op.params]
    T = [None if f.mode == "zero" else f.features(dtype) for f in op.feeds]
    R = None if op.res is None else (T[op.res_is] if op.res_is is not None else op.res.features(dtype))
    return P, T, R


def forward(op: Op, P, T, R, flips=None):
    """-> (rows [B * n, out_width], agg [B * n_dst, out_width] or None, hidden [relu outputs], pre_norm, pre-activations).
    ``flips[l]`` (bool, the shape of layer l's pre-activation): entries whose ReLU gate is the opposite of sign(z) - for the
    end-to-end reference where a kernel's gate differs on an entry under the margin, i.e. where z is zero to working precision
    and the derivative of ReLU is either value."""
    B, n_lin = op.B, op.n_lin
    W0, b0 = P[0], P[1]
    raw = [i for i, f in enumerate(op.feeds) if f.mode == "raw"]
    if raw:  # the reference's form: cat of the gathered rows -> Linear
        x = torch.cat([_gather(T[i], op.feeds[i].rows_pb, op.feeds[i].idx, B)[:, :op.feeds[i].k] for i in raw], 1)
        w = torch.cat([W0[:, op.splits[i][0]:op.splits[i][0] + op.feeds[i].k] for i in raw], 1)
        z = torch.nn.functional.linear(x, w, b0)
    else:
        z = b0[None].expand(op.rows, -1)
    for i, f in enumerate(op.feeds):
        if f.mode == "proj":
            z = z + _gather(T[i], f.rows_pb, f.idx, B)[:, :W0.shape[0]]
    def relu(z, l):
        return torch.relu(z) if flips is None or not bool(flips[l].any()) else z * ((z > 0) ^ flips[l])

    pre, hidden = [z], [relu(z, 0)]
    for l in range(1, n_lin - 1):
        z = torch.nn.functional.linear(hidden[-1], P[2 * l], P[2 * l + 1])
        pre.append(z)
        hidden.append(relu(z, l))
    y = torch.nn.functional.linear(hidden[-1], P[2 * n_lin - 2], P[2 * n_lin - 1])
    o = y
    if op.norm:
        lw = op.ln_width or int(y.shape[1])
        o = _pad(torch.nn.functional.layer_norm(y[:, :lw], (lw,), P[-2][:lw], P[-1][:lw], 1e-5), int(y.shape[1]))
    out = _pad(o, op.out_width)
    if R is not None:
        out = out + _gather(R, op.res.rows_pb, op.res.idx, B)[:, :op.out_width]
    agg = None
    if op.dst is not None:
        agg = torch.zeros(B, op.n_dst, op.out_width, dtype=out.dtype)
        agg = agg.index_add(1, op.dst, out.reshape(B, op.n, op.out_width)).reshape(B * op.n_dst, op.out_width)
    return out, agg, hidden, (y if op.norm else None), pre


def incoming(op: Op, dout: Optional[torch.Tensor], dagg: Optional[torch.Tensor], dtype) -> torch.Tensor:
    """Gradient at the op's output rows: the gather of the aggregate's gradient by destination (index_select backward of
    scatter_sum) plus the gradient of the exposed rows."""
    dn = torch.zeros(op.rows, op.out_width, dtype=dtype)
    if dagg is not None:
        dn = dn + dagg.to(dtype).reshape(op.B, op.n_dst, -1)[:, op.dst].reshape(op.rows, -1)
    if dout is not None:
        dn = dn + dout.to(dtype)
    return dn


def backward_from_saves(op: Op, hidden: Sequence[torch.Tensor], pre_norm: Optional[torch.Tensor], dout, dagg, dtype=F64) -> dict:
    """Every parameter and input gradient of the op by the formulas of autograd.py, from given saves (``hidden[l]``: the relu
    output of Linear_l, ``pre_norm``: the rows before LayerNorm), in ``dtype``.  Keys: W0, b0, ..., gamma, beta, op0.., res.  The
    gradient of a residual that is also a feed is NOT joined here: ``op<i>`` and ``res`` are its two uses."""
    P, T, _ = leaves(op, dtype)
    hidden = [h.to(dtype) for h in hidden]
    B, n_lin = op.B, op.n_lin
    dn = incoming(op, dout, dagg, dtype)
    g = {}
    if op.res is not None and op.res.grad:
        g["res"] = _scatter(_pad(dn, op.res.width) if op.res.width > op.out_width else dn, op.res, B)
    n_out = int(P[2 * n_lin - 2].shape[0])
    d = dn[:, :n_out]
    if op.norm:  # LayerNorm backward on the saved pre-norm rows
        lw = op.ln_width or n_out
        y, gamma, dl = pre_norm.to(dtype)[:, :lw], P[-2][:lw], d[:, :lw]
        mu = y.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + 1e-5)
        xhat = (y - mu) * rstd
        g["gamma"], g["beta"] = _pad((dl * xhat).sum(0)[None], n_out)[0], _pad(dl.sum(0)[None], n_out)[0]
        dxh = dl * gamma
        d = _pad(rstd * (dxh - dxh.mean(1, keepdim=True) - xhat * (dxh * xhat).mean(1, keepdim=True)), n_out)
    for l in range(n_lin - 1, 0, -1):
        g["W%d" % l] = d.t() @ hidden[l - 1]
        g["b%d" % l] = d.sum(0)
        d = (d @ P[2 * l]) * (hidden[l - 1] > 0)
    g["b0"] = d.sum(0)
    W0 = P[0]
    gW0 = torch.zeros_like(W0)  # (the block of a projected or absent operand stays zero: its gradient arrives through ProjectFunction)
    for i, f in enumerate(op.feeds):
        lo = op.splits[i][0]
        if f.mode == "raw":
            gW0[:, lo:lo + f.k] = d.t() @ _gather(T[i], f.rows_pb, f.idx, B)[:, :f.k]
            if f.grad:
                g["op%d" % i] = _scatter(_pad(d @ W0[:, lo:lo + f.k], f.width), f, B)
        elif f.mode == "proj" and f.grad:
            g["op%d" % i] = _scatter(_pad(d, f.width), f, B)
    g["W0"] = gW0
    if not op.param_grad:
        g = {k: v for k, v in g.items() if k.startswith("op") or k == "res"}
    return g


def autograd64(op: Op, dout, dagg, flips=None) -> dict:
    """The same gradients from torch's float64 autograd of the reference form (gates from float64; ``flips``: see ``forward``).
    A residual that is also a feed is ONE leaf: ``op<i>`` carries both uses and there is no ``res``."""
    P, T, R = leaves(op, F64)
    P = [p.requires_grad_(op.param_grad) for p in P]
    for i, f in enumerate(op.feeds):
        if T[i] is not None:
            T[i].requires_grad_(f.grad)
    if R is not None:
        if op.res_is is not None:
            R = T[op.res_is]
        else:
            R.requires_grad_(op.res.grad)
    out, agg, _, _, _ = forward(op, P, T, R, flips)
    wanted = {}
    if op.param_grad:
        wanted.update(zip(op.names(), P))
    wanted.update({"op%d" % i: t for i, t in enumerate(T) if t is not None and t.requires_grad})
    if R is not None and op.res_is is None and R.requires_grad:
        wanted["res"] = R
    outs, gs = [], []
    if dout is not None:
        outs.append(out)
        gs.append(dout.double())
    if dagg is not None:
        outs.append(agg)
        gs.append(dagg.double())
    got = torch.autograd.grad(outs, list(wanted.values()), gs, allow_unused=True)
    return {k: (v if v is not None else torch.zeros_like(t)) for (k, t), v in zip(wanted.items(), got)}


def joined(g: dict, op: Op) -> dict:
    """``backward_from_saves`` result with the two uses of a residual that is also a feed summed, as ``autograd64`` returns them."""
    if op.res_is is None or "res" not in g:
        return dict(g)
    out = {k: v for k, v in g.items() if k != "res"}
    key = "op%d" % op.res_is
    out[key] = out[key] + g["res"] if key in out else g["res"]
    return out


def margin_counts(pre: Sequence[torch.Tensor]):
    """(entries, entries with |z| < MARGIN * max |z| of their layer) over the float64 pre-activations."""
    total = sum(z.numel() for z in pre)
    inside = sum(int((z.abs() < MARGIN * z.abs().max()).sum()) for z in pre)
    return total, inside


def longest_sums(op: Op) -> dict:
    """K, the number of terms of the longest float32 sum behind every gradient (the floor 2^-24 sqrt(K) of a plain sum): the rows
    for a weight or bias gradient; the most rows that meet in one table row (x samples for a shared table) times the 256 terms of
    the row product for a raw operand; 256 for a row product alone."""
    K = {name: op.rows for name in op.names()}
    for i, f in enumerate(list(op.feeds) + [op.res]):
        if f is None or f.mode == "zero":
            continue
        deg = int(torch.bincount(f.idx).max()) * (op.B if f.rows_pb == 0 else 1)
        K["res" if i == len(op.feeds) else "op%d" % i] = deg * (256 if f.mode == "raw" and i < len(op.feeds) else 1)
    if op.res_is is not None:
        K["op%d" % op.res_is] += 1
    return K


def fp32_floor(k: int) -> float:
    return max(1e-6, 2.0 ** -24 * math.sqrt(k))


# ---------------------------------------------------------------------------------------------------------------------
# operands of the cases
# ---------------------------------------------------------------------------------------------------------------------
def make_params(rs, in_dim: int, hid: int, out: int, hidden_layers: int, norm: bool) -> List[torch.Tensor]:
    """Biases, gamma - 1 and beta of size 0.1: a constant read from the wrong place is far outside every bar."""
    dims = [in_dim] + [hid] * hidden_layers + [out]
    ps = []
    for i in range(len(dims) - 1):
        ps.append(torch.from_numpy((rs.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)))
        ps.append(torch.from_numpy((0.1 * rs.standard_normal(dims[i + 1])).astype(np.float32)))
    if norm:
        ps.append(torch.from_numpy((1 + 0.1 * rs.standard_normal(out)).astype(np.float32)))
        ps.append(torch.from_numpy((0.1 * rs.standard_normal(out)).astype(np.float32)))
    return ps


def make_table(rs, rows: int, k: int = 256, ld: int = 256) -> torch.Tensor:
    """[rows, ld]: k random features, zeros up to 256 (a narrow model's padded table), PAD_VALUE in the padding past 256."""
    t = torch.full((rows, ld), PAD_VALUE, dtype=F32)
    t[:, :256] = 0.0
    t[:, :k] = torch.from_numpy(rs.standard_normal((rows, k)).astype(np.float32))
    return t


def _seed(*parts) -> int:
    return sum(map(ord, "".join(map(str, parts))))


@functools.lru_cache(maxsize=None)
def edge_op(case: EdgeCase, gname: str):
    """(Op, output gradients (de_out or None, dagg)) of an edge-update case on a graph."""
    g = graph(gname)
    rs = np.random.RandomState(_seed("edge", case.name, gname) + case.seed)
    wid, hidden_layers, norm = MLPS[case.mlp]
    params = make_params(rs, 3 * wid, wid, wid, hidden_layers, norm)
    idx = (torch.from_numpy(g.src).long(), torch.from_numpy(g.dst).long(), torch.arange(g.E))
    n_tab = (g.n_src, g.n_dst, g.E)
    feeds = []
    for i in range(3):
        if case.modes[i] == "zero":
            feeds.append(Feed("zero", None, idx[i], 0, grad=False))
            continue
        rows_pb = 0 if case.shared[i] else n_tab[i]
        t = make_table(rs, n_tab[i] if case.shared[i] else g.B * n_tab[i], wid, LD if i in case.strided else 256)
        feeds.append(Feed(case.modes[i], t, idx[i], rows_pb, k=wid, grad=case.grads != "params"))
    if case.res == "e_in":
        res, res_is = dataclasses.replace(feeds[2], mode="raw"), 2
    else:
        shared = case.res == "shared"
        t = make_table(rs, g.E if shared else g.B * g.E, wid, LD if 3 in case.strided else 256)
        res, res_is = Feed("raw", t, idx[2], 0 if shared else g.E, k=wid, grad=case.grads != "params"), None
    op = Op(g.B, g.E, feeds, [(0, wid), (wid, 2 * wid), (2 * wid, 3 * wid)], params, norm, res, res_is, 256, idx[1], g.n_dst,
            param_grad=case.grads != "inputs")
    dagg = torch.from_numpy(rs.standard_normal((g.B * g.n_dst, 256)).astype(np.float32))
    de_out = torch.from_numpy(rs.standard_normal((g.B * g.E, 256)).astype(np.float32)) if case.want_edges else None
    return op, (de_out, dagg)


@functools.lru_cache(maxsize=None)
def node_op(case: NodeCase, n: int):
    rs = np.random.RandomState(_seed("node", case.name, n) + case.seed)
    wid, hidden_layers, norm = MLPS[case.mlp]
    params = make_params(rs, 2 * wid, wid, wid, hidden_layers, norm)
    ar = torch.arange(n)
    ld, live = (LD, False) if case.frozen_strided else (256, True)
    if case.x_mode == "zero":
        x = Feed("zero", None, ar, 0, grad=False)
    else:
        x = Feed(case.x_mode, make_table(rs, n if case.x_shared else case.B * n, wid, ld), ar, 0 if case.x_shared else n, k=wid,
                 grad=live)
    agg = Feed("raw", make_table(rs, case.B * n, wid, ld), ar, n, k=wid, grad=case.agg_grad)
    res = None
    if case.res is not None:
        shared = case.res == "shared"
        res = Feed("raw", make_table(rs, n if shared else case.B * n, wid, ld), ar, 0 if shared else n, k=wid, grad=live)
    op = Op(case.B, n, [x, agg], [(0, wid), (wid, 2 * wid)], params, norm, res, None, 256)
    dout = torch.from_numpy(rs.standard_normal((case.B * n, 256)).astype(np.float32))
    return op, (dout, None)


@functools.lru_cache(maxsize=None)
def rows_op(case: RowsCase, n: int):
    rs = np.random.RandomState(_seed("rows", case.name, n) + case.seed + ROWS_SEED_SHIFT.get((case.name, n), 0))
    params = make_params(rs, case.in_dim, case.hidden, case.out, 2, case.norm)
    ar = torch.arange(n)
    x = Feed("raw", make_table(rs, n, case.in_dim, case.in_dim) if case.in_dim < 256 else make_table(rs, n), ar, n,
             width=case.in_dim, k=case.in_dim)
    res = None
    if case.res_width is not None:
        res = Feed("raw", torch.from_numpy(rs.standard_normal((n, case.res_width)).astype(np.float32)), ar, n,
                   width=case.res_width, k=case.res_width)
    op = Op(1, n, [x], [(0, case.in_dim)], params, case.norm, res, None, case.out)
    dout = torch.from_numpy(rs.standard_normal((n, case.out)).astype(np.float32))
    return op, (dout, None)


# ---------------------------------------------------------------------------------------------------------------------
# ProjectFunction: out_s = x @ W0[:, lo_s:hi_s]^T (+ x itself as one more output)
# ---------------------------------------------------------------------------------------------------------------------
PROJECT_SPLITS = ((0, 256), (256, 512), (512, 768))


@functools.lru_cache(maxsize=None)
def project_operands(case: ProjectCase, n: int):
    """(x [n, 256], W0 [256, 768], douts per slice (None where unused), gradient of the passed-through x or None)."""
    rs = np.random.RandomState(_seed("project", case.name, n))
    W0 = torch.from_numpy((rs.standard_normal((256, 768)) / np.sqrt(768)).astype(np.float32))
    x = make_table(rs, n, 256, case.ld)
    douts = [None if i in case.unused else torch.from_numpy(rs.standard_normal((n, 256)).astype(np.float32))
             for i in range(len(case.slices))]
    dpass = torch.from_numpy(rs.standard_normal((n, 256)).astype(np.float32)) if case.passthrough else None
    return x, W0, douts, dpass


def project_forward(case: ProjectCase, x, W0):
    x = x[:, :256]
    return [x @ W0[:, lo:hi].t() for lo, hi in (PROJECT_SPLITS[s] for s in case.slices)]


def project_backward(case: ProjectCase, x, W0, douts, dpass, dtype=F64) -> dict:
    """dW0[:, lo:hi] = d^T x per used slice (zero elsewhere); dx = sum_s d_s W0[:, lo_s:hi_s] (+ the passed-through gradient)."""
    x, W0 = x[:, :256].to(dtype), W0.to(dtype)
    gW, dx = torch.zeros_like(W0), (dpass.to(dtype) if dpass is not None else None)
    for s, d in zip(case.slices, douts):
        if d is None:
            continue
        lo, hi = PROJECT_SPLITS[s]
        gW[:, lo:hi] += d.to(dtype).t() @ x
        if case.x_grad:
            dx = d.to(dtype) @ W0[:, lo:hi] + (dx if dx is not None else 0)
    g = {"W0": gW}
    if case.x_grad and dx is not None:
        g["x"] = dx
    return g


def project_autograd64(case: ProjectCase, x, W0, douts, dpass) -> dict:
    xd, Wd = x[:, :256].double().requires_grad_(case.x_grad), W0.double().requires_grad_(True)
    outs = project_forward(case, xd, Wd)
    pairs = [(o, d.double()) for o, d in zip(outs, douts) if d is not None]
    if dpass is not None and case.x_grad:
        pairs.append((xd * 1.0, dpass.double()))
    wanted = {"W0": Wd, **({"x": xd} if case.x_grad else {})}
    got = torch.autograd.grad([o for o, _ in pairs], list(wanted.values()), [d for _, d in pairs], allow_unused=True)
    return {k: (v if v is not None else torch.zeros_like(t)) for (k, t), v in zip(wanted.items(), got)}


# ---------------------------------------------------------------------------------------------------------------------
# calling the nodes themselves (graph_weather_amd is imported here, not at the top: the oracle above is plain torch)
# ---------------------------------------------------------------------------------------------------------------------
def module_for(kind: str, op: Op, mlp_name: str = "std", rows_case: Optional[RowsCase] = None, device="cpu", dtype=F32):
    """The project's MLP module of a case ("edge" | "node" | "rows") with the op's parameters loaded, on ``device``."""
    from graph_weather_amd import layers

    if kind == "rows":
        m = layers.MLP(rows_case.in_dim, rows_case.out, rows_case.hidden, 2, "LayerNorm" if rows_case.norm else None)
    else:
        wid, hidden_layers, norm = MLPS[mlp_name]
        maker = layers.EdgeProcessor if kind == "edge" else layers.NodeProcessor
        proc = maker(wid, wid, wid, hidden_layers, "LayerNorm" if norm else None)
        m = proc.edge_mlp if kind == "edge" else proc.node_mlp
    ps = list(m.model.parameters())
    assert [tuple(p.shape) for p in ps] == [tuple(v.shape) for v in op.params]
    with torch.no_grad():
        for p, v in zip(ps, op.params):
            p.copy_(v)
    m = m.to(device)
    layers.set_compute_dtype(m, dtype)
    for p in m.parameters():
        p.requires_grad_(op.param_grad)
    return m


def device_tables(op: Op, device):
    """(feed tensors, residual tensor) on ``device`` as the nodes take them: leaves that require a gradient where the case says so
    (those are 256 wide: a gradient has its tensor's shape), the residual the SAME tensor as its feed where they are one."""
    ts = [None if f.mode == "zero" else f.table.to(device).requires_grad_(f.grad) for f in op.feeds]
    res = None
    if op.res is not None:
        res = ts[op.res_is] if op.res_is is not None else op.res.table.to(device).requires_grad_(op.res.grad)
    return ts, res


def call_edge(case: EdgeCase, gname: str, op: Op, mlp, device):
    from graph_weather_amd import autograd as ag
    from graph_weather_amd.graphs import GraphPlan

    g = graph(gname)
    plan = GraphPlan(g.n_src, g.n_dst, torch.from_numpy(g.src), torch.from_numpy(g.dst), torch.arange(g.E), None).to(device)
    ts, res = device_tables(op, device)
    specs = [ag.OperandSpec(f.mode, f.rows_pb) for f in op.feeds]
    agg, e_out = ag.edge_update(mlp, plan, op.B, specs, case.want_edges, ts[0], ts[1], ts[2], res, op.res.rows_pb)
    inputs = {"op%d" % i: t for i, t in enumerate(ts) if t is not None}
    if op.res_is is None:
        inputs["res"] = res
    return {"agg": agg, "rows": e_out}, inputs, agg.grad_fn


def call_node(case: NodeCase, op: Op, mlp, device):
    from graph_weather_amd import autograd as ag

    ts, res = device_tables(op, device)
    x = op.feeds[0]
    out = ag.node_update(mlp, op.rows, op.n, ag.OperandSpec(x.mode, x.rows_pb), ts[0], res, 0 if op.res is None else op.res.rows_pb, ts[1])
    inputs = {"op%d" % i: t for i, t in enumerate(ts) if t is not None}
    if res is not None:
        inputs["res"] = res
    return {"rows": out}, inputs, out.grad_fn


def call_rows(case: RowsCase, op: Op, mlp, device):
    from graph_weather_amd import autograd as ag
    from graph_weather_amd.ops import Operand

    ts, res = device_tables(op, device)
    x2 = ts[0]
    if mlp.native_k() > x2.shape[1]:  # (as MLP.run: zero columns up to the kernel's input width, a differentiable pad)
        x2 = torch.nn.functional.pad(x2, (0, mlp.native_k() - x2.shape[1]))
    rop = None if res is None else Operand(res, op.res.rows_pb, int(res.shape[1]))
    out = ag.mlp_rows(mlp, x2, op.rows, op.n, residual_op=rop)
    inputs = {"op0": ts[0]}
    if res is not None:
        inputs["res"] = res
    return {"rows": out}, inputs, out.grad_fn


def node_grads(outs: dict, douts, mlp, op: Op, inputs: dict) -> dict:
    """torch.autograd.grad through the node: {name: gradient or None} for the module's parameters and every input that requires
    one.  The graph is kept (``raw_backward`` may follow)."""
    dout, dagg = douts
    pairs = [(outs["rows"], dout)] if dout is not None else []
    if dagg is not None:
        pairs.append((outs["agg"], dagg))
    dev = pairs[0][0].device
    wanted = dict(zip(op.names(), mlp.model.parameters())) if op.param_grad else {}
    wanted.update({k: t for k, t in inputs.items() if t.requires_grad})
    got = torch.autograd.grad([o for o, _ in pairs], list(wanted.values()), [d.to(dev) for _, d in pairs], allow_unused=True,
                              retain_graph=True)
    return dict(zip(wanted, got))


def raw_backward(fn, *douts):
    """What the Function's ``backward`` itself returns for these output gradients (Nones included)."""
    with torch.no_grad():  # (as the autograd engine runs it)
        return fn._forward_cls.backward(fn, *douts)


def run_project(case, n, device, dtype):
    """``ag.project`` on a case: ({outputs and gradients}, {their float64 references}, backward's own result)."""
    from graph_weather_amd import autograd as ag

    x, W0, douts, dpass = project_operands(case, n)
    params = list(edge_op(EDGE_CASES[0], "G1")[0].params)  # (an edge MLP; only its W0 matters here)
    params[0] = W0
    op = Op(1, n, [], [], params, True, None, None, 256)
    mlp = module_for("edge", op, "std", device=device, dtype=dtype)
    xd = x.to(device).requires_grad_(case.x_grad)
    outs = ag.project(mlp, case.slices, xd, n, n, passthrough=case.passthrough)
    assert len(outs) == len(case.slices) + (1 if case.passthrough else 0)
    got = {"out%d" % i: o for i, o in enumerate(outs[:len(case.slices)])}
    want = {"out%d" % i: o for i, o in enumerate(project_forward(case, x.double(), W0.double()))}
    if case.passthrough:
        assert outs[-1].data_ptr() == xd.data_ptr()  # x itself, not a copy
    pairs = [(o, d.to(device)) for o, d in zip(outs, douts) if d is not None]
    if case.passthrough:
        pairs.append((outs[-1], dpass.to(device)))
    wanted = {"W0": mlp.model[0].weight, **({"x": xd} if case.x_grad else {})}
    gs = torch.autograd.grad([o for o, _ in pairs], list(wanted.values()), [d for _, d in pairs], retain_graph=True)
    got.update(zip(wanted, gs))
    want.update(project_autograd64(case, x, W0, douts, dpass))
    fn = outs[0].grad_fn
    raw = raw_backward(fn, *[None if d is None else d.to(device) for d in douts], *([dpass.to(device)] if case.passthrough else []))
    return got, want, raw
