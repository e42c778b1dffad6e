"""The GenCast layers of the reference (``graph_weather/models/gencast/layers``): ``MLP``, ``InteractionNetwork``,
``FourierEmbedding``, ``ConditionalLayerNorm``, ``CondTransformerBlock``, ``Encoder``, ``Processor`` and ``Decoder``; the blocks of
``Processor(sparse="native")`` are in ``gencast_sparse``.

Same constructor arguments, defaults, argument checks, attribute names and ``state_dict`` keys (and their order) as the
reference.  The reference builds on two ``torch_geometric`` classes; here ``TransformerConv`` is a parameter holder with PyG's
key names (``lin_key``, ``lin_query``, ``lin_value``, ``lin_edge``, ``lin_skip``, ``lin_beta``) and ``InteractionNetwork`` is a
plain module - their arithmetic is restated from PyG's documentation, not pinned against PyG.

The mesh processor's attention over the incoming edges of every node is one launch of ``csrc/gw_gencast.hip`` that walks the
destination-sorted edge list with an online softmax: nothing of size E x heads x C is written (PyG gathers ``k[src]`` and
``v[src]`` into such temporaries and saves them for autograd); its backward recomputes the probabilities in one launch over
destinations (dq, de) and one over sources (dk, dv).  ConditionalLayerNorm (+ activation), the beta gate, SiLU and the Fourier
features are row kernels of the same file; Linear, LayerNorm, ReLU, adds, row gathers and segment sums are the library's
existing kernels with the ordered (atomic-free) weight gradients of the Aurora path, so every result and gradient is bitwise
reproducible.  The ``cat(x_i, x_j, edge_attr)`` of the interaction network is never formed: layer 1 is split into two
node-level products gathered in the epilogue of the edge-level product (``gw_linear_gather_forward``).

``edge_index`` arrives per call ([2, E] int64 COO, any order, duplicates are separate edges); it is sorted by destination once
per tensor and cached on (address, shape, version).  fp32 only, no dropout, no bf16 modes; there is no CPU path.

Batch-shared form (what ``gencast_model.Denoiser`` runs): the reference batches by replicating the graph - B disconnected copies,
``edge_index`` and ``edge_attr`` concatenated B times - so every product on edge attributes alone and every conditioning row is
computed B times over.  ``Encoder._forward_shared``, ``Processor._forward_shared`` and ``Decoder._forward_shared`` take ONE graph
and node rows [B n, .]: the attention, ConditionalLayerNorm and gather kernels index copy b's node rows at b n and read one edge
table, one plan and one conditioning row per sample.  The public ``forward``s are unchanged.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .aurora import _ln, _Relu, _RowScale, _workspace
from .aurora import gemm_tn_ordered as _gemm_tn_ordered
from .fengwu_ghr import _need_hip
from .graphs import GraphPlan
from .layers import _ver
from .ops import on_device_of
from .wide import _Add, _L, _ld, _rows, _st, add_rows, linear_forward, linear_gather_forward, segment_sum_rows

__all__ = ["MLP", "InteractionNetwork", "FourierEmbedding", "ConditionalLayerNorm", "CondTransformerBlock", "TransformerConv",
           "Encoder", "Processor", "Decoder", "EdgePlan", "edge_plan", "graph_attention_forward", "graph_attention_backward",
           "cond_layernorm_forward", "cond_layernorm_backward", "beta_gate_forward", "beta_gate_backward", "silu_forward",
           "silu_backward", "fourier_forward", "fourier_backward", "graph_attention_batched_forward",
           "graph_attention_batched_backward", "edge_table_stride", "cond_layernorm_grouped_forward",
           "cond_layernorm_grouped_backward", "precond_input_forward", "precond_input_backward", "precond_output_forward",
           "precond_output_backward"]

MAX_ROW = 4096  # heads * dim_head of the graph attention kernels


# ---------------------------------------------------------------------------------------------------------------------
# graph plans
# ---------------------------------------------------------------------------------------------------------------------
class EdgePlan:
    """Index structures of one COO ``edge_index`` on the device: the destination-sorted ``GraphPlan`` (``dst_ptr``, ``src``,
    ``perm``, ``src_sorted``) the attention kernels walk, and - for the interaction network, whose edge-level rows stay in the
    caller's edge order - the edge ids grouped by destination (``perm32`` with ``plan.dst_ptr()``) and by source
    (``by_src``)."""

    def __init__(self, edge_index: torch.Tensor, n_src: int, n_dst: int):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise RuntimeError("graph_weather_amd: edge_index must be an int64 [2, E] tensor in COO format")
        E = int(edge_index.shape[1])
        if max(E, n_src, n_dst) >= 2 ** 31 - 1:
            raise RuntimeError("graph_weather_amd: graph too large for int32 plans")
        src, dst = edge_index[0], edge_index[1]
        if E and (int(src.min()) < 0 or int(src.max()) >= n_src or int(dst.min()) < 0 or int(dst.max()) >= n_dst):
            raise IndexError("edge_index refers to nodes outside the node tables (n_src = %d, n_dst = %d)" % (n_src, n_dst))
        dst_sorted, perm = torch.sort(dst, stable=True)
        self.plan = GraphPlan(n_src, n_dst, src[perm].to(torch.int32).contiguous(), dst_sorted.to(torch.int32).contiguous(),
                              perm.contiguous(), None)
        self.plan.dst_ptr()
        self.plan.src_sorted()
        self.num_edges, self.n_src, self.n_dst = E, n_src, n_dst
        self.src32, self.dst32 = src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous()  # caller's edge order
        self.perm32 = perm.to(torch.int32).contiguous()
        by_src = torch.argsort(src, stable=True)
        counts = torch.bincount(src, minlength=n_src)
        self.by_src = (by_src.to(torch.int32).contiguous(), torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32))
        self.ident_dst = torch.arange(n_dst + 1, dtype=torch.int32, device=edge_index.device)


_PLANS: list = []  # the last few (key, edge_index, EdgePlan); the entry holds the tensor, so its address cannot be recycled


def edge_plan(edge_index: torch.Tensor, n_src: int, n_dst: int) -> EdgePlan:
    """The ``EdgePlan`` of an ``edge_index`` tensor: built once per (address, shape, version, table sizes)."""
    if not edge_index.is_cuda:
        raise RuntimeError("graph_weather_amd: edge_index must live on a HIP device (no CPU path exists)")
    key = (edge_index.data_ptr(), tuple(edge_index.shape), _ver(edge_index), int(n_src), int(n_dst))
    for k, held, plan in _PLANS:
        if k == key and held is edge_index:
            return plan
    plan = EdgePlan(edge_index, int(n_src), int(n_dst))
    _PLANS.append((key, edge_index, plan))
    del _PLANS[:-8]
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _check_attention(heads: int, dim_head: int) -> None:
    if heads < 1 or dim_head < 1:
        raise ValueError("graph attention needs heads >= 1 and dim_head >= 1")
    if heads * dim_head > MAX_ROW:
        raise NotImplementedError("graph_weather_amd: the graph attention kernels take heads * dim_head <= %d, got %d x %d"
                                  % (MAX_ROW, heads, dim_head))


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def graph_attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor], plan: GraphPlan,
                            heads: int, mean: bool, keep_heads: bool = True):
    """Attention over the incoming edges of every destination row (include/gw_amd.h: gw_graph_attention_forward): q [n_dst, H C]
    (views with a row stride are read in place), k, v [n_src, H C], e [E, H C] in the caller's edge order or None ->
    (out [n_dst, H C], or [n_dst, C] with ``mean``; the per-head rows [n_dst, H C] the backward needs (``out`` itself without
    ``mean``, None with ``keep_heads`` False); lse [2, n_dst * H])."""
    q, k, v = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
    hc = int(q.shape[1])
    if hc % heads:
        raise RuntimeError("graph_weather_amd: the width of q (%d) is no multiple of the heads (%d)" % (hc, heads))
    C = hc // heads
    _check_attention(heads, C)
    E, nd, ns = plan.num_edges, plan.n_dst, plan.n_src
    if tuple(q.shape) != (nd, hc) or tuple(k.shape) != (ns, hc) or tuple(v.shape) != (ns, hc):
        raise RuntimeError("graph_weather_amd: graph attention expects q [%d, %d] and k, v [%d, %d], got %s, %s, %s"
                           % (nd, hc, ns, hc, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    if e is not None:
        e = _rows(e, "edge features")
        if tuple(e.shape) != (E, hc):
            raise RuntimeError("graph_weather_amd: graph attention expects edge features [%d, %d], got %s" % (E, hc, tuple(e.shape)))
    # (0 edges: the library launches nothing; every output row is then the zero this fill leaves)
    new = torch.zeros if E == 0 else torch.empty
    out = new((nd, C if mean else hc), dtype=torch.float32, device=q.device)
    out_heads = new((nd, hc), dtype=torch.float32, device=q.device) if (mean and keep_heads) else None
    lse = new((2, nd * heads), dtype=torch.float32, device=q.device)
    with on_device_of(out):
        _lib.check(_L().gw_graph_attention_forward(nd, ns, E, heads, C, plan.dst_ptr().data_ptr(), plan.src.data_ptr(),
                                                   plan.perm.data_ptr(), q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(),
                                                   _ld(v), _p(e), 0 if e is None else _ld(e), 1 if mean else 0, out.data_ptr(),
                                                   _ld(out), _p(out_heads), hc, lse.data_ptr(), _st(out)),
                   "gw_graph_attention_forward")
    return out, (out_heads if mean else out), lse


def graph_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor], plan: GraphPlan,
                             heads: int, mean: bool, out_heads: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor,
                             want_de: bool = True):
    """(dq, dk, dv, de or None) of ``graph_attention_forward``, dense rows."""
    q, k, v, out_heads, dout = _rows(q, "q"), _rows(k, "k"), _rows(v, "v"), _rows(out_heads, "out"), _rows(dout, "dout")
    hc = int(q.shape[1])
    C = hc // heads
    E, nd, ns = plan.num_edges, plan.n_dst, plan.n_src
    if e is not None:
        e = _rows(e, "edge features")
    new = torch.zeros if E == 0 else torch.empty
    dq = new((nd, hc), dtype=torch.float32, device=q.device)
    dk, dv = new((ns, hc), dtype=torch.float32, device=q.device), new((ns, hc), dtype=torch.float32, device=q.device)
    de = new((E, hc), dtype=torch.float32, device=q.device) if (e is not None and want_de) else None
    delta = torch.empty((max(nd * heads, 1),), dtype=torch.float32, device=q.device)
    src_pos, src_ptr = plan.src_sorted()
    with on_device_of(dq):
        _lib.check(_L().gw_graph_attention_backward(nd, ns, E, heads, C, plan.dst_ptr().data_ptr(), plan.src.data_ptr(),
                                                    plan.dst.data_ptr(), plan.perm.data_ptr(), src_pos.data_ptr(), src_ptr.data_ptr(),
                                                    q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), _p(e),
                                                    0 if e is None else _ld(e), 1 if mean else 0, out_heads.data_ptr(), _ld(out_heads),
                                                    dout.data_ptr(), _ld(dout), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), hc,
                                                    dk.data_ptr(), hc, dv.data_ptr(), hc, _p(de), hc, _st(dq)),
                   "gw_graph_attention_backward")
    return dq, dk, dv, de


_ACT_CODE = {None: _lib.ACT_NONE, "relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU}


def cond_layernorm_forward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, act: Optional[str] = None) -> torch.Tensor:
    """act(scale[r] * LayerNorm(x[r]) + bias[r]) (no affine, eps 1e-5); act None, "relu" or "silu"."""
    x, scale, bias = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias")
    if scale.shape != x.shape or bias.shape != x.shape:
        raise RuntimeError("graph_weather_amd: scale and bias must be shaped like x %s, got %s and %s"
                           % (tuple(x.shape), tuple(scale.shape), tuple(bias.shape)))
    rows, width = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((rows, width), dtype=torch.float32, device=x.device)
    with on_device_of(out):
        _lib.check(_L().gw_cond_layernorm_forward(rows, width, _ACT_CODE[act], x.data_ptr(), _ld(x), scale.data_ptr(), _ld(scale),
                                                  bias.data_ptr(), _ld(bias), out.data_ptr(), width, _st(out)),
                   "gw_cond_layernorm_forward")
    return out


def cond_layernorm_backward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, act: Optional[str], dout: torch.Tensor):
    """(dx, dscale, dbias) of ``cond_layernorm_forward``."""
    x, scale, bias, dout = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias"), _rows(dout, "dout")
    rows, width = int(x.shape[0]), int(x.shape[1])
    dx, dscale, dbias = (torch.empty((rows, width), dtype=torch.float32, device=x.device) for _ in range(3))
    with on_device_of(dx):
        _lib.check(_L().gw_cond_layernorm_backward(rows, width, _ACT_CODE[act], x.data_ptr(), _ld(x), scale.data_ptr(), _ld(scale),
                                                   bias.data_ptr(), _ld(bias), dout.data_ptr(), _ld(dout), dx.data_ptr(), width,
                                                   dscale.data_ptr(), dbias.data_ptr(), width, _st(dx)),
                   "gw_cond_layernorm_backward")
    return dx, dscale, dbias


def beta_gate_forward(out: torch.Tensor, x_r: torch.Tensor, w: torch.Tensor):
    """g = sigmoid(w . cat(out, x_r, out - x_r)), y = g x_r + (1 - g) out; w = lin_beta.weight [1, 3 width] -> (y, g [rows])."""
    out, x_r = _rows(out, "out"), _rows(x_r, "x_r")
    rows, width = int(out.shape[0]), int(out.shape[1])
    w = w.contiguous()
    if x_r.shape != out.shape or w.numel() != 3 * width:
        raise RuntimeError("graph_weather_amd: the beta gate expects x_r shaped like out %s and 3 x %d weights, got %s and %d"
                           % (tuple(out.shape), width, tuple(x_r.shape), w.numel()))
    y = torch.empty((rows, width), dtype=torch.float32, device=out.device)
    gate = torch.empty((rows,), dtype=torch.float32, device=out.device)
    with on_device_of(y):
        _lib.check(_L().gw_beta_gate_forward(rows, width, out.data_ptr(), _ld(out), x_r.data_ptr(), _ld(x_r), w.data_ptr(), y.data_ptr(),
                                             width, gate.data_ptr(), _st(y)), "gw_beta_gate_forward")
    return y, gate


def beta_gate_backward(out: torch.Tensor, x_r: torch.Tensor, w: torch.Tensor, gate: torch.Tensor, dy: torch.Tensor):
    """(d_out, d_x_r, dw shaped like w) of ``beta_gate_forward``."""
    out, x_r, dy = _rows(out, "out"), _rows(x_r, "x_r"), _rows(dy, "dy")
    rows, width = int(out.shape[0]), int(out.shape[1])
    w = w.contiguous()
    d_out, d_xr = (torch.empty((rows, width), dtype=torch.float32, device=out.device) for _ in range(2))
    dw = torch.zeros_like(w)
    if rows:
        nbytes = int(_L().gw_beta_gate_workspace_bytes(rows, width))
        ws = _workspace(nbytes, "gw_beta_gate_workspace_bytes", out.device)
        with on_device_of(dw):
            _lib.check(_L().gw_beta_gate_backward(rows, width, out.data_ptr(), _ld(out), x_r.data_ptr(), _ld(x_r), w.data_ptr(),
                                                  gate.data_ptr(), dy.data_ptr(), _ld(dy), ws.data_ptr(), nbytes, d_out.data_ptr(),
                                                  d_xr.data_ptr(), width, dw.data_ptr(), _st(dw)), "gw_beta_gate_backward")
    return d_out, d_xr, dw


def silu_forward(x: torch.Tensor) -> torch.Tensor:
    _need_hip(x, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    with on_device_of(y):
        _lib.check(_L().gw_silu_forward(x.numel(), x.data_ptr(), y.data_ptr(), _st(y)), "gw_silu_forward")
    return y


def silu_backward(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    x, dy = x.contiguous(), dy.contiguous()
    dx = torch.empty_like(x)
    with on_device_of(dx):
        _lib.check(_L().gw_silu_backward(x.numel(), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), _st(dx)), "gw_silu_backward")
    return dx


def fourier_forward(t: torch.Tensor, num_frequencies: int, base_period: float) -> torch.Tensor:
    """t [rows, 1] -> [rows, 2 F]: cos(t f_i) then sin(t f_i), f_i = exp(-ln(base_period) i / F)."""
    _need_hip(t, "t")
    if t.dim() != 2 or t.shape[1] != 1:
        raise RuntimeError("graph_weather_amd: the Fourier features take t [rows, 1], got %s" % (tuple(t.shape),))
    t = t.contiguous()
    rows = int(t.shape[0])
    out = torch.empty((rows, 2 * num_frequencies), dtype=torch.float32, device=t.device)
    with on_device_of(out):
        _lib.check(_L().gw_fourier_forward(rows, num_frequencies, float(base_period), t.data_ptr(), out.data_ptr(), 2 * num_frequencies,
                                           _st(out)), "gw_fourier_forward")
    return out


def fourier_backward(t: torch.Tensor, dout: torch.Tensor, num_frequencies: int, base_period: float) -> torch.Tensor:
    t, dout = t.contiguous(), _rows(dout, "dout")
    dt = torch.empty_like(t)
    with on_device_of(dt):
        _lib.check(_L().gw_fourier_backward(int(t.shape[0]), num_frequencies, float(base_period), t.data_ptr(), dout.data_ptr(), _ld(dout),
                                            dt.data_ptr(), _st(dt)), "gw_fourier_backward")
    return dt


# ---- batch-shared forms -------------------------------------------------------------------------------------------------
def edge_table_stride(e_rows: Optional[int], num_edges: int, batch: int) -> int:
    """The rows between two copies' edge tables for a table of ``e_rows`` rows (None: no table): 0 - one table [E, .] read by
    every copy - or E - one table per copy, [batch E, .].  With one copy the two coincide (0)."""
    if e_rows is None or e_rows == num_edges:
        return 0
    if e_rows == batch * num_edges:
        return num_edges
    raise RuntimeError("graph_weather_amd: batch-shared graph attention takes edge features with %d rows (shared) or %d (one table "
                       "per copy), got %d" % (num_edges, batch * num_edges, e_rows))


def graph_attention_batched_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor], plan: GraphPlan,
                                    heads: int, mean: bool, batch: int, keep_heads: bool = True):
    """``graph_attention_forward`` on ``batch`` copies of the plan's graph (include/gw_amd.h: gw_graph_attention_batched_forward):
    q [batch n_dst, H C], k, v [batch n_src, H C]; e [E, H C] shared by the copies, [batch E, H C] one table per copy, or None ->
    (out, per-head rows, lse [2, batch n_dst H])."""
    q, k, v = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
    hc = int(q.shape[1])
    if batch < 1 or hc % heads:
        raise RuntimeError("graph_weather_amd: batch-shared graph attention needs batch >= 1 and a width of q (%d) that is a multiple "
                           "of the heads (%d)" % (hc, heads))
    C = hc // heads
    _check_attention(heads, C)
    E, nd, ns = plan.num_edges, plan.n_dst, plan.n_src
    if tuple(q.shape) != (batch * nd, hc) or tuple(k.shape) != (batch * ns, hc) or tuple(v.shape) != (batch * ns, hc):
        raise RuntimeError("graph_weather_amd: batch-shared graph attention expects q [%d, %d] and k, v [%d, %d], got %s, %s, %s"
                           % (batch * nd, hc, batch * ns, hc, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    if e is not None:
        e = _rows(e, "edge features")
        if int(e.shape[1]) != hc:
            raise RuntimeError("graph_weather_amd: graph attention expects edge features %d wide, got %d" % (hc, int(e.shape[1])))
    stride = edge_table_stride(None if e is None else int(e.shape[0]), E, batch)
    new = torch.zeros if E == 0 else torch.empty
    out = new((batch * nd, C if mean else hc), dtype=torch.float32, device=q.device)
    out_heads = new((batch * nd, hc), dtype=torch.float32, device=q.device) if (mean and keep_heads) else None
    lse = new((2, batch * nd * heads), dtype=torch.float32, device=q.device)
    with on_device_of(out):
        _lib.check(_L().gw_graph_attention_batched_forward(
            batch, stride, nd, ns, E, heads, C, plan.dst_ptr().data_ptr(), plan.src.data_ptr(), plan.perm.data_ptr(), q.data_ptr(),
            _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), _p(e), 0 if e is None else _ld(e), 1 if mean else 0, out.data_ptr(),
            _ld(out), _p(out_heads), hc, lse.data_ptr(), _st(out)), "gw_graph_attention_batched_forward")
    return out, (out_heads if mean else out), lse


def graph_attention_batched_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: Optional[torch.Tensor], plan: GraphPlan,
                                     heads: int, mean: bool, batch: int, out_heads: torch.Tensor, lse: torch.Tensor,
                                     dout: torch.Tensor, want_de: bool = True):
    """(dq, dk, dv, de or None) of ``graph_attention_batched_forward``; de is shaped like e - for a shared table the sum over the
    copies in copy order."""
    q, k, v, out_heads, dout = _rows(q, "q"), _rows(k, "k"), _rows(v, "v"), _rows(out_heads, "out"), _rows(dout, "dout")
    hc = int(q.shape[1])
    C = hc // heads
    E, nd, ns = plan.num_edges, plan.n_dst, plan.n_src
    if e is not None:
        e = _rows(e, "edge features")
    stride = edge_table_stride(None if e is None else int(e.shape[0]), E, batch)
    new = torch.zeros if E == 0 else torch.empty
    dq = new((batch * nd, hc), dtype=torch.float32, device=q.device)
    dk, dv = (new((batch * ns, hc), dtype=torch.float32, device=q.device) for _ in range(2))
    de = new((int(e.shape[0]), hc), dtype=torch.float32, device=q.device) if (e is not None and want_de) else None
    delta = torch.empty((max(batch * nd * heads, 1),), dtype=torch.float32, device=q.device)
    src_pos, src_ptr = plan.src_sorted()
    with on_device_of(dq):
        _lib.check(_L().gw_graph_attention_batched_backward(
            batch, stride, nd, ns, E, heads, C, plan.dst_ptr().data_ptr(), plan.src.data_ptr(), plan.dst.data_ptr(),
            plan.perm.data_ptr(), src_pos.data_ptr(), src_ptr.data_ptr(), q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(),
            _ld(v), _p(e), 0 if e is None else _ld(e), 1 if mean else 0, out_heads.data_ptr(), _ld(out_heads), dout.data_ptr(),
            _ld(dout), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), hc, dk.data_ptr(), hc, dv.data_ptr(), hc, _p(de), hc, _st(dq)),
            "gw_graph_attention_batched_backward")
    return dq, dk, dv, de


def _group_rows(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_group: int) -> int:
    rows, width = int(x.shape[0]), int(x.shape[1])
    groups = -(-rows // rows_per_group) if rows_per_group >= 1 else -1
    if rows_per_group < 1 or tuple(scale.shape) != (groups, width) or tuple(bias.shape) != (groups, width):
        raise RuntimeError("graph_weather_amd: %d rows in groups of %d need scale and bias [%d, %d], got %s and %s"
                           % (rows, rows_per_group, groups, width, tuple(scale.shape), tuple(bias.shape)))
    return groups


def cond_layernorm_grouped_forward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_group: int,
                                   act: Optional[str] = None) -> torch.Tensor:
    """``cond_layernorm_forward`` with one scale and bias row per ``rows_per_group`` consecutive rows of x."""
    x, scale, bias = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias")
    _group_rows(x, scale, bias, rows_per_group)
    rows, width = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((rows, width), dtype=torch.float32, device=x.device)
    with on_device_of(out):
        _lib.check(_L().gw_cond_layernorm_grouped_forward(rows, width, _ACT_CODE[act], rows_per_group, x.data_ptr(), _ld(x),
                                                          scale.data_ptr(), _ld(scale), bias.data_ptr(), _ld(bias), out.data_ptr(), width,
                                                          _st(out)), "gw_cond_layernorm_grouped_forward")
    return out


def cond_layernorm_grouped_backward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_group: int, act: Optional[str],
                                    dout: torch.Tensor):
    """(dx, dscale [groups, width], dbias [groups, width]) of ``cond_layernorm_grouped_forward``."""
    x, scale, bias, dout = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias"), _rows(dout, "dout")
    groups = _group_rows(x, scale, bias, rows_per_group)
    rows, width = int(x.shape[0]), int(x.shape[1])
    dx = torch.empty((rows, width), dtype=torch.float32, device=x.device)
    dscale, dbias = (torch.zeros((groups, width), dtype=torch.float32, device=x.device) for _ in range(2))
    if rows:
        nbytes = int(_L().gw_cond_layernorm_grouped_workspace_bytes(rows, width, rows_per_group))
        ws = _workspace(nbytes, "gw_cond_layernorm_grouped_workspace_bytes", x.device)
        with on_device_of(dx):
            _lib.check(_L().gw_cond_layernorm_grouped_backward(rows, width, _ACT_CODE[act], rows_per_group, x.data_ptr(), _ld(x),
                                                               scale.data_ptr(), _ld(scale), bias.data_ptr(), _ld(bias), dout.data_ptr(),
                                                               _ld(dout), ws.data_ptr(), nbytes, dx.data_ptr(), width, dscale.data_ptr(),
                                                               dbias.data_ptr(), width, _st(dx)), "gw_cond_layernorm_grouped_backward")
    return dx, dscale, dbias


def _sigma_rows(sigma: torch.Tensor, rows: int, what: str):
    _need_hip(sigma, "noise_levels")
    sigma = sigma.reshape(-1).contiguous()
    batch = int(sigma.numel())
    if sigma.dtype != torch.float32 or batch < 1 or rows % batch:
        raise RuntimeError("graph_weather_amd: %s needs float32 noise levels, one per sample, and rows that split evenly among them "
                           "(%d rows, %d levels)" % (what, rows, batch))
    return sigma, batch, rows // batch


def precond_input_forward(z: torch.Tensor, x: torch.Tensor, sigma: torch.Tensor, static: torch.Tensor, sigma_data: float = 1.0):
    """The encoder's grid input rows and the scaled noise levels: (c_in(sigma_b) z | x | static[g]) for row b G + g, z [B G, wz],
    x [B G, wx], static [G, ws], sigma [B] or [B, 1] -> ([B G, wz + wx + ws], c_noise [B, 1])."""
    z, x, static = _rows(z, "corrupted targets"), _rows(x, "previous inputs"), _rows(static, "static grid features")
    sigma, batch, G = _sigma_rows(sigma, int(z.shape[0]), "the input preconditioning")
    if int(x.shape[0]) != batch * G or int(static.shape[0]) != G:
        raise RuntimeError("graph_weather_amd: the input preconditioning expects %d rows of previous inputs and %d static rows, got %d "
                           "and %d" % (batch * G, G, int(x.shape[0]), int(static.shape[0])))
    wz, wx, ws = int(z.shape[1]), int(x.shape[1]), int(static.shape[1])
    out = torch.empty((batch * G, wz + wx + ws), dtype=torch.float32, device=z.device)
    c_noise = torch.empty((batch, 1), dtype=torch.float32, device=z.device)
    with on_device_of(out):
        _lib.check(_L().gw_gencast_precond_input_forward(batch, G, wz, wx, ws, float(sigma_data), sigma.data_ptr(), z.data_ptr(), _ld(z),
                                                         x.data_ptr(), _ld(x), static.data_ptr(), _ld(static), out.data_ptr(),
                                                         wz + wx + ws, c_noise.data_ptr(), _st(out)), "gw_gencast_precond_input_forward")
    return out, c_noise


def precond_input_backward(dout: torch.Tensor, sigma: torch.Tensor, wz: int, wx: int, sigma_data: float = 1.0):
    """(dz, dx) of ``precond_input_forward``."""
    dout = _rows(dout, "dout")
    sigma, batch, G = _sigma_rows(sigma, int(dout.shape[0]), "the input preconditioning")
    dz = torch.empty((batch * G, wz), dtype=torch.float32, device=dout.device)
    dx = torch.empty((batch * G, wx), dtype=torch.float32, device=dout.device)
    with on_device_of(dz):
        _lib.check(_L().gw_gencast_precond_input_backward(batch, G, wz, wx, float(sigma_data), sigma.data_ptr(), dout.data_ptr(), _ld(dout),
                                                          dz.data_ptr(), wz, dx.data_ptr(), wx, _st(dz)),
                   "gw_gencast_precond_input_backward")
    return dz, dx


def precond_output_forward(z: torch.Tensor, preds: torch.Tensor, sigma: torch.Tensor, sigma_data: float = 1.0) -> torch.Tensor:
    """c_skip(sigma_b) z + c_out(sigma_b) preds on rows b G + g."""
    z, preds = _rows(z, "corrupted targets"), _rows(preds, "predictions")
    sigma, batch, G = _sigma_rows(sigma, int(z.shape[0]), "the output preconditioning")
    if z.shape != preds.shape:
        raise RuntimeError("graph_weather_amd: the output preconditioning expects predictions shaped like the targets %s, got %s"
                           % (tuple(z.shape), tuple(preds.shape)))
    width = int(z.shape[1])
    out = torch.empty((batch * G, width), dtype=torch.float32, device=z.device)
    with on_device_of(out):
        _lib.check(_L().gw_gencast_precond_output_forward(batch, G, width, float(sigma_data), sigma.data_ptr(), z.data_ptr(), _ld(z),
                                                          preds.data_ptr(), _ld(preds), out.data_ptr(), width, _st(out)),
                   "gw_gencast_precond_output_forward")
    return out


def precond_output_backward(dout: torch.Tensor, sigma: torch.Tensor, sigma_data: float = 1.0):
    """(dz, dpreds) of ``precond_output_forward``."""
    dout = _rows(dout, "dout")
    sigma, batch, G = _sigma_rows(sigma, int(dout.shape[0]), "the output preconditioning")
    width = int(dout.shape[1])
    dz, dp = (torch.empty((batch * G, width), dtype=torch.float32, device=dout.device) for _ in range(2))
    with on_device_of(dz):
        _lib.check(_L().gw_gencast_precond_output_backward(batch, G, width, float(sigma_data), sigma.data_ptr(), dout.data_ptr(), _ld(dout),
                                                           dz.data_ptr(), width, dp.data_ptr(), width, _st(dz)),
                   "gw_gencast_precond_output_backward")
    return dz, dp


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
_TN_CHUNK = 64 * 1024  # rows per call of the ordered weight-gradient product (its scratch grows with the rows: m n floats per 1024)


def gemm_tn_ordered(a: torch.Tensor, b: torch.Tensor, want_colsum: bool):
    """``aurora.gemm_tn_ordered`` (a^T @ b and the column sums of a, row slabs added in one fixed order) for any number of rows:
    edge-level products (5 M rows on GenCast's mesh) run in chunks of 65 536 rows whose results are added in chunk order."""
    rows = int(a.shape[0])
    if rows <= _TN_CHUNK:
        return _gemm_tn_ordered(a, b, want_colsum)
    c = colsum = None
    for r0 in range(0, rows, _TN_CHUNK):
        ci, si = _gemm_tn_ordered(a[r0:r0 + _TN_CHUNK], b[r0:r0 + _TN_CHUNK], want_colsum)
        c = ci if c is None else add_rows(c, ci)
        if want_colsum:
            colsum = si if colsum is None else add_rows(colsum[None], si[None])[0]
    return c, colsum


class _Linear(Function):
    """nn.Linear on the wide path's forward kernel with the ordered weight and bias gradients (``aurora._Linear``, any row count)."""

    @staticmethod
    def forward(ctx, x, w, b, relu: bool):
        out = linear_forward(x, w, b, relu)
        ctx.relu, ctx.has_b = relu, b is not None
        ctx.save_for_backward(x, w, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .wide import _relu_mask

        x, w, out = ctx.saved_tensors
        dz = _relu_mask(dout, out) if ctx.relu else _rows(dout, "dout")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear_forward(dz, w.detach().t().contiguous(), None, False)
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = gemm_tn_ordered(dz, x, ctx.has_b)
        return dx, dw, db, None


class _GraphAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, e, plan: GraphPlan, heads: int, mean: bool):
        need = any(ctx.needs_input_grad[:4])
        out, out_heads, lse = graph_attention_forward(q, k, v, e, plan, heads, mean, keep_heads=need)
        ctx.plan, ctx.heads, ctx.mean = plan, heads, mean
        ctx.save_for_backward(q, k, v, e, out_heads, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, e, out_heads, lse = ctx.saved_tensors
        dq, dk, dv, de = graph_attention_backward(q, k, v, e, ctx.plan, ctx.heads, ctx.mean, out_heads, lse, dout,
                                                  want_de=e is not None and ctx.needs_input_grad[3])
        return dq, dk, dv, de, None, None, None


class _CondLayerNorm(Function):
    @staticmethod
    def forward(ctx, x, scale, bias, act):
        ctx.act = act
        ctx.save_for_backward(x, scale, bias)
        return cond_layernorm_forward(x, scale, bias, act)

    @staticmethod
    def backward(ctx, dout):
        x, scale, bias = ctx.saved_tensors
        return cond_layernorm_backward(x, scale, bias, ctx.act, dout) + (None,)


class _BetaGate(Function):
    @staticmethod
    def forward(ctx, out, x_r, w):
        y, gate = beta_gate_forward(out, x_r, w)
        ctx.save_for_backward(out, x_r, w, gate)
        return y

    @staticmethod
    def backward(ctx, dy):
        return beta_gate_backward(*ctx.saved_tensors, dy)


class _Silu(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return silu_forward(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return silu_backward(x, dy)


class _Fourier(Function):
    @staticmethod
    def forward(ctx, t, num_frequencies: int, base_period: float):
        ctx.meta = (num_frequencies, base_period)
        ctx.save_for_backward(t)
        return fourier_forward(t, num_frequencies, base_period)

    @staticmethod
    def backward(ctx, dout):
        (t,) = ctx.saved_tensors
        return fourier_backward(t, dout, *ctx.meta), None, None


class _LinearGather(Function):
    """x @ w.T + b + sum_i table_i[idx_i] (``gw_linear_gather_forward``, no activation): the layer-1 split of an MLP whose input is
    a ``cat`` of gathered node rows and per-row features.  ``meta[i]`` = (idx or None, (perm, ptr)): how table i is read, and the
    CSR that groups the reading rows by table row - the table's gradient is that segment sum of dout, walked in one fixed order;
    the weight and bias gradients are ``gemm_tn_ordered``'s."""

    @staticmethod
    def forward(ctx, x, w, b, meta, *tables):
        rows = int(x.shape[0])
        out = linear_gather_forward(x, w, b, False, [(t, m[0], int(t.shape[0])) for t, m in zip(tables, meta)], rows, max(rows, 1))
        ctx.meta, ctx.has_b = meta, b is not None
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        dz = _rows(dout, "dout")
        rows = int(dz.shape[0])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear_forward(dz, w.detach().t().contiguous(), None, False)
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = gemm_tn_ordered(dz, x, ctx.has_b)
        dts = []
        for i, (idx, (perm, ptr)) in enumerate(ctx.meta):
            if not ctx.needs_input_grad[4 + i]:
                dts.append(None)
            elif idx is None:
                dts.append(dz)
            else:
                dts.append(segment_sum_rows(dz, rows, 1, 1, int(ptr.numel()) - 1, ptr, perm))
        return (dx, dw, db, None, *dts)


class _SegmentSum(Function):
    """out[i] = sum of the rows whose edge ends in i, rows in the caller's edge order, each run walked in sorted order."""

    @staticmethod
    def forward(ctx, rows, ep: EdgePlan):
        ctx.ep = ep
        return segment_sum_rows(rows, ep.num_edges, 1, 1, ep.n_dst, ep.plan.dst_ptr(), ep.perm32)

    @staticmethod
    def backward(ctx, dout):
        from .wide import gather_rows

        ep = ctx.ep
        return gather_rows(dout.contiguous(), ep.n_dst, ep.dst32, 1, ep.num_edges), None


class _GraphAttentionBatched(Function):
    @staticmethod
    def forward(ctx, q, k, v, e, plan: GraphPlan, heads: int, mean: bool, batch: int):
        need = any(ctx.needs_input_grad[:4])
        out, out_heads, lse = graph_attention_batched_forward(q, k, v, e, plan, heads, mean, batch, keep_heads=need)
        ctx.plan, ctx.heads, ctx.mean, ctx.batch = plan, heads, mean, batch
        ctx.save_for_backward(q, k, v, e, out_heads, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, e, out_heads, lse = ctx.saved_tensors
        dq, dk, dv, de = graph_attention_batched_backward(q, k, v, e, ctx.plan, ctx.heads, ctx.mean, ctx.batch, out_heads, lse, dout,
                                                          want_de=e is not None and ctx.needs_input_grad[3])
        return dq, dk, dv, de, None, None, None, None


class _CondLayerNormGrouped(Function):
    @staticmethod
    def forward(ctx, x, scale, bias, rows_per_group: int, act):
        ctx.act, ctx.rpg = act, rows_per_group
        ctx.save_for_backward(x, scale, bias)
        return cond_layernorm_grouped_forward(x, scale, bias, rows_per_group, act)

    @staticmethod
    def backward(ctx, dout):
        x, scale, bias = ctx.saved_tensors
        return cond_layernorm_grouped_backward(x, scale, bias, ctx.rpg, ctx.act, dout) + (None, None)


class _PrecondInput(Function):
    @staticmethod
    def forward(ctx, z, x, sigma, static, sigma_data: float):
        out, c_noise = precond_input_forward(z, x, sigma, static, sigma_data)
        ctx.meta = (int(z.shape[1]), int(x.shape[1]), sigma_data)
        ctx.save_for_backward(sigma)
        ctx.mark_non_differentiable(c_noise)
        return out, c_noise

    @staticmethod
    def backward(ctx, dout, _):
        (sigma,) = ctx.saved_tensors
        dz, dx = precond_input_backward(dout, sigma, *ctx.meta)
        return dz, dx, None, None, None


class _PrecondOutput(Function):
    @staticmethod
    def forward(ctx, z, preds, sigma, sigma_data: float):
        ctx.sigma_data = sigma_data
        ctx.save_for_backward(sigma)
        return precond_output_forward(z, preds, sigma, sigma_data)

    @staticmethod
    def backward(ctx, dout):
        (sigma,) = ctx.saved_tensors
        dz, dp = precond_output_backward(dout, sigma, ctx.sigma_data)
        return dz, dp, None, None


class _LinearGatherShared(Function):
    """``_LinearGather`` on ``batch`` copies of one graph: row m = (b, r) = divmod(m, rows_per_batch) of the output is
    x[m] @ w.T + b + sum_i table_i[b rows_pb_i + idx_i[r]] (x, w None: no product).  ``meta[i]`` = (idx or None, rows_pb, (perm,
    ptr)): rows_pb 0 is a table shared by the copies, whose gradient sums over the copies too (``gw_segment_sum_rows_wide`` with one
    output batch: one fixed order); (perm, ptr) the CSR that groups the rows r by table row (identity idx: perm None, ptr 0..n)."""

    @staticmethod
    def forward(ctx, x, w, b, meta, batch: int, rows_per_batch: int, *tables):
        rows = batch * rows_per_batch
        out = linear_gather_forward(x, w, b, False, [(t, m[0], m[1]) for t, m in zip(tables, meta)], rows, max(rows_per_batch, 1))
        ctx.meta, ctx.has_b, ctx.batch, ctx.rpb = meta, b is not None, batch, rows_per_batch
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        dz = _rows(dout, "dout")
        dx = dw = db = None
        if w is not None:
            if ctx.needs_input_grad[0]:
                dx = linear_forward(dz, w.detach().t().contiguous(), None, False)
            if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
                dw, db = gemm_tn_ordered(dz, x, ctx.has_b)
        dts = []
        for i, (idx, rows_pb, (perm, ptr)) in enumerate(ctx.meta):
            if not ctx.needs_input_grad[6 + i]:
                dts.append(None)
            elif idx is None and rows_pb:
                dts.append(dz)
            else:
                dts.append(segment_sum_rows(dz, ctx.rpb, ctx.batch, ctx.batch if rows_pb else 1, int(ptr.numel()) - 1, ptr, perm))
        return (dx, dw, db, None, None, None, *dts)


class _SegmentSumShared(Function):
    """``_SegmentSum`` per copy: rows [batch E, .] in the caller's edge order -> [batch n_dst, .]."""

    @staticmethod
    def forward(ctx, rows, ep: EdgePlan, batch: int):
        ctx.ep, ctx.batch = ep, batch
        return segment_sum_rows(rows, ep.num_edges, batch, batch, ep.n_dst, ep.plan.dst_ptr(), ep.perm32)

    @staticmethod
    def backward(ctx, dout):
        from .wide import gather_rows

        ep = ctx.ep
        return gather_rows(dout.contiguous(), ep.n_dst, ep.dst32, ctx.batch, ep.num_edges), None, None


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def _act_name(activation: Optional[nn.Module]) -> Optional[str]:
    if activation is None:
        return None
    if isinstance(activation, nn.ReLU):
        return "relu"
    if isinstance(activation, nn.SiLU):
        return "silu"
    raise NotImplementedError("graph_weather_amd: activation_layer must be nn.ReLU or nn.SiLU, got %s" % type(activation).__name__)


def _apply_act(name: Optional[str], x2: torch.Tensor) -> torch.Tensor:
    if name == "relu":
        return _Relu.apply(x2)
    if name == "silu":
        return _Silu.apply(x2)
    return x2


def _rows_in(x: torch.Tensor, name: str) -> torch.Tensor:
    _need_hip(x, name)
    if x.dim() != 2:
        raise RuntimeError(f"graph_weather_amd: {name} must be [rows, features]")
    return x


class MLP(nn.Module):
    """Classic multi-layer perceptron (modules.py)."""

    def __init__(self, input_dim: int, hidden_dims: list, activation_layer: nn.Module = nn.ReLU, use_layer_norm: bool = False,
                 bias: bool = True, activate_final: bool = False):
        super().__init__()
        self.linears = nn.ModuleList()
        self.linears.append(nn.Linear(input_dim, hidden_dims[0], bias=bias))
        for i in range(0, len(hidden_dims) - 1):
            self.linears.append(nn.Linear(hidden_dims[i], hidden_dims[i + 1], bias=bias))
        self.activation = activation_layer()
        _act_name(self.activation)
        self.norm_layer = None
        if use_layer_norm:
            self.norm_layer = nn.LayerNorm(hidden_dims[-1])
        self.activate_final = activate_final

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        l0 = self.linears[0]
        return self.tail(self._layer(0, _Linear.apply(_rows_in(x, "x"), l0.weight, l0.bias, False)))

    def _layer(self, i: int, y: torch.Tensor) -> torch.Tensor:
        """What follows Linear i: the activation (behind the last one only with ``activate_final``)."""
        if i < len(self.linears) - 1 or self.activate_final:
            return _apply_act(_act_name(self.activation), y)
        return y

    def tail(self, h: torch.Tensor) -> torch.Tensor:
        """Everything behind the first Linear and what follows it."""
        for i in range(1, len(self.linears)):
            lin = self.linears[i]
            h = self._layer(i, _Linear.apply(h, lin.weight, lin.bias, False))
        if self.norm_layer is not None:
            h = _ln(self.norm_layer, h)
        return h


class InteractionNetwork(nn.Module):
    """Single message-passing interaction network (modules.py): the message is ``scale_factor * mlp_edges(cat(x_i, x_j,
    edge_attr))`` with x_i the receiver's and x_j the sender's row, the messages are summed per receiver (a receiver without
    edges gets zeros) and the output is ``mlp_nodes(cat(x_recv, sum))``.  Neither ``cat`` is formed."""

    def __init__(self, sender_dim: int, receiver_dim: int, edge_attr_dim: int, hidden_dims: list, use_layer_norm: bool = False,
                 activation_layer: nn.Module = nn.ReLU, scale_factor: float = 1.0):
        super().__init__()
        self.mlp_edges = MLP(input_dim=sender_dim + receiver_dim + edge_attr_dim, hidden_dims=hidden_dims,
                             activation_layer=activation_layer, use_layer_norm=use_layer_norm, bias=True, activate_final=False)
        self.mlp_nodes = MLP(input_dim=receiver_dim + hidden_dims[-1], hidden_dims=hidden_dims, activation_layer=activation_layer,
                             use_layer_norm=use_layer_norm, bias=True, activate_final=False)
        self.scale_factor = scale_factor
        self._dims = (sender_dim, receiver_dim, edge_attr_dim)

    def forward(self, x: Tuple[torch.Tensor, torch.Tensor], edge_index: torch.Tensor, edge_attr: torch.Tensor) -> torch.Tensor:
        x_send, x_recv = _rows_in(x[0], "sender rows"), _rows_in(x[1], "receiver rows")
        edge_attr = _rows_in(edge_attr, "edge_attr")
        ds, dr, de = self._dims
        if int(x_send.shape[1]) != ds or int(x_recv.shape[1]) != dr or int(edge_attr.shape[1]) != de:
            raise RuntimeError("graph_weather_amd: the interaction network expects %d sender, %d receiver and %d edge features, got "
                               "%d, %d, %d" % (ds, dr, de, int(x_send.shape[1]), int(x_recv.shape[1]), int(edge_attr.shape[1])))
        ep = edge_plan(edge_index, int(x_send.shape[0]), int(x_recv.shape[0]))
        if int(edge_attr.shape[0]) != ep.num_edges:
            raise RuntimeError("graph_weather_amd: edge_attr must have one row per edge")
        # layer-1 split: cat(x_i, x_j, e) . W^T = (x_recv . Wi^T)[dst] + (x_send . Wj^T)[src] + e . We^T
        l0 = self.mlp_edges.linears[0]
        w0 = l0.weight
        p_recv = _Linear.apply(x_recv, w0[:, :dr], None, False)
        p_send = _Linear.apply(x_send, w0[:, dr:dr + ds], None, False)
        meta = ((ep.dst32, (ep.perm32, ep.plan.dst_ptr())), (ep.src32, ep.by_src))
        h = _LinearGather.apply(edge_attr, w0[:, dr + ds:], l0.bias, meta, p_recv, p_send)
        msg = self.mlp_edges.tail(self.mlp_edges._layer(0, h))
        aggr = _SegmentSum.apply(msg, ep)
        if self.scale_factor != 1.0:  # (the sum of the scaled messages, scaled once per receiver)
            aggr = _RowScale.apply(aggr, torch.full((ep.n_dst,), float(self.scale_factor), dtype=torch.float32, device=aggr.device))
        n0 = self.mlp_nodes.linears[0]
        p_node = _Linear.apply(x_recv, n0.weight[:, :dr], None, False)
        h = _LinearGather.apply(aggr, n0.weight[:, dr:], n0.bias, ((None, (None, ep.ident_dst)),), p_node)
        return self.mlp_nodes.tail(self.mlp_nodes._layer(0, h))

    def _forward_shared(self, x_send: torch.Tensor, x_recv: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor,
                        batch: int, n_send: int, n_recv: int) -> torch.Tensor:
        """``forward`` on ``batch`` copies of one graph -> [batch n_recv, .]: ``edge_index`` and ``edge_attr`` [E, .] describe one
        copy; a node table has ``batch n`` rows (copy b at b n) or ``n`` rows (shared by the copies).  The edge-level part of the
        first message layer, edge_attr . We^T + bias, is formed on E rows and gathered per copy: nothing of size batch E comes
        from the edge attributes alone."""
        ds, dr, _ = self._dims
        ep = edge_plan(edge_index, n_send, n_recv)
        E = ep.num_edges
        dev = edge_attr.device

        def rows_pb(t, n):  # 0: shared by the copies
            if int(t.shape[0]) not in (n, batch * n):
                raise RuntimeError("graph_weather_amd: a node table of a batch-shared graph has n or batch n rows")
            return n if int(t.shape[0]) == batch * n and batch > 1 else 0

        l0 = self.mlp_edges.linears[0]
        w0 = l0.weight
        p_recv = _Linear.apply(x_recv, w0[:, :dr], None, False)
        p_send = _Linear.apply(x_send, w0[:, dr:dr + ds], None, False)
        p_edge = _Linear.apply(edge_attr, w0[:, dr + ds:], l0.bias, False)  # [E, .]
        meta = ((None, 0, (None, ep.plan.identity_ptr())), (ep.dst32, rows_pb(x_recv, n_recv), (ep.perm32, ep.plan.dst_ptr())),
                (ep.src32, rows_pb(x_send, n_send), ep.by_src))
        h = _LinearGatherShared.apply(None, None, None, meta, batch, E, p_edge, p_recv, p_send)
        msg = self.mlp_edges.tail(self.mlp_edges._layer(0, h))
        aggr = _SegmentSumShared.apply(msg, ep, batch)
        if self.scale_factor != 1.0:
            aggr = _RowScale.apply(aggr, torch.full((batch * n_recv,), float(self.scale_factor), dtype=torch.float32, device=dev))
        n0 = self.mlp_nodes.linears[0]
        p_node = _Linear.apply(x_recv, n0.weight[:, :dr], None, False)
        h = _LinearGatherShared.apply(aggr, n0.weight[:, dr:], n0.bias, ((None, rows_pb(x_recv, n_recv), (None, ep.ident_dst)),), batch,
                                      n_recv, p_node)
        return self.mlp_nodes.tail(self.mlp_nodes._layer(0, h))


class FourierEmbedding(nn.Module):
    """Fourier embedding module (modules.py)."""

    def __init__(self, output_dim: int, num_frequencies: int, base_period: int):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(2 * num_frequencies, output_dim, bias=True), nn.SiLU(),
                                 nn.Linear(output_dim, output_dim, bias=True))
        self.num_frequencies = num_frequencies
        self.base_period = base_period

    def fourier_features(self, t):
        _need_hip(t, "t")
        return _Fourier.apply(t, int(self.num_frequencies), float(self.base_period))

    def forward(self, t):
        h = _Silu.apply(_Linear.apply(self.fourier_features(t), self.mlp[0].weight, self.mlp[0].bias, False))
        return _Linear.apply(h, self.mlp[2].weight, self.mlp[2].bias, False)


class ConditionalLayerNorm(nn.Module):
    """LayerNorm without affine whose scale and bias are Linears of a conditioning parameter (modules.py)."""

    def __init__(self, conditioning_dim: int, features_dim: int):
        super().__init__()
        self.linear_scale = nn.Linear(conditioning_dim, features_dim, bias=True)
        self.linear_bias = nn.Linear(conditioning_dim, features_dim, bias=True)
        self.norm = nn.LayerNorm(features_dim, eps=1e-05, elementwise_affine=False)

    def forward(self, x: torch.Tensor, cond_param: torch.Tensor, _act: Optional[str] = None) -> torch.Tensor:
        if not x.shape[0] == cond_param.shape[0]:
            raise ValueError(
                "Expected same batch dimension for the input and the conditioning "
                f"parameter, got {x.shape[0]} and {cond_param.shape[0]}"
            )
        x, cond_param = _rows_in(x, "x"), _rows_in(cond_param, "cond_param")
        scale = _Linear.apply(cond_param, self.linear_scale.weight, self.linear_scale.bias, False)
        bias = _Linear.apply(cond_param, self.linear_bias.weight, self.linear_bias.bias, False)
        return _CondLayerNorm.apply(x, scale, bias, _act)

    def _forward_grouped(self, x: torch.Tensor, cond_param: torch.Tensor, rows_per_group: int, _act: Optional[str] = None):
        """``forward`` with one conditioning row per ``rows_per_group`` consecutive rows of x: the two Linears run on the groups."""
        scale = _Linear.apply(cond_param, self.linear_scale.weight, self.linear_scale.bias, False)
        bias = _Linear.apply(cond_param, self.linear_bias.weight, self.linear_bias.bias, False)
        return _CondLayerNormGrouped.apply(x, scale, bias, rows_per_group, _act)


class TransformerConv(nn.Module):
    """Parameter holder and forward of PyG's ``TransformerConv(in, out, heads, concat, beta=True, edge_dim, bias=True,
    root_weight=True)`` without dropout, as restated in the module docstring of tests/gencast_oracle.py."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, beta: bool = False,
                 edge_dim: Optional[int] = None):
        super().__init__()
        if not beta:
            raise NotImplementedError("graph_weather_amd: TransformerConv is provided with beta=True (as GenCast builds it)")
        _check_attention(heads, out_channels)
        self.in_channels, self.out_channels, self.heads, self.concat, self.edge_dim = in_channels, out_channels, heads, concat, edge_dim
        hc = heads * out_channels
        self.lin_key = nn.Linear(in_channels, hc)
        self.lin_query = nn.Linear(in_channels, hc)
        self.lin_value = nn.Linear(in_channels, hc)
        if edge_dim is not None:
            self.lin_edge = nn.Linear(edge_dim, hc, bias=False)
        else:
            self.lin_edge = self.register_parameter("lin_edge", None)
        self.lin_skip = nn.Linear(in_channels, hc if concat else out_channels)
        self.lin_beta = nn.Linear(3 * (hc if concat else out_channels), 1, bias=False)

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _rows_in(x, "x")
        n = int(x.shape[0])
        ep = edge_plan(edge_index, n, n)
        q = _Linear.apply(x, self.lin_query.weight, self.lin_query.bias, False)
        k = _Linear.apply(x, self.lin_key.weight, self.lin_key.bias, False)
        v = _Linear.apply(x, self.lin_value.weight, self.lin_value.bias, False)
        e = None
        if self.lin_edge is not None:
            if edge_attr is None:
                raise RuntimeError("graph_weather_amd: this TransformerConv was built with edge_dim: edge_attr is required")
            e = _Linear.apply(_rows_in(edge_attr, "edge_attr"), self.lin_edge.weight, None, False)
        elif edge_attr is not None:
            raise RuntimeError("graph_weather_amd: edge_attr given to a TransformerConv built without edge_dim")
        out = _GraphAttention.apply(q, k, v, e, ep.plan, self.heads, not self.concat)
        x_r = _Linear.apply(x, self.lin_skip.weight, self.lin_skip.bias, False)
        return _BetaGate.apply(out, x_r, self.lin_beta.weight)

    def _forward_shared(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], batch: int) -> torch.Tensor:
        """``forward`` on x [batch n, .] over ``batch`` copies of one graph: ``edge_index`` and ``edge_attr`` [E, .] describe one
        copy, ``lin_edge`` runs on E rows and the attention reads that one table from every copy."""
        n = int(x.shape[0]) // batch
        ep = edge_plan(edge_index, n, n)
        q = _Linear.apply(x, self.lin_query.weight, self.lin_query.bias, False)
        k = _Linear.apply(x, self.lin_key.weight, self.lin_key.bias, False)
        v = _Linear.apply(x, self.lin_value.weight, self.lin_value.bias, False)
        e = None
        if self.lin_edge is not None:
            if edge_attr is None:
                raise RuntimeError("graph_weather_amd: this TransformerConv was built with edge_dim: edge_attr is required")
            e = _Linear.apply(_rows_in(edge_attr, "edge_attr"), self.lin_edge.weight, None, False)
        elif edge_attr is not None:
            raise RuntimeError("graph_weather_amd: edge_attr given to a TransformerConv built without edge_dim")
        out = _GraphAttentionBatched.apply(q, k, v, e, ep.plan, self.heads, not self.concat, batch)
        x_r = _Linear.apply(x, self.lin_skip.weight, self.lin_skip.bias, False)
        return _BetaGate.apply(out, x_r, self.lin_beta.weight)


class CondTransformerBlock(nn.Module):
    """A single conditioned transformer block for graphs (modules.py)."""

    def __init__(self, input_dim: int, output_dim: int, num_heads: int, conditioning_dim: Optional[int] = None,
                 edges_dim: Optional[int] = None, concat: bool = True, beta: bool = True,
                 activation_layer: Optional[nn.Module] = nn.ReLU):
        super().__init__()
        self.transformer_conv = TransformerConv(in_channels=input_dim, out_channels=output_dim, heads=num_heads, concat=concat,
                                                beta=beta, edge_dim=edges_dim)
        self.activation = activation_layer() if activation_layer is not None else None
        _act_name(self.activation)
        if conditioning_dim is not None:
            final_dim = num_heads * output_dim if concat else output_dim
            self.cond_norm = ConditionalLayerNorm(conditioning_dim=conditioning_dim, features_dim=final_dim)
        else:
            self.cond_norm = None

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None,
                cond_param: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = self.transformer_conv(x=x, edge_index=edge_index, edge_attr=edge_attr)
        act = _act_name(self.activation)
        if self.cond_norm is not None:
            return self.cond_norm(x, cond_param, _act=act)  # (the activation rides on the norm's kernel)
        return _apply_act(act, x)

    def _forward_shared(self, x, edge_index, edge_attr, cond_param, batch: int):
        """``forward`` on ``batch`` copies of one graph: x [batch n, .], ``cond_param`` one row per copy."""
        x = self.transformer_conv._forward_shared(x, edge_index, edge_attr, batch)
        act = _act_name(self.activation)
        if self.cond_norm is not None:
            return self.cond_norm._forward_grouped(x, cond_param, int(x.shape[0]) // batch, _act=act)
        return _apply_act(act, x)


class Encoder(nn.Module):
    """GenCast's encoder (encoder.py)."""

    def __init__(self, grid_dim: int, mesh_dim: int, edge_dim: int, hidden_dims: list, activation_layer: nn.Module = nn.ReLU,
                 use_layer_norm: bool = True, scale_factor: float = 1.0):
        super().__init__()
        self.latent_dim = hidden_dims[-1]
        kw = dict(hidden_dims=hidden_dims, activation_layer=activation_layer, use_layer_norm=use_layer_norm, bias=True,
                  activate_final=False)
        self.grid_mlp = MLP(input_dim=grid_dim, **kw)
        self.mesh_mlp = MLP(input_dim=mesh_dim, **kw)
        self.edges_mlp = MLP(input_dim=edge_dim, **kw)
        self.gnn = InteractionNetwork(sender_dim=self.latent_dim, receiver_dim=self.latent_dim, edge_attr_dim=self.latent_dim,
                                      hidden_dims=hidden_dims, use_layer_norm=use_layer_norm, activation_layer=activation_layer,
                                      scale_factor=scale_factor)
        self.grid_mlp_final = MLP(input_dim=self.latent_dim, **kw)

    def forward(self, input_grid_nodes: torch.Tensor, input_mesh_nodes: torch.Tensor, input_edge_attr: torch.Tensor,
                edge_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        grid_emb = self.grid_mlp(input_grid_nodes)
        mesh_emb = self.mesh_mlp(input_mesh_nodes)
        edges_emb = self.edges_mlp(input_edge_attr)
        latent_mesh_nodes = _Add.apply(mesh_emb, self.gnn(x=(grid_emb, mesh_emb), edge_index=edge_index, edge_attr=edges_emb))
        latent_grid_nodes = _Add.apply(grid_emb, self.grid_mlp_final(grid_emb))
        return latent_grid_nodes, latent_mesh_nodes

    def _forward_shared(self, input_grid_nodes: torch.Tensor, input_mesh_nodes: torch.Tensor, input_edge_attr: torch.Tensor,
                        edge_index: torch.Tensor, batch: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``forward`` on ``batch`` copies of one graph: grid rows [batch G, .]; the mesh node features [M, .], the edge attributes
        [E, .] and ``edge_index`` describe one copy, so ``mesh_mlp`` and ``edges_mlp`` run once -> ([batch G, .], [batch M, .])."""
        G, M = int(input_grid_nodes.shape[0]) // batch, int(input_mesh_nodes.shape[0])
        grid_emb = self.grid_mlp(input_grid_nodes)
        mesh_emb = self.mesh_mlp(input_mesh_nodes)
        edges_emb = self.edges_mlp(input_edge_attr)
        update = self.gnn._forward_shared(grid_emb, mesh_emb, edge_index, edges_emb, batch, G, M)
        ident = (None, edge_plan(edge_index, G, M).ident_dst)  # (the plan the interaction network just used)
        latent_mesh_nodes = _LinearGatherShared.apply(None, None, None, ((None, 0, ident), (None, M, ident)), batch, M, mesh_emb, update)
        latent_grid_nodes = _Add.apply(grid_emb, self.grid_mlp_final(grid_emb))
        return latent_grid_nodes, latent_mesh_nodes


class Decoder(nn.Module):
    """GenCast's decoder (decoder.py)."""

    def __init__(self, edges_dim: int, output_dim: int, hidden_dims: list, activation_layer: nn.Module = nn.ReLU,
                 use_layer_norm: bool = True):
        super().__init__()
        self.latent_dim = hidden_dims[-1]
        self.edges_mlp = MLP(input_dim=edges_dim, hidden_dims=hidden_dims, activation_layer=activation_layer,
                             use_layer_norm=use_layer_norm, bias=True, activate_final=False)
        self.gnn = InteractionNetwork(sender_dim=self.latent_dim, receiver_dim=self.latent_dim, edge_attr_dim=self.latent_dim,
                                      hidden_dims=hidden_dims, use_layer_norm=use_layer_norm, activation_layer=activation_layer)
        self.grid_mlp_final = MLP(input_dim=self.latent_dim, hidden_dims=hidden_dims[:-1] + [output_dim],
                                  activation_layer=activation_layer, use_layer_norm=use_layer_norm, bias=True, activate_final=False)

    def forward(self, input_mesh_nodes: torch.Tensor, input_grid_nodes: torch.Tensor, input_edge_attr: torch.Tensor,
                edge_index: torch.Tensor) -> torch.Tensor:
        if not (input_grid_nodes.shape[-1] == self.latent_dim and input_mesh_nodes.shape[-1] == self.latent_dim):
            raise ValueError(
                "The dimension of grid nodes and mesh nodes' features must be "
                "equal to the last hidden dimension."
            )
        edges_emb = self.edges_mlp(input_edge_attr)
        latent_grid_nodes = _Add.apply(_rows_in(input_grid_nodes, "input_grid_nodes"),
                                       self.gnn(x=(input_mesh_nodes, input_grid_nodes), edge_index=edge_index, edge_attr=edges_emb))
        return self.grid_mlp_final(latent_grid_nodes)

    def _forward_shared(self, input_mesh_nodes: torch.Tensor, input_grid_nodes: torch.Tensor, input_edge_attr: torch.Tensor,
                        edge_index: torch.Tensor, batch: int) -> torch.Tensor:
        """``forward`` on ``batch`` copies of one graph: node rows [batch M, .] and [batch G, .], one copy's edges."""
        M, G = int(input_mesh_nodes.shape[0]) // batch, int(input_grid_nodes.shape[0]) // batch
        edges_emb = self.edges_mlp(input_edge_attr)
        update = self.gnn._forward_shared(input_mesh_nodes, input_grid_nodes, edge_index, edges_emb, batch, M, G)
        return self.grid_mlp_final(_Add.apply(_rows_in(input_grid_nodes, "input_grid_nodes"), update))


def _sparse_mode(sparse) -> bool:
    """The ``sparse`` argument of the processors: False - the ``TransformerConv`` blocks; "native" - the sparse blocks on this
    package's kernels (True); anything else that is true asks for DGL, as the reference's ``sparse=True`` does."""
    if isinstance(sparse, str) and sparse == "native":
        return True
    if sparse:
        raise ValueError("Please install DGL to use sparsity. (sparse=\"native\" selects this package's own sparse processor.)")
    return False


def _sparse_blocks(blocks: nn.ModuleList, num_blocks: int, noise_emb_dim: int, latent_dim: int, num_heads: int, activation_layer) -> None:
    from .gencast_sparse import SparseTransformer  # (that module builds on this one)

    for _ in range(num_blocks):
        blocks.append(SparseTransformer(conditioning_dim=noise_emb_dim, input_dim=latent_dim, output_dim=latent_dim,
                                        num_heads=num_heads, activation_layer=activation_layer))


class Processor(nn.Module):
    """GenCast's processor (processor.py): transformer blocks over the mesh conditioned on the noise level.  ``sparse="native"``
    builds ``num_blocks`` ``gencast_sparse.SparseTransformer`` blocks (the reference's ``sparse=True`` processor on this package's
    kernels; edge features are then ignored, as in the reference); ``sparse=True`` itself asks for the reference's DGL backend,
    which is not installed here, and raises as the reference does without DGL."""

    def __init__(self, latent_dim: int, hidden_dims: list, num_blocks: int, num_heads: int, num_frequencies: int, base_period: int,
                 noise_emb_dim: int, edges_dim: Optional[int] = None, activation_layer: nn.Module = nn.ReLU,
                 use_layer_norm: bool = True, sparse=False):
        super().__init__()
        self.latent_dim = latent_dim
        if latent_dim % num_heads != 0:
            raise ValueError("The latent dimension should be divisible by the number of heads.")
        self.fourier_embedder = FourierEmbedding(output_dim=noise_emb_dim, num_frequencies=num_frequencies, base_period=base_period)
        self.edges_dim = edges_dim
        if edges_dim is not None:
            self.edges_mlp = MLP(input_dim=edges_dim, hidden_dims=hidden_dims, activation_layer=activation_layer,
                                 use_layer_norm=use_layer_norm, bias=True, activate_final=False)
        self.cond_transformers = nn.ModuleList()
        self.sparse = _sparse_mode(sparse)
        if self.sparse:
            _sparse_blocks(self.cond_transformers, num_blocks, noise_emb_dim, latent_dim, num_heads, activation_layer)
            return
        e_dim = hidden_dims[-1] if (edges_dim is not None) else None
        for _ in range(num_blocks - 1):  # concatenating multi-head attention
            self.cond_transformers.append(CondTransformerBlock(conditioning_dim=noise_emb_dim, input_dim=latent_dim,
                                                               output_dim=latent_dim // num_heads, edges_dim=e_dim,
                                                               num_heads=num_heads, concat=True, beta=True,
                                                               activation_layer=activation_layer))
        # averaging multi-head attention
        self.cond_transformers.append(CondTransformerBlock(conditioning_dim=noise_emb_dim, input_dim=latent_dim, output_dim=latent_dim,
                                                           edges_dim=e_dim, num_heads=num_heads, concat=False, beta=True,
                                                           activation_layer=None))

    def _check_args(self, latent_mesh_nodes, noise_levels, input_edge_attr):
        if not latent_mesh_nodes.shape[-1] == self.latent_dim:
            raise ValueError(
                "The dimension of the mesh nodes is different from the latent dimension provided at"
                " initialization."
            )
        if not latent_mesh_nodes.shape[0] == noise_levels.shape[0]:
            raise ValueError(
                "The number of noise levels and mesh nodes should be the same, but got "
                f"{latent_mesh_nodes.shape[0]} and {noise_levels.shape[0]}. Eventually repeat the "
                " noise level for each node in the same batch."
            )
        if (input_edge_attr is not None) and (self.edges_dim is None):
            raise ValueError("To use input_edge_attr initialize the processor with edges_dim.")

    def forward(self, latent_mesh_nodes: torch.Tensor, edge_index: torch.Tensor, noise_levels: torch.Tensor,
                input_edge_attr: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_args(latent_mesh_nodes, noise_levels, input_edge_attr)
        noise_emb = self.fourier_embedder(noise_levels)
        edges_emb = self.edges_mlp(input_edge_attr) if self.edges_dim is not None else None
        for cond_transformer in self.cond_transformers:
            latent_mesh_nodes = cond_transformer(x=latent_mesh_nodes, edge_index=edge_index, cond_param=noise_emb, edge_attr=edges_emb)
        return latent_mesh_nodes

    def _forward_shared(self, latent_mesh_nodes: torch.Tensor, edge_index: torch.Tensor, noise_levels: torch.Tensor,
                        input_edge_attr: Optional[torch.Tensor], batch: int) -> torch.Tensor:
        """``forward`` on ``batch`` copies of one graph: mesh rows [batch M, .], ``noise_levels`` [batch, 1] (one row per copy, not
        per node), one copy's ``edge_index`` and edge attributes.  The noise embedding and every block's scale and bias run on
        ``batch`` rows, ``edges_mlp`` and every ``lin_edge`` on E rows."""
        if (input_edge_attr is not None) and (self.edges_dim is None):
            raise ValueError("To use input_edge_attr initialize the processor with edges_dim.")
        noise_emb = self.fourier_embedder(noise_levels)
        edges_emb = self.edges_mlp(input_edge_attr) if self.edges_dim is not None else None
        for cond_transformer in self.cond_transformers:
            if self.sparse:
                latent_mesh_nodes = cond_transformer._forward_shared(latent_mesh_nodes, edge_index, noise_emb, batch)
            else:
                latent_mesh_nodes = cond_transformer._forward_shared(latent_mesh_nodes, edge_index, edges_emb, noise_emb, batch)
        return latent_mesh_nodes
