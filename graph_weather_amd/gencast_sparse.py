"""GenCast's experimental sparse processor block (``graph_weather/models/gencast/layers/experimental/sparse_transformer.py``):
``SparseAttention`` and ``SparseTransformer``, with the reference's constructor arguments, attribute names and ``state_dict`` keys.

The reference builds the block on ``dgl.sparse`` (``spmatrix``, ``bsddmm``, ``SparseMatrix.softmax``, ``bspmm``); here the masked
attention is ``csrc/gw_sparse_attn.hip``: one wave per attending row walks the row-sorted mask with an online softmax for all
heads at once, the backward recomputes the probabilities in one launch over rows (dq) and one over columns (dk, dv).  Arithmetic,
restated from the reference and DGL's documentation (not pinned against DGL): with ``D = output_dim``, ``nh`` heads and
``dh = D / nh``, ``q = (x Wq^T + bq) dh^-0.5``, ``k`` and ``v`` likewise without the scale; a row is viewed ``[dh, nh]`` - column
``c`` is ``(d = c // nh, h = c % nh)``, heads interleaved; entry ``e`` of ``edge_index`` attends from row ``edge_index[0, e]`` to
column ``edge_index[1, e]`` (the opposite direction of ``TransformerConv``), the softmax runs per head over the entries of a row,
every entry is its own term (duplicates count twice), a row without entries gets zeros.

Working layout: the kernels read head-major rows (head ``h`` is the contiguous segment ``[h dh, (h + 1) dh)``), so the three
projections are ONE Linear over a stacked ``[3 D, input_dim]`` weight whose rows are permuted to ``h dh + d``, ``out_proj`` runs on a
weight whose input columns are permuted the same way, and the kernel reads ``q``, ``k``, ``v`` in place as column blocks of the
stacked product.  The packs are cached per parameter version; the parameters, their gradients and every public tensor stay in
the reference's layout.  fp32 only; there is no CPU path.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .gencast import (MAX_ROW, ConditionalLayerNorm, _act_name, _apply_act, _Linear, _rows_in, gemm_tn_ordered)
from .graphs import GraphPlan
from .layers import KeyedCache, _ver, _version_key
from .ops import on_device_of
from .wide import _Add, _L, _ld, _rows, _st, linear_forward

__all__ = ["SparseAttention", "SparseTransformer", "SparsePlan", "sparse_plan", "sparse_attention_forward",
           "sparse_attention_backward", "head_major_index"]


# ---------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------
class SparsePlan:
    """The mask ``spmatrix(indices=edge_index, shape=(n, n))`` as the index structures the kernels walk: a ``GraphPlan`` whose
    "destination" is the attending row ``edge_index[0]`` and whose "source" is the attended column ``edge_index[1]`` - entries sorted
    by row (stable: a row's entries keep the caller's order), ``dst_ptr`` the row pointer, ``src_sorted`` the column-side walk."""

    def __init__(self, edge_index: torch.Tensor, n: int):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise RuntimeError("graph_weather_amd: edge_index must be an int64 [2, E] tensor in COO format")
        E = int(edge_index.shape[1])
        if max(E, n) >= 2 ** 31 - 1:
            raise RuntimeError("graph_weather_amd: graph too large for int32 plans")
        if E and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
            raise IndexError("edge_index refers to nodes outside the node table (n = %d)" % n)
        row, col = edge_index[0], edge_index[1]
        row_sorted, perm = torch.sort(row, stable=True)
        self.plan = GraphPlan(n, n, col[perm].to(torch.int32).contiguous(), row_sorted.to(torch.int32).contiguous(), perm.contiguous(),
                              None)
        self.plan.dst_ptr()
        self.plan.src_sorted()
        self.num_edges, self.n = E, n


_PLANS: list = []  # the last few (key, edge_index, SparsePlan); the entry holds the tensor, so its address cannot be recycled


def sparse_plan(edge_index: torch.Tensor, n: int) -> SparsePlan:
    """The ``SparsePlan`` of an ``edge_index`` tensor: built once per (address, shape, version, n)."""
    if not edge_index.is_cuda:
        raise RuntimeError("graph_weather_amd: edge_index must live on a HIP device (no CPU path exists)")
    key = (edge_index.data_ptr(), tuple(edge_index.shape), _ver(edge_index), int(n))
    for k, held, plan in _PLANS:
        if k == key and held is edge_index:
            return plan
    plan = SparsePlan(edge_index, int(n))
    _PLANS.append((key, edge_index, plan))
    del _PLANS[:-8]
    return plan


def head_major_index(num_heads: int, head_dim: int, device=None) -> torch.Tensor:
    """perm [D] int64: working (head-major) column ``h dh + d`` holds the reference's interleaved column ``perm = d nh + h``."""
    h = torch.arange(num_heads, device=device).repeat_interleave(head_dim)
    d = torch.arange(head_dim, device=device).repeat(num_heads)
    return d * num_heads + h


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _check_shapes(q, k, v, plan: GraphPlan, heads: int, batch: int) -> Tuple[int, int]:
    D = int(q.shape[1])
    if heads < 1 or batch < 1 or D % heads:
        raise RuntimeError("graph_weather_amd: sparse attention needs batch >= 1 and a width of q (%d) that is a multiple of the heads "
                           "(%d)" % (D, heads))
    if D > MAX_ROW:
        raise NotImplementedError("graph_weather_amd: the sparse attention kernels take heads * dim_head <= %d, got %d" % (MAX_ROW, D))
    nr, nc = plan.n_dst, plan.n_src
    if tuple(q.shape) != (batch * nr, D) or tuple(k.shape) != (batch * nc, D) or tuple(v.shape) != (batch * nc, D):
        raise RuntimeError("graph_weather_amd: sparse attention expects q [%d, %d] and k, v [%d, %d], got %s, %s, %s"
                           % (batch * nr, D, batch * nc, D, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    return D, D // heads


def sparse_attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, plan: GraphPlan, heads: int, scale: float,
                             batch: int = 1):
    """Masked attention on ``batch`` copies of the plan's mask (include/gw_amd.h: gw_sparse_attention_forward): q [batch n, H dh]
    (views with a row stride are read in place), k, v likewise, head-major rows -> (out [batch n, H dh], lse [2, batch n H])."""
    q, k, v = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
    D, dh = _check_shapes(q, k, v, plan, heads, batch)
    E, nr, nc = plan.num_edges, plan.n_dst, plan.n_src
    # (0 entries: the library launches nothing; every output row is then the zero this fill leaves)
    new = torch.zeros if E == 0 else torch.empty
    out = new((batch * nr, D), dtype=torch.float32, device=q.device)
    lse = new((2, batch * nr * heads), dtype=torch.float32, device=q.device)
    with on_device_of(out):
        _lib.check(_L().gw_sparse_attention_forward(batch, nr, nc, E, heads, dh, float(scale), plan.dst_ptr().data_ptr(),
                                                    plan.src.data_ptr(), q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(),
                                                    _ld(v), out.data_ptr(), D, lse.data_ptr(), _st(out)),
                   "gw_sparse_attention_forward")
    return out, lse


def sparse_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, plan: GraphPlan, heads: int, scale: float,
                              batch: int, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, stacked: bool = False):
    """(dq, dk, dv) of ``sparse_attention_forward``; dq is the gradient of the unscaled q.  ``stacked``: the three are the column
    blocks of one [batch n, 3 H dh] tensor (the layout of a stacked projection), which is returned as a fourth value."""
    q, k, v, out, dout = _rows(q, "q"), _rows(k, "k"), _rows(v, "v"), _rows(out, "out"), _rows(dout, "dout")
    D, dh = _check_shapes(q, k, v, plan, heads, batch)
    E, nr, nc = plan.num_edges, plan.n_dst, plan.n_src
    if out.shape != q.shape or dout.shape != q.shape:
        raise RuntimeError("graph_weather_amd: sparse attention backward expects out and dout shaped like q %s, got %s and %s"
                           % (tuple(q.shape), tuple(out.shape), tuple(dout.shape)))
    new = torch.zeros if E == 0 else torch.empty
    if stacked:
        if nr != nc:
            raise RuntimeError("graph_weather_amd: stacked gradients need a square mask")
        dqkv = new((batch * nr, 3 * D), dtype=torch.float32, device=q.device)
        dq, dk, dv = dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
    else:
        dqkv = None
        dq = new((batch * nr, D), dtype=torch.float32, device=q.device)
        dk, dv = (new((batch * nc, D), dtype=torch.float32, device=q.device) for _ in range(2))
    delta = torch.empty((max(batch * nr * heads, 1),), dtype=torch.float32, device=q.device)
    col_pos, col_ptr = plan.src_sorted()
    with on_device_of(dq):
        _lib.check(_L().gw_sparse_attention_backward(batch, nr, nc, E, heads, dh, float(scale), plan.dst_ptr().data_ptr(),
                                                     plan.src.data_ptr(), plan.dst.data_ptr(), col_pos.data_ptr(), col_ptr.data_ptr(),
                                                     q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(),
                                                     _ld(out), dout.data_ptr(), _ld(dout), lse.data_ptr(), delta.data_ptr(),
                                                     dq.data_ptr(), _ld(dq), dk.data_ptr(), _ld(dk), dv.data_ptr(), _ld(dv), _st(dq)),
                   "gw_sparse_attention_backward")
    return (dq, dk, dv, dqkv) if stacked else (dq, dk, dv)


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
class _SparseAttentionStacked(Function):
    """The masked attention on q, k, v read in place as the column blocks of one stacked projection [batch n, 3 D]; the gradient is
    one stacked tensor too, each block written by the kernels through its leading dimension."""

    @staticmethod
    def forward(ctx, qkv, plan: GraphPlan, heads: int, scale: float, batch: int):
        D = int(qkv.shape[1]) // 3
        out, lse = sparse_attention_forward(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], plan, heads, scale, batch)
        ctx.meta = (plan, heads, scale, batch, D)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        plan, heads, scale, batch, D = ctx.meta
        dqkv = sparse_attention_backward(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], plan, heads, scale, batch, out, lse, dout,
                                         stacked=True)[3]
        return dqkv, None, None, None, None


class _PackedLinear(Function):
    """x @ wp.T + bp on a packed copy (wp, bp) of the parameters ``params``; ``unpack(dwp, dbp)`` maps the packed gradients (the
    ordered, atomic-free ones of ``gencast._Linear``) back to one gradient per parameter, in the parameters' own layout."""

    @staticmethod
    def forward(ctx, x, wp, bp, unpack, *params):
        ctx.unpack = unpack
        ctx.save_for_backward(x, wp)
        return linear_forward(x, wp, bp, False)

    @staticmethod
    def backward(ctx, dout):
        x, wp = ctx.saved_tensors
        dz = _rows(dout, "dout")
        dx = linear_forward(dz, wp.t().contiguous(), None, False) if ctx.needs_input_grad[0] else None
        grads = (None,) * (len(ctx.needs_input_grad) - 4)
        if any(ctx.needs_input_grad[4:]):
            dwp, dbp = gemm_tn_ordered(dz, x, True)
            grads = ctx.unpack(dwp, dbp)
        return (dx, None, None, None, *grads)


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
class SparseAttention(nn.Module):
    """Sparse Multi-head Attention Module (sparse_transformer.py).  ``adj`` is the mask as an int64 ``edge_index`` [2, E]: entry e
    lets row ``edge_index[0, e]`` attend to column ``edge_index[1, e]`` (``dglsp.spmatrix(indices=edge_index, shape=(N, N))``)."""

    def __init__(self, input_dim=512, output_dim=512, num_heads=4):
        super().__init__()
        if output_dim % num_heads:
            raise ValueError("Output dimension should be divisible by the number of heads.")
        if output_dim > MAX_ROW:
            raise NotImplementedError("graph_weather_amd: the sparse attention kernels take output_dim <= %d, got %d"
                                      % (MAX_ROW, output_dim))
        self.hidden_size = output_dim
        self.num_heads = num_heads
        self.head_dim = output_dim // num_heads
        self.scaling = self.head_dim**-0.5

        self.q_proj = nn.Linear(input_dim, output_dim)
        self.k_proj = nn.Linear(input_dim, output_dim)
        self.v_proj = nn.Linear(input_dim, output_dim)
        self.out_proj = nn.Linear(output_dim, output_dim)

    # ---- packs: head-major copies of the parameters, one per parameter version -------------------------------------------------
    def _packs(self):
        """(w_qkv [3 D, in], b_qkv [3 D], w_out [D, D], inv): rows of the three projections and input columns of ``out_proj``
        permuted to head-major order; ``inv`` maps a reference column to its working column (for the gradients' way back)."""
        params = [self.q_proj.weight, self.q_proj.bias, self.k_proj.weight, self.k_proj.bias, self.v_proj.weight, self.v_proj.bias,
                  self.out_proj.weight]
        cache = self.__dict__.get("_pack_cache")
        if cache is None:
            cache = self.__dict__["_pack_cache"] = KeyedCache()

        def make():
            with torch.no_grad():
                perm = head_major_index(self.num_heads, self.head_dim, device=self.q_proj.weight.device)
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(perm.numel(), device=perm.device)
                w = torch.cat([p.weight.detach().index_select(0, perm) for p in (self.q_proj, self.k_proj, self.v_proj)]).contiguous()
                b = torch.cat([p.bias.detach().index_select(0, perm) for p in (self.q_proj, self.k_proj, self.v_proj)]).contiguous()
                wo = self.out_proj.weight.detach().index_select(1, perm).contiguous()
            return w, b, wo, inv

        return cache.get("packs", _version_key(params), make)

    def _run(self, x: torch.Tensor, edge_index: torch.Tensor, batch: int) -> torch.Tensor:
        x = _rows_in(x, "x")
        if int(x.shape[0]) % batch:
            raise RuntimeError("graph_weather_amd: %d rows do not split into %d copies" % (int(x.shape[0]), batch))
        sp = sparse_plan(edge_index, int(x.shape[0]) // batch)
        w, b, wo, inv = self._packs()
        D = self.hidden_size

        def unpack_qkv(dwp, dbp):
            return tuple(g for i in range(3) for g in (dwp[i * D:(i + 1) * D].index_select(0, inv), dbp[i * D:(i + 1) * D].index_select(0, inv)))

        def unpack_out(dwp, dbp):
            return dwp.index_select(1, inv), dbp

        qkv = _PackedLinear.apply(x, w, b, unpack_qkv, self.q_proj.weight, self.q_proj.bias, self.k_proj.weight, self.k_proj.bias,
                                  self.v_proj.weight, self.v_proj.bias)
        out = _SparseAttentionStacked.apply(qkv, sp.plan, self.num_heads, float(self.scaling), batch)
        return _PackedLinear.apply(out, wo, self.out_proj.bias, unpack_out, self.out_proj.weight, self.out_proj.bias)

    def forward(self, x: torch.Tensor, adj: torch.Tensor) -> torch.Tensor:
        return self._run(x, adj, 1)

    def _forward_shared(self, x: torch.Tensor, edge_index: torch.Tensor, batch: int) -> torch.Tensor:
        """``forward`` on x [batch n, .] over ``batch`` copies of one mask."""
        return self._run(x, edge_index, batch)


class SparseTransformer(nn.Module):
    """A single transformer block for graph neural networks (sparse_transformer.py): pre-norm (``norm_first``) or post-norm
    attention and MLP sublayers with conditional layer normalisation, the attention masked to ``edge_index``.

    Deviation: the reference accepts ``input_dim != output_dim`` at construction and then fails in the residual of the first
    forward; here the constructor raises ``ValueError``."""

    def __init__(self, conditioning_dim: int, input_dim: int, output_dim: int, num_heads: int,
                 activation_layer: torch.nn.Module = nn.ReLU, norm_first: bool = True):
        super().__init__()
        if input_dim != output_dim:
            raise ValueError("graph_weather_amd: SparseTransformer adds its input to the attention's output: input_dim (%d) and "
                             "output_dim (%d) must be equal" % (input_dim, output_dim))
        self.sparse_attention = SparseAttention(input_dim=input_dim, output_dim=output_dim, num_heads=num_heads)
        self.activation = activation_layer()
        _act_name(self.activation)
        self.mlp = nn.Sequential(nn.Linear(output_dim, output_dim), self.activation, nn.Linear(output_dim, output_dim))
        self.cond_norm_1 = ConditionalLayerNorm(conditioning_dim=conditioning_dim, features_dim=output_dim)
        self.cond_norm_2 = ConditionalLayerNorm(conditioning_dim=conditioning_dim, features_dim=output_dim)
        self.norm_first = norm_first

    def _mlp(self, x: torch.Tensor) -> torch.Tensor:
        h = _apply_act(_act_name(self.activation), _Linear.apply(x, self.mlp[0].weight, self.mlp[0].bias, False))
        return _Linear.apply(h, self.mlp[2].weight, self.mlp[2].bias, False)

    def _block(self, x, edge_index, norm_1, norm_2, batch: int):
        attn = self.sparse_attention
        if self.norm_first:
            x = _Add.apply(x, attn._run(norm_1(x), edge_index, batch))
            return _Add.apply(x, self._mlp(norm_2(x)))
        x = norm_1(_Add.apply(x, attn._run(x, edge_index, batch)))
        return norm_2(_Add.apply(x, self._mlp(x)))

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, cond_param: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        """x [N, D], ``cond_param`` one row per node; further arguments (the processors pass ``edge_attr``) are ignored."""
        x = _rows_in(x, "x")
        return self._block(x, edge_index, lambda t: self.cond_norm_1(t, cond_param), lambda t: self.cond_norm_2(t, cond_param), 1)

    def _forward_shared(self, x: torch.Tensor, edge_index: torch.Tensor, cond_param: torch.Tensor, batch: int) -> torch.Tensor:
        """``forward`` on ``batch`` copies of one graph: x [batch n, D], ``cond_param`` one row per copy, one copy's
        ``edge_index``."""
        x = _rows_in(x, "x")
        cond_param = _rows_in(cond_param, "cond_param")
        n = int(x.shape[0]) // batch
        if int(cond_param.shape[0]) != batch or n * batch != int(x.shape[0]):
            raise RuntimeError("graph_weather_amd: the batch-shared block takes %d conditioning rows and rows that split evenly "
                               "among them, got %d and %d" % (batch, int(cond_param.shape[0]), int(x.shape[0])))
        return self._block(x, edge_index, lambda t: self.cond_norm_1._forward_grouped(t, cond_param, n),
                           lambda t: self.cond_norm_2._forward_grouped(t, cond_param, n), batch)
