"""The Functional Generative Network of the reference (``graph_weather/models/fgn``): ``Processor`` (fgn/layers/processor.py),
``FunctionalGenerativeNetwork`` and ``FunctionalGenerativeNetworkConfig`` (fgn/model.py).

FGN stands on GenCast's ``GraphBuilder``, ``Encoder`` and ``Decoder`` unchanged; its processor is GenCast's without the Fourier
embedder - the blocks are conditioned on a random noise vector, so one forward gives an ensemble.  Same constructor arguments,
defaults, attribute names, ``state_dict`` keys and order, the 14 non-persistent graph buffers and the reference's error messages.

The reference's ``forward(previous_weather_state, num_ensemble=N)`` runs encoder -> processor -> decoder N times in a Python loop
over the same input.  ``FunctionalGenerativeNetwork.forward`` here runs B samples x N members = B N copies of ONE graph, copy
c = b N + n, and computes what the members of a sample share once:

* the encoder runs on the B samples (``Encoder._forward_shared``); the static grid features join the input in one concatenation
  of size B G (an expanded view of the [G, .] table - the features are not repeated first);
* the first block's ``TransformerConv`` runs at batch B; its ``ConditionalLayerNorm`` is where the members first differ, and
  ``gw_cond_layernorm_fanout_forward`` turns every row [B M, W] into its N conditioned rows [B N M, W] with the row statistics
  formed once;
* the later blocks run at batch B N on the batched attention and the grouped norm;
* the decoder's receiver-side tables (``p_recv``, ``p_node`` and the residual) are built on the B G grid rows and read by copy c
  at block c / N (``gw_linear_gather_grouped_forward``); their gradients sum the N copies of a block in copy order
  (``gw_segment_sum_rows_grouped``), so the encoder receives the gradient summed over the members once.

``_forward_member_loop`` is the reference's route on this package's kernels (one member at a time at batch B), for comparison
and measurement.

One deliberate deviation: the reference returns ``torch.stack(predictions, 1) if len(prediction) > 1 else
predictions[0].unsqueeze(1)`` and ``len(prediction)`` is the batch size, so at B = 1 it drops every member but the first.  Here
all members are returned at every B, as the reference's docstring promises.  Not reproduced: the reference's per-stage
``assert not torch.isnan(...)`` host reads.  fp32 only, no dropout; there is no CPU path.

``sparse="native"`` (with ``use_edges_features=False``) runs the processor on ``gencast_sparse.SparseTransformer`` blocks.  Their
first norm already sees the noise, so the mesh rows fan out to the B N copies before block 0 and every block runs at batch B N;
``sparse=True`` asks for the reference's DGL backend and raises as the reference does without DGL.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .aurora import _RowScale, _workspace
from .gencast import (_ACT_CODE, MLP, CondTransformerBlock, Decoder, Encoder, _act_name, _Linear, _rows_in, _SegmentSumShared,
                      _sparse_blocks, _sparse_mode, edge_plan, gemm_tn_ordered)
from .gencast_graphs import GraphBuilder
from .gencast_model import Denoiser
from .ops import on_device_of
from .wide import _L, _ld, _rows, _st, linear_forward

try:  # the hub mixin gives save_pretrained / from_pretrained / push_to_hub
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover
    class PyTorchModelHubMixin:  # type: ignore
        pass

__all__ = ["Processor", "FunctionalGenerativeNetwork", "FunctionalGenerativeNetworkConfig", "cond_layernorm_fanout_forward",
           "cond_layernorm_fanout_backward", "linear_gather_grouped_forward", "segment_sum_rows_grouped"]


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _fanout_shapes(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_sample: int, members: int) -> int:
    rows, width = int(x.shape[0]), int(x.shape[1])
    if rows_per_sample < 1 or members < 1 or rows % rows_per_sample:
        raise RuntimeError("graph_weather_amd: the fan-out norm needs members >= 1 and x rows (%d) that split into samples of %d"
                           % (rows, rows_per_sample))
    groups = rows // rows_per_sample * members
    if tuple(scale.shape) != (groups, width) or tuple(bias.shape) != (groups, width):
        raise RuntimeError("graph_weather_amd: %d samples x %d members need scale and bias [%d, %d], got %s and %s"
                           % (rows // rows_per_sample, members, groups, width, tuple(scale.shape), tuple(bias.shape)))
    return groups


def cond_layernorm_fanout_forward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_sample: int, members: int,
                                  act: Optional[str] = None) -> torch.Tensor:
    """x [B M, W], scale and bias [B N, W] -> [B N M, W]: row (b, n, m) = act(scale[b N + n] * LayerNorm(x[b M + m]) + bias[b N + n])
    (include/gw_amd.h: gw_cond_layernorm_fanout_forward)."""
    x, scale, bias = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias")
    groups = _fanout_shapes(x, scale, bias, rows_per_sample, members)
    rows, width = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((groups * rows_per_sample, width), dtype=torch.float32, device=x.device)
    with on_device_of(out):
        _lib.check(_L().gw_cond_layernorm_fanout_forward(rows, width, _ACT_CODE[act], rows_per_sample, members, x.data_ptr(), _ld(x),
                                                         scale.data_ptr(), _ld(scale), bias.data_ptr(), _ld(bias), out.data_ptr(), width,
                                                         _st(out)), "gw_cond_layernorm_fanout_forward")
    return out


def cond_layernorm_fanout_backward(x: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, rows_per_sample: int, members: int,
                                   act: Optional[str], dout: torch.Tensor):
    """(dx [B M, W], dscale [B N, W], dbias [B N, W]) of ``cond_layernorm_fanout_forward``."""
    x, scale, bias, dout = _rows(x, "x"), _rows(scale, "scale"), _rows(bias, "bias"), _rows(dout, "dout")
    groups = _fanout_shapes(x, scale, bias, rows_per_sample, members)
    rows, width = int(x.shape[0]), int(x.shape[1])
    if tuple(dout.shape) != (groups * rows_per_sample, width):
        raise RuntimeError("graph_weather_amd: the fan-out norm's dout must be [%d, %d], got %s"
                           % (groups * rows_per_sample, width, tuple(dout.shape)))
    dx = torch.empty((rows, width), dtype=torch.float32, device=x.device)
    dscale, dbias = (torch.zeros((groups, width), dtype=torch.float32, device=x.device) for _ in range(2))
    if rows:
        nbytes = int(_L().gw_cond_layernorm_fanout_workspace_bytes(rows, width, rows_per_sample, members))
        ws = _workspace(nbytes, "gw_cond_layernorm_fanout_workspace_bytes", x.device)
        with on_device_of(dx):
            _lib.check(_L().gw_cond_layernorm_fanout_backward(rows, width, _ACT_CODE[act], rows_per_sample, members, x.data_ptr(), _ld(x),
                                                              scale.data_ptr(), _ld(scale), bias.data_ptr(), _ld(bias), dout.data_ptr(),
                                                              _ld(dout), ws.data_ptr(), nbytes, dx.data_ptr(), width, dscale.data_ptr(),
                                                              dbias.data_ptr(), width, _st(dx)), "gw_cond_layernorm_fanout_backward")
    return dx, dscale, dbias


def linear_gather_grouped_forward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], bias: Optional[torch.Tensor], relu: bool,
                                  adds: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int, int]], rows: int,
                                  rows_per_batch: int) -> torch.Tensor:
    """``wide.linear_gather_forward`` with a share count per table: ``adds`` = [(table, idx or None, rows_pb, share)] and copy
    b = m // rows_per_batch reads block b // share of the table."""
    n = int(adds[0][0].shape[1]) if w is None else int(w.shape[0])
    k = 0
    if w is not None:
        x, w = _rows(x, "x"), _rows(w, "weight")
        k = int(x.shape[1])
        if int(w.shape[1]) != k or int(x.shape[0]) != rows:
            raise RuntimeError("graph_weather_amd: Linear operand shapes do not match")
    na = len(adds)
    tabs = [_rows(a[0], "addend") for a in adds]
    copies = -(-rows // max(1, rows_per_batch))
    for t, (_, idx, rows_pb, share) in zip(tabs, adds):  # every block a copy can reach lies inside its table
        if share < 1 or rows_pb < 0 or int(t.shape[1]) != n:
            raise RuntimeError("graph_weather_amd: a grouped addend needs share >= 1, rows_pb >= 0 and the output's width")
        if idx is None and rows and int(t.shape[0]) < ((copies - 1) // share) * rows_pb + min(rows, rows_per_batch):
            raise RuntimeError("graph_weather_amd: a grouped addend table has too few rows for its copies")
    dev = tabs[0].device if na else x.device
    out = torch.empty((rows, n), dtype=torch.float32, device=dev)
    tp = (ctypes.c_void_p * max(na, 1))(*[t.data_ptr() for t in tabs])
    ip = (ctypes.c_void_p * max(na, 1))(*[None if a[1] is None else a[1].data_ptr() for a in adds])
    lp = (ctypes.c_int32 * max(na, 1))(*[_ld(t) for t in tabs])
    rp = (ctypes.c_int32 * max(na, 1))(*[int(a[2]) for a in adds])
    sp = (ctypes.c_int32 * max(na, 1))(*([int(a[3]) for a in adds] or [1]))
    with on_device_of(out):
        _lib.check(_L().gw_linear_gather_grouped_forward(rows, max(1, rows_per_batch), k, n, None if w is None else x.data_ptr(),
                                                         0 if w is None else _ld(x), None if w is None else w.data_ptr(),
                                                         0 if w is None else _ld(w), None if bias is None else bias.contiguous().data_ptr(),
                                                         na, tp, ip, lp, rp, sp, 1 if relu else 0, out.data_ptr(), n, _st(out)),
                   "gw_linear_gather_grouped_forward")
    return out


def segment_sum_rows_grouped(rows: torch.Tensor, rows_pb_in: int, batch: int, share: int, n_seg: int, ptr: torch.Tensor,
                             perm: Optional[torch.Tensor]) -> torch.Tensor:
    """rows [batch rows_pb_in, W] -> [batch / share, n_seg, W]: block g is the sum over copies g share .. g share + share - 1, in
    copy order, of the rows perm[ptr[s] : ptr[s + 1]] of the copy (perm None: the rows themselves)."""
    rows = _rows(rows, "rows")
    width = int(rows.shape[1])
    if share < 1 or batch % share or int(rows.shape[0]) < batch * rows_pb_in or int(ptr.numel()) != n_seg + 1:
        raise RuntimeError("graph_weather_amd: the grouped segment sum needs a batch (%d) that is a multiple of the share (%d), "
                           "batch x %d rows and n_seg + 1 pointers" % (batch, share, rows_pb_in))
    out = torch.empty((batch // share * n_seg, width), dtype=torch.float32, device=rows.device)
    with on_device_of(out):
        _lib.check(_L().gw_segment_sum_rows_grouped(batch, share, n_seg, width, rows.data_ptr(), _ld(rows), rows_pb_in,
                                                    None if perm is None else perm.data_ptr(), ptr.data_ptr(), out.data_ptr(), width,
                                                    _st(out)), "gw_segment_sum_rows_grouped")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
class _CondLayerNormFanout(Function):
    @staticmethod
    def forward(ctx, x, scale, bias, rows_per_sample: int, members: int, act):
        ctx.meta = (rows_per_sample, members, act)
        ctx.save_for_backward(x, scale, bias)
        return cond_layernorm_fanout_forward(x, scale, bias, rows_per_sample, members, act)

    @staticmethod
    def backward(ctx, dout):
        x, scale, bias = ctx.saved_tensors
        rps, members, act = ctx.meta
        return cond_layernorm_fanout_backward(x, scale, bias, rps, members, act, dout) + (None, None, None)


class _LinearGatherGrouped(Function):
    """``gencast._LinearGatherShared`` with a share count per table: row m = (c, r) = divmod(m, rows_per_batch) of the output is
    x[m] @ w.T + b + sum_i table_i[(c // share_i) rows_pb_i + idx_i[r]] (x, w None: no product).  ``meta[i]`` = (idx or None,
    rows_pb, share, (perm, ptr)); the gradient of table i sums the ``share_i`` copies of a block in copy order (all ``batch``
    copies with rows_pb 0), each walked in the CSR (perm, ptr) that groups the rows r by table row."""

    @staticmethod
    def forward(ctx, x, w, b, meta, batch: int, rows_per_batch: int, *tables):
        rows = batch * rows_per_batch
        out = linear_gather_grouped_forward(x, w, b, False, [(t, m[0], m[1], m[2]) for t, m in zip(tables, meta)], rows,
                                            max(rows_per_batch, 1))
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
        for i, (idx, rows_pb, share, (perm, ptr)) in enumerate(ctx.meta):
            if not ctx.needs_input_grad[6 + i]:
                dts.append(None)
            elif idx is None and rows_pb and share == 1:
                dts.append(dz)
            else:
                dts.append(segment_sum_rows_grouped(dz, ctx.rpb, ctx.batch, share if rows_pb else ctx.batch, int(ptr.numel()) - 1, ptr,
                                                    perm))
        return (dx, dw, db, None, None, None, *dts)


# ---------------------------------------------------------------------------------------------------------------------
# fgn/layers/processor.py
# ---------------------------------------------------------------------------------------------------------------------
class Processor(nn.Module):
    """FGN's processor (fgn/layers/processor.py): GenCast's transformer blocks over the mesh, conditioned on a noise vector
    instead of an embedded noise level (there is no ``fourier_embedder``).  ``sparse="native"`` builds ``num_blocks``
    ``gencast_sparse.SparseTransformer`` blocks, as ``gencast.Processor`` does; ``sparse=True`` (the reference's DGL backend) raises
    as the reference does without DGL."""

    def __init__(self, latent_dim: int, hidden_dims: list, num_blocks: int, num_heads: int, noise_emb_dim: int,
                 edges_dim: Optional[int] = None, activation_layer: nn.Module = nn.ReLU, use_layer_norm: bool = True,
                 sparse=False):
        super().__init__()
        self.latent_dim = latent_dim
        if latent_dim % num_heads != 0:
            raise ValueError("The latent dimension should be divisible by the number of heads.")
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

    def forward(self, latent_mesh_nodes: torch.Tensor, edge_index: torch.Tensor, noise_vector: torch.Tensor,
                input_edge_attr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One noise row per node, as in the reference; runs on the per-row kernels."""
        self._check_args(latent_mesh_nodes, noise_vector, input_edge_attr)
        edges_emb = self.edges_mlp(input_edge_attr) if self.edges_dim is not None else None
        for cond_transformer in self.cond_transformers:
            latent_mesh_nodes = cond_transformer(x=latent_mesh_nodes, edge_index=edge_index, cond_param=noise_vector,
                                                 edge_attr=edges_emb)
        return latent_mesh_nodes

    def _edges(self, input_edge_attr):
        if (input_edge_attr is not None) and (self.edges_dim is None):
            raise ValueError("To use input_edge_attr initialize the processor with edges_dim.")
        return self.edges_mlp(input_edge_attr) if self.edges_dim is not None else None

    def _forward_shared(self, latent_mesh_nodes: torch.Tensor, edge_index: torch.Tensor, noise_vector: torch.Tensor,
                        input_edge_attr: Optional[torch.Tensor], batch: int) -> torch.Tensor:
        """``forward`` on ``batch`` copies of one graph: mesh rows [batch M, .], ``noise_vector`` [batch, .] (one row per copy, not
        per node), one copy's ``edge_index`` and edge attributes."""
        edges_emb = self._edges(input_edge_attr)
        for cond_transformer in self.cond_transformers:
            if self.sparse:
                latent_mesh_nodes = cond_transformer._forward_shared(latent_mesh_nodes, edge_index, noise_vector, batch)
            else:
                latent_mesh_nodes = cond_transformer._forward_shared(latent_mesh_nodes, edge_index, edges_emb, noise_vector, batch)
        return latent_mesh_nodes

    def _forward_ensemble(self, latent_mesh_nodes: torch.Tensor, edge_index: torch.Tensor, noise_vector: torch.Tensor,
                          input_edge_attr: Optional[torch.Tensor], batch: int, members: int) -> torch.Tensor:
        """mesh rows [batch M, .] shared by the ``members`` of a sample, ``noise_vector`` [batch members, .] (row b members + n)
        -> [batch members M, .].  The first block's TransformerConv sees no noise and runs at ``batch``; its norm fans every row
        out into the members' rows; the later blocks run at ``batch members``."""
        edges_emb = self._edges(input_edge_attr)
        M = int(latent_mesh_nodes.shape[0]) // batch
        if self.sparse:  # cond_norm_1 sees the noise before anything else: the rows fan out first, every block runs at batch members
            ident = (None, torch.arange(M + 1, dtype=torch.int32, device=latent_mesh_nodes.device))
            x = _LinearGatherGrouped.apply(None, None, None, ((None, M, members, ident),), batch * members, M,
                                           _rows_in(latent_mesh_nodes, "latent_mesh_nodes"))
            for cond_transformer in self.cond_transformers:
                x = cond_transformer._forward_shared(x, edge_index, _rows_in(noise_vector, "noise_vector"), batch * members)
            return x
        first = self.cond_transformers[0]
        x = first.transformer_conv._forward_shared(latent_mesh_nodes, edge_index, edges_emb, batch)
        norm = first.cond_norm
        cond = _rows_in(noise_vector, "noise_vector")
        scale = _Linear.apply(cond, norm.linear_scale.weight, norm.linear_scale.bias, False)
        bias = _Linear.apply(cond, norm.linear_bias.weight, norm.linear_bias.bias, False)
        x = _CondLayerNormFanout.apply(x, scale, bias, M, members, _act_name(first.activation))
        for cond_transformer in list(self.cond_transformers)[1:]:
            x = cond_transformer._forward_shared(x, edge_index, edges_emb, noise_vector, batch * members)
        return x


# ---------------------------------------------------------------------------------------------------------------------
# the decoder on grouped copies
# ---------------------------------------------------------------------------------------------------------------------
def _decoder_ensemble(dec: Decoder, mesh: torch.Tensor, grid: torch.Tensor, edge_attr: torch.Tensor, edge_index: torch.Tensor,
                      batch: int, members: int) -> torch.Tensor:
    """``Decoder._forward_shared`` on ``batch members`` copies whose grid latents [batch G, .] are shared by the members of a
    sample: mesh rows [batch members M, .] -> [batch members G, out].  The receiver-side tables of the interaction network - the
    layer-1 products of ``mlp_edges`` and ``mlp_nodes`` on receiver rows, and the residual - are formed on batch G rows; copy c
    reads block c // members."""
    copies = batch * members
    M, G = int(mesh.shape[0]) // copies, int(grid.shape[0]) // batch
    gnn = dec.gnn
    ds, dr, _ = gnn._dims
    ep = edge_plan(edge_index, M, G)
    E = ep.num_edges
    edges_emb = dec.edges_mlp(edge_attr)
    l0 = gnn.mlp_edges.linears[0]
    w0 = l0.weight
    grid = _rows_in(grid, "input_grid_nodes")
    p_recv = _Linear.apply(grid, w0[:, :dr], None, False)  # [batch G, .]
    p_send = _Linear.apply(mesh, w0[:, dr:dr + ds], None, False)  # [copies M, .]
    p_edge = _Linear.apply(edges_emb, w0[:, dr + ds:], l0.bias, False)  # [E, .]
    meta = ((None, 0, 1, (None, ep.plan.identity_ptr())), (ep.dst32, G, members, (ep.perm32, ep.plan.dst_ptr())),
            (ep.src32, M, 1, ep.by_src))
    h = _LinearGatherGrouped.apply(None, None, None, meta, copies, E, p_edge, p_recv, p_send)
    msg = gnn.mlp_edges.tail(gnn.mlp_edges._layer(0, h))
    aggr = _SegmentSumShared.apply(msg, ep, copies)
    if gnn.scale_factor != 1.0:
        aggr = _RowScale.apply(aggr, torch.full((copies * G,), float(gnn.scale_factor), dtype=torch.float32, device=aggr.device))
    n0 = gnn.mlp_nodes.linears[0]
    ident = (None, ep.ident_dst)
    p_node = _Linear.apply(grid, n0.weight[:, :dr], None, False)  # [batch G, .]
    h = _LinearGatherGrouped.apply(aggr, n0.weight[:, dr:], n0.bias, ((None, G, members, ident),), copies, G, p_node)
    update = gnn.mlp_nodes.tail(gnn.mlp_nodes._layer(0, h))
    latent = _LinearGatherGrouped.apply(None, None, None, ((None, G, members, ident), (None, G, 1, ident)), copies, G, grid, update)
    return dec.grid_mlp_final(latent)


# ---------------------------------------------------------------------------------------------------------------------
# fgn/model.py
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class FunctionalGenerativeNetworkConfig:
    """Configuration for FunctionalGenerativeNetwork model."""

    grid_lon: np.ndarray
    grid_lat: np.ndarray
    input_features_dim: int
    output_features_dim: int
    noise_dimension: int
    hidden_dims: list = None
    num_blocks: int = 24
    num_heads: int = 4
    splits: int = 6
    num_hops: int = 6
    device: torch.device = torch.device("cpu")
    sparse: object = False  # False, True (the reference's DGL backend: raises) or "native"
    use_edges_features: bool = True
    scale_factor: float = 1.0

    def __post_init__(self):
        if self.hidden_dims is None:
            self.hidden_dims = [768, 768]

    def build(self) -> "FunctionalGenerativeNetwork":
        return FunctionalGenerativeNetwork(
            grid_lon=self.grid_lon, grid_lat=self.grid_lat, input_features_dim=self.input_features_dim,
            output_features_dim=self.output_features_dim, noise_dimension=self.noise_dimension, hidden_dims=self.hidden_dims,
            num_blocks=self.num_blocks, num_heads=self.num_heads, splits=self.splits, num_hops=self.num_hops, device=self.device,
            sparse=self.sparse, use_edges_features=self.use_edges_features, scale_factor=self.scale_factor)


class FunctionalGenerativeNetwork(torch.nn.Module, PyTorchModelHubMixin):
    """Functional Generative Network: an (encoder, noise-conditioned processor, decoder) model over the grid-to-mesh, k-hop mesh
    and mesh-to-grid graphs whose forward returns an ensemble of next states."""

    def __init__(self, grid_lon: np.ndarray, grid_lat: np.ndarray, input_features_dim: int, output_features_dim: int,
                 noise_dimension: int, hidden_dims: list[int] = [768, 768], num_blocks: int = 24, num_heads: int = 4, splits: int = 6,
                 num_hops: int = 6, device: torch.device = torch.device("cpu"), sparse=False, use_edges_features: bool = True,
                 scale_factor: float = 1.0):
        super().__init__()
        self.num_lon = len(grid_lon)
        self.num_lat = len(grid_lat)
        self.input_features_dim = input_features_dim
        self.output_features_dim = output_features_dim
        self.use_edges_features = use_edges_features
        self.noise_dimension = noise_dimension

        self.graphs = GraphBuilder(grid_lon=grid_lon, grid_lat=grid_lat, splits=splits, num_hops=num_hops, device=device,
                                   add_edge_features_to_khop=use_edges_features)
        self._register_graph()

        self.encoder = Encoder(grid_dim=input_features_dim + self.graphs.grid_nodes_dim, mesh_dim=self.graphs.mesh_nodes_dim,
                               edge_dim=self.graphs.g2m_edges_dim, hidden_dims=hidden_dims, activation_layer=torch.nn.SiLU,
                               use_layer_norm=True, scale_factor=scale_factor)
        if sparse and use_edges_features:
            raise ValueError("Sparse processor don't support edges features.")
        self.processor = Processor(latent_dim=hidden_dims[-1], edges_dim=self.graphs.mesh_edges_dim if use_edges_features else None,
                                   hidden_dims=hidden_dims, num_blocks=num_blocks, num_heads=num_heads, noise_emb_dim=noise_dimension,
                                   activation_layer=torch.nn.SiLU, use_layer_norm=True, sparse=sparse)
        self.decoder = Decoder(edges_dim=self.graphs.m2g_edges_dim, output_dim=output_features_dim, hidden_dims=hidden_dims,
                               activation_layer=torch.nn.SiLU, use_layer_norm=True)

    _register_graph = Denoiser._register_graph  # (the same 14 non-persistent buffers, in the same order)

    # ---- inputs -----------------------------------------------------------------------------------------------------------
    def _check_input(self, previous_weather_state: torch.Tensor, num_ensemble: int) -> int:
        exp = (self.num_lon, self.num_lat, self.input_features_dim)
        if previous_weather_state.dim() != 4 or tuple(previous_weather_state.shape[1:]) != exp or previous_weather_state.shape[0] < 1:
            raise ValueError("The shape of the input tensor doesn't match with the initialization parameters: expected "
                             f"(batch_size, {exp[0]}, {exp[1]}, {exp[2]}), got {tuple(previous_weather_state.shape)}.")
        if int(num_ensemble) != num_ensemble or num_ensemble < 1:
            raise ValueError(f"num_ensemble must be a positive integer, got {num_ensemble}.")
        return int(previous_weather_state.shape[0])

    def _noise(self, previous_weather_state, batch: int, members: int, noise_vectors, generator) -> torch.Tensor:
        """[batch, members, noise_dimension]: the given vectors, or member n's drawn as the reference draws them - one
        ``torch.randn((batch, noise_dimension))`` per member, in member order."""
        if noise_vectors is None:
            draws = [torch.randn((batch, self.noise_dimension), device=previous_weather_state.device, generator=generator)
                     for _ in range(members)]
            return torch.stack(draws, dim=1)
        exp = (batch, members, self.noise_dimension)
        if tuple(noise_vectors.shape) != exp:
            raise ValueError(f"noise_vectors must have shape {exp} (batch_size, num_ensemble, noise_dimension), got "
                             f"{tuple(noise_vectors.shape)}.")
        return noise_vectors

    def _grid_input(self, previous_weather_state: torch.Tensor, batch: int) -> torch.Tensor:
        """The encoder's grid rows [batch G, in + static]: "b lon lat f -> (b lon lat) f" beside the static grid features, joined
        in one concatenation (the [G, .] table enters as an expanded view)."""
        static = self.g2m_grid_nodes
        x = previous_weather_state.reshape(batch, -1, self.input_features_dim)
        return torch.cat([x, static.unsqueeze(0).expand(batch, -1, -1)], dim=-1).reshape(-1, self.input_features_dim + int(static.shape[1]))

    def forward(self, previous_weather_state: torch.Tensor, num_ensemble: int = 2, *, noise_vectors: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """previous_weather_state [B, lon, lat, in] -> [B, num_ensemble, lon, lat, out] (all members at every B).
        ``noise_vectors`` [B, num_ensemble, noise_dimension] supplies the conditioning; without it member n's vectors are
        ``torch.randn((B, noise_dimension), device=..., generator=generator)``, drawn once per member in member order."""
        B = self._check_input(previous_weather_state, num_ensemble)
        N = int(num_ensemble)
        noise = self._noise(previous_weather_state, B, N, noise_vectors, generator).reshape(B * N, self.noise_dimension)
        grid_in = self._grid_input(previous_weather_state, B)
        latent_grid, latent_mesh = self.encoder._forward_shared(grid_in, self.g2m_mesh_nodes, self.g2m_edge_attr, self.g2m_edge_index, B)
        latent_mesh = self.processor._forward_ensemble(latent_mesh, self.khop_mesh_edge_index, noise,
                                                       self.khop_mesh_edge_attr if self.use_edges_features else None, B, N)
        out = _decoder_ensemble(self.decoder, latent_mesh, latent_grid, self.m2g_edge_attr, self.m2g_edge_index, B, N)
        return out.reshape(B, N, self.num_lon, self.num_lat, self.output_features_dim)


def _forward_member_loop(model: FunctionalGenerativeNetwork, previous_weather_state: torch.Tensor,
                         noise_vectors: torch.Tensor) -> torch.Tensor:
    """``model``'s forward by the reference's route on this package's kernels: for every member, encoder -> processor -> decoder
    on the B samples (the batch-shared forms of the layers at batch B), the results stacked - all members, at B = 1 too.  For
    comparison and measurement; ``FunctionalGenerativeNetwork.forward`` is the ensemble-shared route."""
    N = int(noise_vectors.shape[1]) if noise_vectors.dim() == 3 else 0
    B = model._check_input(previous_weather_state, max(N, 1))
    noise_vectors = model._noise(previous_weather_state, B, N, noise_vectors, None)
    predictions = []
    for n in range(N):
        grid_in = model._grid_input(previous_weather_state, B)
        latent_grid, latent_mesh = model.encoder._forward_shared(grid_in, model.g2m_mesh_nodes, model.g2m_edge_attr,
                                                                 model.g2m_edge_index, B)
        latent_mesh = model.processor._forward_shared(latent_mesh, model.khop_mesh_edge_index, noise_vectors[:, n].contiguous(),
                                                      model.khop_mesh_edge_attr if model.use_edges_features else None, B)
        out = model.decoder._forward_shared(latent_mesh, latent_grid, model.m2g_edge_attr, model.m2g_edge_index, B)
        predictions.append(out.reshape(B, model.num_lon, model.num_lat, model.output_features_dim))
    return torch.stack(predictions, dim=1)
