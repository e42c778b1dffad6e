"""A restatement of the reference's sparse GenCast processor (graph_weather/models/gencast/layers/experimental/
sparse_transformer.py: ``SparseAttention``, ``SparseTransformer``; the ``sparse=True`` branch of gencast/layers/processor.py and
fgn/layers/processor.py) as plain torch compositions over a ``state_dict``: float64 for the oracle, float32 on the CPU for the
yardstick.  Nothing here touches the HIP kernels or graph_weather_amd.

``dgl`` is not installed and not part of the reference tree.  The four things of ``dgl.sparse`` the reference calls are restated
here from DGL's documentation as a torch-only stand-in (``spmatrix``, ``bsddmm``, ``SparseMatrix.softmax``, ``bspmm``) that
scripts/gen_gencast_sparse_golden.py registers as ``dgl`` / ``dgl.sparse`` to run the reference's own classes.  The reading: entry
e of ``spmatrix(indices)`` sits at (row ``indices[0, e]``, column ``indices[1, e]``); the matrix is not coalesced, so every entry
is its own term (a duplicate counts twice); ``softmax`` normalises over the entries of a row, per head.  DGL's arithmetic is
restated, not pinned.

The model restatements reuse tests/gencast_model_oracle.py, tests/genda_oracle.py and tests/fgn_oracle.py with the processor
swapped (``sparse_models``): those files call ``go.processor`` / ``fo.fgn_processor`` by name, and the sparse processors take the
same arguments.

What was measured at the recorded seeds is in the comment at ``MODEL_CASES``.
"""
from __future__ import annotations

import contextlib
import types
from typing import Dict

import numpy as np
import torch

from . import fgn_oracle as fo
from . import gencast_model_oracle as mo
from . import gencast_oracle as go
from . import genda_oracle as do
from .cafa_oracle import fill_, params  # noqa: F401


# ---- the stand-in for dgl.sparse -----------------------------------------------------------------------------------------------
class SparseMatrix:
    """COO entries (row, col) of an [n_rows, n_cols] matrix with one value row per entry (None: ones); not coalesced."""

    def __init__(self, row, col, shape, val=None):
        self.row, self.col, self.shape, self.val = row, col, tuple(shape), val

    def softmax(self):
        """Softmax over the entries of each row (the last sparse dimension), per trailing value column."""
        s = self.val
        idx = self.row[:, None].expand_as(s)
        smax = torch.full((self.shape[0], s.shape[1]), -float("inf"), dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax",
                                                                                                      include_self=True)
        ex = (s - smax[self.row]).exp()
        den = torch.zeros((self.shape[0], s.shape[1]), dtype=s.dtype).index_add_(0, self.row, ex)
        return SparseMatrix(self.row, self.col, self.shape, ex / den[self.row])


def spmatrix(indices, val=None, shape=None):
    return SparseMatrix(indices[0], indices[1], shape, val)


def bsddmm(A: SparseMatrix, X1: torch.Tensor, X2: torch.Tensor) -> SparseMatrix:
    """Batched sampled dense-dense product: X1 [L, M, K], X2 [M, N, K] -> value [e, k] = sum_m X1[row_e, m, k] X2[m, col_e, k]."""
    return SparseMatrix(A.row, A.col, A.shape, (X1[A.row] * X2.transpose(0, 1)[A.col]).sum(dim=1))


def bspmm(A: SparseMatrix, X: torch.Tensor) -> torch.Tensor:
    """Batched sparse-dense product: A values [E, K], X [N, M, K] -> [L, M, K] with out[i, m, k] = sum_{e in row i} A[e, k] X[col_e, m, k]."""
    out = torch.zeros((A.shape[0],) + tuple(X.shape[1:]), dtype=X.dtype)
    return out.index_add_(0, A.row, A.val[:, None, :] * X[A.col])


def dgl_modules() -> Dict[str, types.ModuleType]:
    """name -> module to put into sys.modules before the reference's sparse_transformer.py is executed."""
    mods = {n: types.ModuleType(n) for n in ("dgl", "dgl.sparse")}
    mods["dgl"].sparse = mods["dgl.sparse"]
    for f in (SparseMatrix, spmatrix, bsddmm, bspmm):
        setattr(mods["dgl.sparse"], f.__name__, f)
    return mods


# ---- the classes over a state_dict ---------------------------------------------------------------------------------------------
def sparse_attention_core(q, k, v, edge_index, num_heads: int):
    """q (already scaled), k, v [N, D] in the reference's interleaved layout (column c = (d = c // nh, h = c % nh)) -> [N, D]."""
    N, D = q.shape
    dh = D // num_heads
    q3, k3, v3 = (t.reshape(N, dh, num_heads) for t in (q, k, v))
    adj = spmatrix(edge_index, shape=(N, N))
    attn = bsddmm(adj, q3, k3.transpose(1, 0)).softmax()
    return bspmm(attn, v3).reshape(N, -1)


def sparse_attention(p, key, x, edge_index, num_heads: int):
    D = p[key + ".q_proj.weight"].shape[0]
    q = go.linear(p, key + ".q_proj", x) * (D // num_heads) ** -0.5
    out = sparse_attention_core(q, go.linear(p, key + ".k_proj", x), go.linear(p, key + ".v_proj", x), edge_index, num_heads)
    return go.linear(p, key + ".out_proj", out)


def sparse_transformer(p, key, x, edge_index, cond, num_heads: int, act: str, norm_first: bool = True):
    f = go._act(act)

    def mlp(t):
        return go.linear(p, key + ".mlp.2", f(go.linear(p, key + ".mlp.0", t)))

    if norm_first:
        x = x + sparse_attention(p, key + ".sparse_attention", go.cond_layer_norm(p, key + ".cond_norm_1", x, cond), edge_index, num_heads)
        return x + mlp(go.cond_layer_norm(p, key + ".cond_norm_2", x, cond))
    x = go.cond_layer_norm(p, key + ".cond_norm_1", x + sparse_attention(p, key + ".sparse_attention", x, edge_index, num_heads), cond)
    return go.cond_layer_norm(p, key + ".cond_norm_2", x + mlp(x), cond)


def processor(p, cfg, x, edge_index, noise_levels, edge_attr=None):
    """gencast/layers/processor.py with sparse=True: the noise embedding conditions ``num_blocks`` identical blocks; edge
    attributes are ignored."""
    emb = go.fourier_embedding(p, "fourier_embedder", noise_levels, cfg["num_frequencies"], cfg["base_period"])
    for b in range(cfg["num_blocks"]):
        x = sparse_transformer(p, "cond_transformers.%d" % b, x, edge_index, emb, cfg["num_heads"], cfg.get("activation_layer", "ReLU"))
    return x


def fgn_processor(p, cfg, x, edge_index, noise_vector, edge_attr=None):
    """fgn/layers/processor.py with sparse=True: the noise vector itself is the conditioning."""
    for b in range(cfg["num_blocks"]):
        x = sparse_transformer(p, "cond_transformers.%d" % b, x, edge_index, noise_vector, cfg["num_heads"],
                               cfg.get("activation_layer", "ReLU"))
    return x


@contextlib.contextmanager
def sparse_models():
    """Inside, ``mo.denoiser_forward``, ``do.genda_forward`` / ``do.genda_guided`` and ``fo.fgn_forward`` run the sparse processors."""
    saved = go.processor, fo.fgn_processor
    go.processor, fo.fgn_processor = processor, fgn_processor
    try:
        yield
    finally:
        go.processor, fo.fgn_processor = saved


def dense_masked_attention(q, k, v, edge_index, num_heads: int):
    """``sparse_attention_core`` for a duplicate-free mask, written without the stand-in: a dense [N, N] masked softmax per head."""
    N, D = q.shape
    dh = D // num_heads
    mask = torch.zeros((N, N), dtype=torch.bool)
    mask[edge_index[0], edge_index[1]] = True
    out = torch.zeros_like(q)
    for h in range(num_heads):
        cols = torch.arange(dh) * num_heads + h  # head h owns every nh-th column
        s = (q[:, cols] @ k[:, cols].T).masked_fill(~mask, -float("inf"))
        a = torch.softmax(s, dim=1)
        a = torch.where(mask.any(dim=1, keepdim=True), a, torch.zeros_like(a))  # a row without entries: zeros, not NaN
        out[:, cols] = a @ v[:, cols]
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
# layer cases: name -> (kind, constructor keywords (activation_layer by name), n_nodes, seed)
_BLOCK = dict(input_dim=64, output_dim=64, num_heads=4)
_PROC = dict(latent_dim=32, hidden_dims=[40, 24], num_heads=4, num_frequencies=8, base_period=16, noise_emb_dim=12, sparse=True)
_FPROC = dict(latent_dim=32, hidden_dims=[40, 24], num_heads=4, noise_emb_dim=6, sparse=True)
CASES = {
    "gencast_sparse_attention": ("attention", dict(input_dim=12, output_dim=24, num_heads=4), 37, 61),
    "gencast_sparse_block_pre_relu": ("block", dict(_BLOCK, conditioning_dim=16, activation_layer="ReLU", norm_first=True), 37, 62),
    "gencast_sparse_block_post_relu": ("block", dict(_BLOCK, conditioning_dim=3, activation_layer="ReLU", norm_first=False), 37, 63),
    "gencast_sparse_block_pre_silu": ("block", dict(_BLOCK, conditioning_dim=3, activation_layer="SiLU", norm_first=True), 37, 64),
    "gencast_sparse_block_post_silu": ("block", dict(_BLOCK, conditioning_dim=16, activation_layer="SiLU", norm_first=False), 37, 65),
    "gencast_sparse_processor_2": ("processor", dict(_PROC, num_blocks=2, activation_layer="SiLU"), 37, 66),
    "gencast_sparse_processor_3": ("processor", dict(_PROC, num_blocks=3), 37, 67),
    "gencast_sparse_fgn_processor_2": ("fgn_processor", dict(_FPROC, num_blocks=2, activation_layer="SiLU"), 37, 68),
    "gencast_sparse_fgn_processor_3": ("fgn_processor", dict(_FPROC, num_blocks=3), 37, 69),
}
# model cases on a 16 x 9 grid (``model_grid``): name -> (kind, constructor keywords without the grid, batch, seed).
# Seeds: every figure of tests/test_gpu_gencast_sparse.py is printed before it is asserted; the seeds below are the first and only
# ones tried, and all three cases passed on an MI355X.  The bar is the project's (4 x the float32 CPU restatement's own error, floor
# 1e-6 of the maximum) and is not widened.  It is tight for the gradients of the existing row kernels, as tests/genda_oracle.py
# records for GenDA: the worst figure was 3.89 x on ``processor.cond_transformers.1.cond_norm_2.linear_scale.bias`` through
# ``guided_forward`` (the grouped ConditionalLayerNorm kernel's gradient), 3.47 x on block 0's, 3.39 x on a decoder bias of FGN; the
# attention kernels' own cases stay below 3.3 x.  The gradient of ``k_proj.bias`` is zero in exact arithmetic (a shift of every key
# leaves the softmax unchanged), so there both sides are rounding noise (3.0 x measured) and the yardstick depends on the host CPU's
# float32 sums.
_MODEL = dict(hidden_dims=[16, 16], num_blocks=2, num_heads=4, splits=1, num_hops=1, sparse=True, use_edges_features=False)
MODEL_CASES = {
    "gencast_sparse_denoiser": ("denoiser", dict(_MODEL, input_features_dim=3, output_features_dim=5), 2, 71),
    "gencast_sparse_genda": ("genda", dict(_MODEL, input_features_dim=3, output_features_dim=5), 2, 72),
    "gencast_sparse_fgn": ("fgn", dict(_MODEL, input_features_dim=3, output_features_dim=5, noise_dimension=6), 2, 73),
}
GRID_LON0, GRID_LAT0 = 2.75, 3.25  # shifted until every grid point's closest-face gap at splits 1 is >= 1e-5 (the generator asserts it)
SIGMA = (0.5, 3.0)
FGN_MEMBERS = 3
GAMMA = do.GAMMA


def model_grid():
    """The 16 x 9 grid of the model cases."""
    return GRID_LON0 + 22.5 * np.arange(16), np.linspace(-80, 80, 9) + GRID_LAT0


def sparse_graph(rs, n: int) -> np.ndarray:
    """Shuffled asymmetric COO [2, E] on n nodes: row i attends to i % 7 columns drawn without replacement (row 0 and every 7th
    row attend to nothing), so the transposed mask is a different one and there are no duplicates."""
    rows, cols = [], []
    for i in range(n):
        c = rs.choice(n, size=i % 7, replace=False)
        rows += [i] * len(c)
        cols += c.tolist()
    ei = np.stack([np.asarray(rows), np.asarray(cols)]).astype(np.int64)
    return ei[:, rs.permutation(ei.shape[1])]


def _f32(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def case_inputs(name: str) -> Dict[str, torch.Tensor]:
    kind, cfg, n, seed = CASES[name]
    rs = np.random.RandomState(seed)
    ei = torch.from_numpy(sparse_graph(rs, n))
    if kind == "attention":
        return dict(x=_f32(rs, n, cfg["input_dim"]), edge_index=ei)
    if kind == "block":
        return dict(x=_f32(rs, n, cfg["input_dim"]), edge_index=ei, cond=_f32(rs, n, cfg["conditioning_dim"]))
    if kind == "processor":  # one noise level per node, two levels over the nodes
        noise = np.where(np.arange(n) < n // 2, rs.uniform(-2.0, 2.0), rs.uniform(-2.0, 2.0)).astype(np.float32)[:, None]
        return dict(x=_f32(rs, n, cfg["latent_dim"]), edge_index=ei, cond=torch.from_numpy(noise))
    return dict(x=_f32(rs, n, cfg["latent_dim"]), edge_index=ei, cond=_f32(rs, n, cfg["noise_emb_dim"]))


def build(classes, name: str, sparse=None):
    """The module of ``classes`` (a namespace with SparseAttention, SparseTransformer, Processor, FgnProcessor) with the seeded
    parameters; ``sparse`` replaces the case's ``sparse=True`` (this package takes "native")."""
    kind, cfg, _, seed = CASES[name]
    kw = dict(cfg)
    if "activation_layer" in kw:
        kw["activation_layer"] = go.ACTS[kw["activation_layer"]]
    if sparse is not None and "sparse" in kw:
        kw["sparse"] = sparse
    cls = {"attention": "SparseAttention", "block": "SparseTransformer", "processor": "Processor", "fgn_processor": "FgnProcessor"}[kind]
    return fill_(getattr(classes, cls)(**kw), seed)


def call(module, name: str, inp, adj=None):
    """Run a module (the reference's or ours) on a case's inputs; ``adj``: what the reference's SparseAttention takes in place of
    ``edge_index`` (a ``spmatrix``)."""
    if CASES[name][0] == "attention":
        return module(inp["x"], inp["edge_index"] if adj is None else adj)
    return module(inp["x"], inp["edge_index"], inp["cond"])


def run(name: str, p, inp):
    """The restatement on a case's inputs (already of p's dtype)."""
    kind, cfg, _, _ = CASES[name]
    if kind == "attention":
        return sparse_attention({"a." + k: v for k, v in p.items()}, "a", inp["x"], inp["edge_index"], cfg["num_heads"])
    if kind == "block":
        return sparse_transformer({"b." + k: v for k, v in p.items()}, "b", inp["x"], inp["edge_index"], inp["cond"], cfg["num_heads"],
                                  cfg["activation_layer"], cfg["norm_first"])
    if kind == "processor":
        return processor(p, cfg, inp["x"], inp["edge_index"], inp["cond"])
    return fgn_processor(p, cfg, inp["x"], inp["edge_index"], inp["cond"])


def cast(inp, dtype, requires_grad: bool = False):
    return go.cast(inp, dtype, requires_grad)


def model_kwargs(name: str, sparse=True) -> dict:
    lon, lat = model_grid()
    return dict(grid_lon=lon, grid_lat=lat, **dict(MODEL_CASES[name][1], sparse=sparse))


def model_inputs(name: str):
    """denoiser: (corrupted_targets, prev_inputs, noise_levels); genda: those and (sensor_mask, sensor_values); fgn:
    (previous_weather_state, noise_vectors [B, N, noise]) - float32 from the case's seed."""
    kind, kw, B, seed = MODEL_CASES[name]
    lon, lat = model_grid()
    rs = np.random.RandomState(seed)
    shape = (B, len(lon), len(lat))
    if kind == "fgn":
        x = rs.standard_normal(shape + (kw["input_features_dim"],)).astype(np.float32)
        noise = rs.standard_normal((B, FGN_MEMBERS, kw["noise_dimension"])).astype(np.float32)
        return torch.from_numpy(x), torch.from_numpy(noise)
    z = rs.standard_normal(shape + (kw["output_features_dim"],)).astype(np.float32)
    x = rs.standard_normal(shape + (2 * kw["input_features_dim"],)).astype(np.float32)
    s = np.array([SIGMA[i % len(SIGMA)] for i in range(B)], dtype=np.float32)[:, None]
    out = [z, x, s]
    if kind == "genda":
        mask = (rs.random_sample(shape + (1,)) < do.MASK_P).astype(np.float32)
        out += [mask, (mask * rs.standard_normal(mask.shape)).astype(np.float32)]
    return tuple(torch.from_numpy(a) for a in out)


def model_forward(name: str, p, kw, graphs, inputs, guided: bool = False):
    """The model restatement of a case on tensors of p's dtype with the sparse processors in place."""
    kind = MODEL_CASES[name][0]
    with sparse_models():
        if kind == "denoiser":
            return mo.denoiser_forward(p, kw, graphs, *inputs)
        if kind == "genda":
            return (do.genda_guided if guided else do.genda_forward)(p, kw, graphs, *inputs)
        return fo.fgn_forward(p, kw, graphs, *inputs)


def bar(err32: float, ref_max: float) -> float:
    return do.bar(err32, ref_max)
