"""A restatement of the reference's GenCast layers (graph_weather/models/gencast/layers: modules, encoder, processor, decoder),
written from their arithmetic as plain torch compositions over a ``state_dict``: float64 for the oracle, float32 on the CPU for
the yardstick (what fp32 arithmetic in the reference's own order of operations costs).  Nothing here touches the HIP kernels.

The two classes of ``torch_geometric`` the reference builds on are not installed and not part of the reference tree; their
documented arithmetic is restated here, once as functions over a ``state_dict`` (``transformer_conv``, ``interaction``) and
once as the stand-in classes ``MessagePassing`` / ``TransformerConv`` that scripts/gen_gencast_golden.py registers as
``torch_geometric.nn`` / ``torch_geometric.nn.conv`` to run the reference's own files.  PyG's arithmetic and key names are
restated, not pinned.

It also carries the per-key seeded ``fill_`` of tests/cafa_oracle.py and the case table of scripts/gen_gencast_golden.py.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .cafa_oracle import fill_, params  # noqa: F401  (per-key seeded weights; state_dict -> {key: tensor of a dtype})

ACTS = {"ReLU": nn.ReLU, "SiLU": nn.SiLU}


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------
def segment_softmax(s: torch.Tensor, index: torch.Tensor, n: int) -> torch.Tensor:
    """softmax of s [E, H] over the rows that share ``index``: the segment maximum (a constant for autograd) is subtracted and the
    sum gets + 1e-16."""
    idx = index[:, None].expand_as(s)
    smax = torch.full((n, s.shape[1]), -math.inf, dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = (s - smax[index]).exp()
    den = torch.zeros((n, s.shape[1]), dtype=s.dtype).index_add_(0, index, ex) + 1e-16
    return ex / den[index]


def graph_attention(q, k, v, e, src, dst, n_dst: int, heads: int, mean: bool):
    """q [n_dst, H C], k, v [n_src, H C], e [E, H C] or None -> [n_dst, H C] (or [n_dst, C], the mean over the heads)."""
    C = q.shape[1] // heads
    qi, kj, vj = q.view(-1, heads, C)[dst], k.view(-1, heads, C)[src], v.view(-1, heads, C)[src]
    if e is not None:
        ev = e.view(-1, heads, C)
        kj, vj = kj + ev, vj + ev
    alpha = segment_softmax((qi * kj).sum(-1) / math.sqrt(C), dst, n_dst)
    out = torch.zeros((n_dst, heads, C), dtype=q.dtype).index_add_(0, dst, alpha[..., None] * vj)
    return out.mean(dim=1) if mean else out.reshape(n_dst, heads * C)


def linear(p, key, x):
    y = x @ p[key + ".weight"].T
    return y + p[key + ".bias"] if key + ".bias" in p else y


def transformer_conv(p, key, x, edge_index, edge_attr, heads: int, concat: bool):
    """TransformerConv(beta=True, root_weight=True, bias=True) as the issue fixes it."""
    src, dst = edge_index[0], edge_index[1]
    q, k, v = linear(p, key + ".lin_query", x), linear(p, key + ".lin_key", x), linear(p, key + ".lin_value", x)
    e = linear(p, key + ".lin_edge", edge_attr) if edge_attr is not None else None
    out = graph_attention(q, k, v, e, src, dst, x.shape[0], heads, not concat)
    x_r = linear(p, key + ".lin_skip", x)
    g = linear(p, key + ".lin_beta", torch.cat([out, x_r, out - x_r], dim=-1)).sigmoid()
    return g * x_r + (1 - g) * out


class MessagePassing(nn.Module):
    """``MessagePassing(aggr="add", flow="source_to_target")`` as InteractionNetwork uses it."""

    def __init__(self, aggr="add", flow="source_to_target"):
        super().__init__()
        assert aggr == "add" and flow == "source_to_target"

    def propagate(self, edge_index, x, edge_attr, size):
        x_send, x_recv = x
        msg = self.message(x_i=x_recv[edge_index[1]], x_j=x_send[edge_index[0]], edge_attr=edge_attr)
        return torch.zeros((size[1], msg.shape[1]), dtype=msg.dtype).index_add_(0, edge_index[1], msg)


class TransformerConv(nn.Module):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True,
                 root_weight=True):
        super().__init__()
        assert beta and root_weight and bias and dropout == 0.0
        self.heads, self.concat = heads, concat
        hc = heads * out_channels
        self.lin_key = nn.Linear(in_channels, hc)
        self.lin_query = nn.Linear(in_channels, hc)
        self.lin_value = nn.Linear(in_channels, hc)
        if edge_dim is not None:
            self.lin_edge = nn.Linear(edge_dim, hc, bias=False)
        self.lin_skip = nn.Linear(in_channels, hc if concat else out_channels)
        self.lin_beta = nn.Linear(3 * (hc if concat else out_channels), 1, bias=False)

    def forward(self, x, edge_index, edge_attr=None):
        p = {"c." + k: v for k, v in self.state_dict(keep_vars=True).items()}
        return transformer_conv(p, "c", x, edge_index, edge_attr, self.heads, self.concat)


# ---- the eight classes over a state_dict -------------------------------------------------------------------------------------
def _act(name):
    return {"ReLU": F.relu, "SiLU": F.silu, None: (lambda x: x)}[name]


def mlp(p, key, x, act: str, activate_final: bool = False):
    n = sum(1 for k in p if k.startswith(key + ".linears.") and k.endswith(".weight"))
    f = _act(act)
    for i in range(n - 1):
        x = f(linear(p, "%s.linears.%d" % (key, i), x))
    x = linear(p, "%s.linears.%d" % (key, n - 1), x)
    if activate_final:
        x = f(x)
    if key + ".norm_layer.weight" in p:
        x = F.layer_norm(x, (x.shape[-1],), p[key + ".norm_layer.weight"], p[key + ".norm_layer.bias"], 1e-5)
    return x


def interaction(p, key, x_send, x_recv, edge_index, edge_attr, act: str, scale_factor: float = 1.0):
    msg = scale_factor * mlp(p, key + ".mlp_edges", torch.cat((x_recv[edge_index[1]], x_send[edge_index[0]], edge_attr), dim=-1), act)
    aggr = torch.zeros((x_recv.shape[0], msg.shape[1]), dtype=msg.dtype).index_add_(0, edge_index[1], msg)
    return mlp(p, key + ".mlp_nodes", torch.cat((x_recv, aggr), dim=-1), act)


def fourier_features(t, num_frequencies: int, base_period):
    freqs = torch.exp(-math.log(base_period) * torch.arange(0, num_frequencies, dtype=torch.float32) / num_frequencies).to(t.dtype)
    args = t * freqs[None, :]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def fourier_embedding(p, key, t, num_frequencies: int, base_period):
    h = F.silu(linear(p, key + ".mlp.0", fourier_features(t, num_frequencies, base_period)))
    return linear(p, key + ".mlp.2", h)


def cond_layer_norm(p, key, x, cond):
    scale, bias = linear(p, key + ".linear_scale", cond), linear(p, key + ".linear_bias", cond)
    return scale * F.layer_norm(x, (x.shape[-1],), None, None, 1e-5) + bias


def cond_transformer_block(p, key, x, edge_index, edge_attr, cond, heads: int, concat: bool, act: Optional[str]):
    x = transformer_conv(p, key + ".transformer_conv", x, edge_index, edge_attr, heads, concat)
    if key + ".cond_norm.linear_scale.weight" in p:
        x = cond_layer_norm(p, key + ".cond_norm", x, cond)
    return _act(act)(x)


def encoder(p, cfg, grid, mesh, edge_attr, edge_index):
    act = cfg.get("activation_layer", "ReLU")
    g, m, e = mlp(p, "grid_mlp", grid, act), mlp(p, "mesh_mlp", mesh, act), mlp(p, "edges_mlp", edge_attr, act)
    lm = m + interaction(p, "gnn", g, m, edge_index, e, act, cfg.get("scale_factor", 1.0))
    return g + mlp(p, "grid_mlp_final", g, act), lm


def decoder(p, cfg, mesh, grid, edge_attr, edge_index):
    act = cfg.get("activation_layer", "ReLU")
    e = mlp(p, "edges_mlp", edge_attr, act)
    return mlp(p, "grid_mlp_final", grid + interaction(p, "gnn", mesh, grid, edge_index, e, act), act)


def processor(p, cfg, x, edge_index, noise_levels, edge_attr=None):
    act = cfg.get("activation_layer", "ReLU")
    emb = fourier_embedding(p, "fourier_embedder", noise_levels, cfg["num_frequencies"], cfg["base_period"])
    e = mlp(p, "edges_mlp", edge_attr, act) if cfg.get("edges_dim") is not None else None
    nb = cfg["num_blocks"]
    for b in range(nb):
        last = b == nb - 1
        x = cond_transformer_block(p, "cond_transformers.%d" % b, x, edge_index, e, emb, cfg["num_heads"], not last, None if last else act)
    return x


# ---- cases -------------------------------------------------------------------------------------------------------------------
# name -> (kind, constructor keywords (activation_layer by name), description of the inputs, seed)
CASES = {
    "gencast_encoder": ("encoder", dict(grid_dim=7, mesh_dim=3, edge_dim=4, hidden_dims=[40, 24], activation_layer="SiLU",
                                        scale_factor=0.5), dict(n_grid=50, n_mesh=12, n_edges=90), 21),
    "gencast_decoder": ("decoder", dict(edges_dim=4, output_dim=5, hidden_dims=[40, 24]), dict(n_grid=50, n_mesh=12, n_edges=120), 22),
    "gencast_processor_edges": ("processor", dict(latent_dim=32, hidden_dims=[40, 24], num_blocks=3, num_heads=4, num_frequencies=8,
                                                  base_period=16, noise_emb_dim=12, edges_dim=4), dict(n_nodes=37, copies=2), 23),
    "gencast_processor_plain": ("processor", dict(latent_dim=32, hidden_dims=[40, 24], num_blocks=3, num_heads=4, num_frequencies=8,
                                                  base_period=16, noise_emb_dim=12, edges_dim=None), dict(n_nodes=37, copies=2), 24),
    "gencast_mlp": ("mlp", dict(input_dim=6, hidden_dims=[10, 7], activation_layer="SiLU", use_layer_norm=False, activate_final=True),
                    dict(rows=13), 25),
    "gencast_fourier": ("fourier", dict(output_dim=12, num_frequencies=8, base_period=16), dict(rows=9), 26),
}
CLASS_OF = {"encoder": "Encoder", "decoder": "Decoder", "processor": "Processor", "mlp": "MLP", "fourier": "FourierEmbedding"}


def meta_of(name):
    """The integers that pin a case: every integer of its configuration and of its input description, in order."""
    _, cfg, spec, _ = CASES[name]
    out = []
    for d in (cfg, spec):
        for v in d.values():
            for x in (v if isinstance(v, (tuple, list)) else (v,)):
                if isinstance(x, (bool, int)):
                    out.append(int(x))
    return out


def random_graph(rs, n: int, max_in: int = 9):
    """Shuffled COO [2, E] on n nodes: the in-degrees cycle through 0 .. max_in, sources drawn with replacement."""
    deg = np.arange(n) % (max_in + 1)
    dst = np.repeat(np.arange(n), deg)
    src = rs.randint(0, n, dst.size)
    order = rs.permutation(dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64)


def _f32(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def case_inputs(name: str) -> Dict[str, torch.Tensor]:
    kind, cfg, spec, seed = CASES[name]
    rs = np.random.RandomState(seed)
    if kind in ("encoder", "decoder"):
        G, M, E = spec["n_grid"], spec["n_mesh"], spec["n_edges"]
        grid_ix, mesh_ix = rs.randint(0, G, E), rs.randint(0, M, E)
        if kind == "encoder":
            return dict(grid=_f32(rs, G, cfg["grid_dim"]), mesh=_f32(rs, M, cfg["mesh_dim"]), edge_attr=_f32(rs, E, cfg["edge_dim"]),
                        edge_index=torch.from_numpy(np.stack([grid_ix, mesh_ix]).astype(np.int64)))
        d = cfg["hidden_dims"][-1]
        return dict(mesh=_f32(rs, M, d), grid=_f32(rs, G, d), edge_attr=_f32(rs, E, cfg["edges_dim"]),
                    edge_index=torch.from_numpy(np.stack([mesh_ix, grid_ix]).astype(np.int64)))
    if kind == "processor":
        n, copies = spec["n_nodes"], spec["copies"]
        one = random_graph(rs, n)
        ei = np.concatenate([one + c * n for c in range(copies)], axis=1)
        noise = np.repeat(rs.uniform(-2.0, 2.0, copies), n).astype(np.float32)[:, None]
        out = dict(x=_f32(rs, copies * n, cfg["latent_dim"]), edge_index=torch.from_numpy(ei), noise_levels=torch.from_numpy(noise))
        if cfg["edges_dim"] is not None:
            out["edge_attr"] = _f32(rs, ei.shape[1], cfg["edges_dim"])
        return out
    if kind == "mlp":
        return dict(x=_f32(rs, spec["rows"], cfg["input_dim"]))
    return dict(t=torch.from_numpy(rs.uniform(-2.0, 2.0, (spec["rows"], 1)).astype(np.float32)))


def build_kind(pkg, kind: str, cfg, seed: int):
    """The module of ``pkg`` (anything with the five class names) with the seeded parameters."""
    kw = dict(cfg)
    if "activation_layer" in kw:
        kw["activation_layer"] = ACTS[kw["activation_layer"]]
    return fill_(getattr(pkg, CLASS_OF[kind])(**kw), seed)


def build(pkg, name: str):
    kind, cfg, _, seed = CASES[name]
    return build_kind(pkg, kind, cfg, seed)


def call_kind(module, kind: str, inp):
    """Run a module (the reference's or ours) on a case's inputs -> tuple of outputs."""
    if kind == "encoder":
        return tuple(module(inp["grid"], inp["mesh"], inp["edge_attr"], inp["edge_index"]))
    if kind == "decoder":
        return (module(inp["mesh"], inp["grid"], inp["edge_attr"], inp["edge_index"]),)
    if kind == "processor":
        return (module(inp["x"], inp["edge_index"], inp["noise_levels"], inp.get("edge_attr")),)
    return (module(inp["x"] if kind == "mlp" else inp["t"]),)


def call(module, name: str, inp):
    return call_kind(module, CASES[name][0], inp)


def run_kind(kind: str, cfg, p, inp):
    """The restatement on a case's inputs (already of p's dtype) -> tuple of outputs."""
    if kind == "encoder":
        return tuple(encoder(p, cfg, inp["grid"], inp["mesh"], inp["edge_attr"], inp["edge_index"]))
    if kind == "decoder":
        return (decoder(p, cfg, inp["mesh"], inp["grid"], inp["edge_attr"], inp["edge_index"]),)
    if kind == "processor":
        return (processor(p, cfg, inp["x"], inp["edge_index"], inp["noise_levels"], inp.get("edge_attr")),)
    if kind == "mlp":
        q = {"m." + k: v for k, v in p.items()}
        return (mlp(q, "m", inp["x"], cfg.get("activation_layer", "ReLU"), cfg.get("activate_final", False)),)
    q = {"f." + k: v for k, v in p.items()}
    return (fourier_embedding(q, "f", inp["t"], cfg["num_frequencies"], cfg["base_period"]),)


def run(name: str, p, inp):
    kind, cfg, _, _ = CASES[name]
    return run_kind(kind, cfg, p, inp)


def cast(inp, dtype, requires_grad: bool = False):
    return {k: (v if v.dtype == torch.int64 else v.to(dtype).clone().requires_grad_(requires_grad)) for k, v in inp.items()}
