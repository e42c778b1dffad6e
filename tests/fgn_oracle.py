"""What the FGN tests measure against: the case table of scripts/gen_fgn_golden.py and a restatement of
``FunctionalGenerativeNetwork.forward`` (graph_weather/models/fgn of the reference) over a ``state_dict`` as plain torch on the CPU
- float64 for the oracle, float32 for the yardstick - built on tests/gencast_oracle.py.  Nothing here touches the HIP kernels or
graph_weather_amd.

The restatement follows the reference member by member and sample by sample (its batch is disconnected copies of one graph) and
returns ALL members at every batch size, [B, N, lon, lat, out]; the reference's own ``forward`` keeps member 0 only at B = 1
(``len(prediction)`` is the batch size), which case c records.
"""
from __future__ import annotations

import numpy as np
import torch

from . import gencast_model_oracle as mo
from . import gencast_oracle as go

# name -> (grid of gencast_model_oracle, constructor keywords without the grid, batch, members, seed)
CASES = {
    "fgn_model_a": ("gencast_model_a", dict(input_features_dim=4, output_features_dim=6, noise_dimension=8, hidden_dims=[16, 16],
                                            num_blocks=2, num_heads=4, splits=1, num_hops=2), 2, 2, 41),
    "fgn_model_b": ("gencast_model_b", dict(input_features_dim=3, output_features_dim=5, noise_dimension=6, hidden_dims=[24, 20],
                                            num_blocks=3, num_heads=4, splits=2, num_hops=3, use_edges_features=False, scale_factor=0.5),
                    3, 3, 42),
    "fgn_model_c": ("gencast_model_a", dict(input_features_dim=4, output_features_dim=6, noise_dimension=8, hidden_dims=[16, 16],
                                            num_blocks=1, num_heads=4, splits=1, num_hops=2), 1, 2, 43),
}
TORCH_SEED = 1000  # + the case's seed: what torch.manual_seed gets before the reference's forward draws its noise vectors


def case_kwargs(name: str) -> dict:
    lon, lat = mo.GRIDS[CASES[name][0]]()
    return dict(grid_lon=lon, grid_lat=lat, **CASES[name][1])


def case_input(name: str, batch: int = None) -> torch.Tensor:
    """previous_weather_state [B, lon, lat, in] float32 from the case's seed."""
    grid, kw, b0, _, seed = CASES[name]
    lon, lat = mo.GRIDS[grid]()
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((b0 if batch is None else batch, len(lon), len(lat), kw["input_features_dim"])).astype(np.float32))


def draw_noise(seed: int, batch: int, members: int, noise_dimension: int) -> torch.Tensor:
    """[B, N, noise] as the reference draws on the CPU after ``torch.manual_seed(seed)``: one (B, noise) draw per member."""
    torch.manual_seed(seed)
    return torch.stack([torch.randn((batch, noise_dimension)) for _ in range(members)], dim=1)


def fgn_processor(p, cfg, x, edge_index, noise_vector, edge_attr=None):
    """fgn/layers/processor.py: the GenCast blocks with the noise vector itself as the conditioning."""
    act = cfg.get("activation_layer", "ReLU")
    e = go.mlp(p, "edges_mlp", edge_attr, act) if cfg.get("edges_dim") is not None else None
    nb = cfg["num_blocks"]
    for b in range(nb):
        last = b == nb - 1
        x = go.cond_transformer_block(p, "cond_transformers.%d" % b, x, edge_index, e, noise_vector, cfg["num_heads"], not last,
                                      None if last else act)
    return x


def fgn_forward(p, kw, graphs, previous_weather_state, noise_vectors):
    """The forward on tensors of p's dtype: ``kw`` the constructor keywords, ``graphs`` the 14 buffers (float tables already of p's
    dtype), ``noise_vectors`` [B, N, noise] -> [B, N, lon, lat, out]."""
    B, N = noise_vectors.shape[0], noise_vectors.shape[1]
    use_e = kw.get("use_edges_features", True)
    enc_cfg = dict(activation_layer="SiLU", scale_factor=kw.get("scale_factor", 1.0))
    proc_cfg = dict(activation_layer="SiLU", num_blocks=kw.get("num_blocks", 24), num_heads=kw.get("num_heads", 4),
                    edges_dim=(graphs["mesh_edge_attr"].shape[1] if use_e else None))
    x = previous_weather_state.reshape(B, -1, previous_weather_state.shape[-1])  # "b lon lat f -> b (lon lat) f"
    pe, pp, pd = mo._sub(p, "encoder."), mo._sub(p, "processor."), mo._sub(p, "decoder.")
    members = []
    for n in range(N):
        outs = []
        for b in range(B):
            grid_in = torch.cat([x[b], graphs["g2m_grid_nodes"]], dim=-1)
            lat_grid, lat_mesh = go.encoder(pe, enc_cfg, grid_in, graphs["g2m_mesh_nodes"], graphs["g2m_edge_attr"], graphs["g2m_edge_index"])
            noise = noise_vectors[b, n][None].expand(lat_mesh.shape[0], -1)
            lat_mesh = fgn_processor(pp, proc_cfg, lat_mesh, graphs["khop_mesh_edge_index"], noise,
                                     graphs["khop_mesh_edge_attr"] if use_e else None)
            outs.append(go.decoder(pd, dict(activation_layer="SiLU"), lat_mesh, lat_grid, graphs["m2g_edge_attr"], graphs["m2g_edge_index"]))
        members.append(torch.stack(outs))
    out = torch.stack(members, dim=1)
    return out.reshape(B, N, *previous_weather_state.shape[1:3], out.shape[-1])
