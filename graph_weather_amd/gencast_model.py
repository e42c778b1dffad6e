"""GenCast's ``Denoiser`` (graph_weather/models/gencast/denoiser.py of the reference) with its ``Preconditioner``, config class
and batching utilities (utils/noise.py, utils/batching.py).

Same constructor arguments, defaults, attribute names, ``state_dict`` keys and order, the 14 non-persistent graph buffers and the
reference's error messages.  The graphs come from ``gencast_graphs.GraphBuilder`` (numpy and scipy).

The reference batches by replicating the graph (``hetero_batch`` / ``batch``: B disconnected copies, ``edge_index`` and
``edge_attr`` concatenated B times, the noise level repeated for every node).  ``Denoiser.forward`` here does not: it runs the
batch-shared form of the layers (``gencast.Encoder._forward_shared`` and its siblings) on ONE graph - input assembly
(``gw_gencast_precond_input_forward``: c_in(sigma) Z | X | static grid features in one pass, with c_noise) -> Encoder -> Processor
-> Decoder -> output combine - and gives the reference's result.  ``batch`` and ``hetero_batch`` stay available, and
``_forward_replicated`` runs the reference's route through them and the layers' public ``forward``s for comparison.

``generate_isotropic_noise`` draws on the device (inverse spherical-harmonic transform of csrc/gw_sht.hip); the ``Sampler`` and
``WeightedMSELoss`` live in ``gencast_sampler``.

Not reproduced: the reference's ``assert not torch.isnan(...)`` after every stage - each one is a host synchronisation.  The
"strictly positive" check reads the device too; it is kept (with the reference's ``.any()``) but skipped while the current stream
is capturing, so the eval forward can be captured in a ``torch.cuda.graph``.  fp32 only.  ``sparse="native"`` (with
``use_edges_features=False``) runs the processor on ``gencast_sparse.SparseTransformer`` blocks; ``sparse=True`` asks for the
reference's DGL backend and raises as the reference does without DGL.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .gencast import Decoder, Encoder, Processor, _PrecondInput, _PrecondOutput
from .gencast_graphs import GraphBuilder

try:  # the hub mixin gives save_pretrained / from_pretrained / push_to_hub
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover
    class PyTorchModelHubMixin:  # type: ignore
        pass

__all__ = ["batch", "hetero_batch", "Preconditioner", "sample_noise_level", "generate_isotropic_noise", "DenoiserConfig", "Denoiser"]


# ---------------------------------------------------------------------------------------------------------------------
# utils/batching.py
# ---------------------------------------------------------------------------------------------------------------------
def batch(senders, edge_index, edge_attr=None, batch_size=1):
    """``batch_size`` disconnected copies of a graph: (node features [(b n), f], edge_index with copy i's indices moved by i n,
    edge_attr repeated or None)."""
    ns = senders.shape[0]
    nodes = torch.cat([senders] * batch_size, dim=0) if batch_size > 1 else senders
    index = torch.cat([edge_index + i * ns for i in range(batch_size)], dim=1) if batch_size > 1 else edge_index
    attr = edge_attr
    if edge_attr is not None and batch_size > 1:
        attr = torch.cat([edge_attr] * batch_size, dim=0)
    return nodes, index, attr


def hetero_batch(senders, receivers, edge_index, edge_attr=None, batch_size=1):
    """``batch`` for a graph whose two ends live in different tables: (senders, receivers, edge_index, edge_attr) of the big
    graph; copy i's sender indices move by i ns and its receiver indices by i nr."""
    if batch_size <= 1:
        return senders, receivers, edge_index, edge_attr
    shift = torch.tensor([[senders.shape[0]], [receivers.shape[0]]]).to(edge_index)
    attr = None if edge_attr is None else torch.cat([edge_attr] * batch_size, dim=0)
    return (torch.cat([senders] * batch_size, dim=0), torch.cat([receivers] * batch_size, dim=0),
            torch.cat([edge_index + i * shift for i in range(batch_size)], dim=1), attr)


# ---------------------------------------------------------------------------------------------------------------------
# utils/noise.py
# ---------------------------------------------------------------------------------------------------------------------
def generate_isotropic_noise(num_lon: int, num_lat: int, num_samples=1, isotropic=True, *, device=None, generator=None, batch=None,
                             coeffs=None):
    """Noise on the grid, on the device: float32 [lon, lat, num_samples], or [batch, lon, lat, num_samples] with ``batch``.

    ``isotropic=True`` is white noise on the sphere: complex64 standard normal coefficients [fields, lmax, lmax + 1] divided by
    ``sqrt(num_lat**2 // 2)``, the inverse spherical-harmonic transform (``ops.isht_forward``, csrc/gw_sht.hip: what the reference
    gets from ``torch_harmonics.InverseRealSHT``) and a factor ``sqrt(2 pi)``; the grid must be 2N x N or 2N x (N + 1).
    ``coeffs`` supplies the unscaled complex draws instead of ``torch.randn(..., generator=generator)``.  ``isotropic=False`` is
    ``torch.randn`` of the output shape.

    The reference returns a numpy array from the host; this package has no CPU path, so without ``device`` the function raises."""
    if device is None:
        raise NotImplementedError("graph_weather_amd: generate_isotropic_noise on the host needs torch_harmonics (the inverse spherical "
                                  "harmonic transform), which this package does not provide; pass device= to draw on a HIP device")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("graph_weather_amd: generate_isotropic_noise draws on a HIP device (no CPU path exists), got %s" % device)
    if isotropic:
        if 2 * num_lat == num_lon:
            extend = False
        elif 2 * (num_lat - 1) == num_lon:
            extend = True
        else:
            raise ValueError(
                "Isotropic noise requires grid's shape to be 2N x N or 2N x (N+1): "
                f"got {num_lon} x {num_lat}. If the shape is correct, please specify"
                "isotropic=False in the constructor.",
            )
    lead = () if batch is None else (int(batch),)
    if not isotropic:
        return torch.randn(*lead, num_lon, num_lat, num_samples, dtype=torch.float32, device=device, generator=generator)
    from . import ops

    fields = (1 if batch is None else int(batch)) * num_samples
    lmax = num_lat - 1 if extend else num_lat
    mmax = lmax + 1
    if coeffs is None:
        coeffs = torch.randn(fields, lmax, mmax, dtype=torch.complex64, device=device, generator=generator)
    elif tuple(coeffs.shape) != (fields, lmax, mmax):
        raise ValueError(f"coeffs must be complex64 of shape {(fields, lmax, mmax)}, got {tuple(coeffs.shape)}")
    coeffs = coeffs / np.sqrt((num_lat**2) // 2)
    noise = ops.isht_forward(coeffs.contiguous(), num_lat, num_lon, num_samples, float(np.sqrt(2 * np.pi)))
    return noise if batch is not None else noise[0]


def sample_noise_level(sigma_min=0.02, sigma_max=88, rho=7):
    """One noise level from the training distribution of the paper."""
    u = np.random.random()
    return (sigma_max ** (1 / rho) + u * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho


class Preconditioner(torch.nn.Module):
    """The preconditioning functions of Karras et al. (2022), table 1, as plain torch expressions (any device).  The Denoiser's
    forward forms the same coefficients inside its two preconditioning kernels."""

    def __init__(self, sigma_data: float = 1):
        super().__init__()
        self.sigma_data = sigma_data

    def c_skip(self, sigma):
        return self.sigma_data**2 / (sigma**2 + self.sigma_data**2)

    def c_out(self, sigma):
        return sigma * self.sigma_data / torch.sqrt(sigma**2 + self.sigma_data**2)

    def c_in(self, sigma):
        return 1 / torch.sqrt(sigma**2 + self.sigma_data**2)

    def c_noise(self, sigma):
        return 1 / 4 * torch.log(sigma)


# ---------------------------------------------------------------------------------------------------------------------
# denoiser.py
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class DenoiserConfig:
    """Configuration for Denoiser model."""

    grid_lon: np.ndarray
    grid_lat: np.ndarray
    input_features_dim: int
    output_features_dim: int
    hidden_dims: list = None
    num_blocks: int = 16
    num_heads: int = 4
    splits: int = 6
    num_hops: int = 6
    device: torch.device = torch.device("cpu")
    sparse: object = False  # False, True (the reference's DGL backend: raises) or "native"
    use_edges_features: bool = True
    scale_factor: float = 1.0

    def __post_init__(self):
        if self.hidden_dims is None:
            self.hidden_dims = [512, 512]

    def build(self) -> "Denoiser":
        return Denoiser(grid_lon=self.grid_lon, grid_lat=self.grid_lat, input_features_dim=self.input_features_dim,
                        output_features_dim=self.output_features_dim, hidden_dims=self.hidden_dims, num_blocks=self.num_blocks,
                        num_heads=self.num_heads, splits=self.splits, num_hops=self.num_hops, device=self.device, sparse=self.sparse,
                        use_edges_features=self.use_edges_features, scale_factor=self.scale_factor)


_GRAPH_BUFFERS = ("g2m_grid_nodes", "g2m_mesh_nodes", "g2m_edge_attr", "g2m_edge_index", "mesh_nodes", "mesh_edge_attr",
                  "mesh_edge_index", "khop_mesh_nodes", "khop_mesh_edge_attr", "khop_mesh_edge_index", "m2g_grid_nodes", "m2g_mesh_nodes",
                  "m2g_edge_attr", "m2g_edge_index")


class Denoiser(torch.nn.Module, PyTorchModelHubMixin):
    """GenCast's Denoiser: D(Z, X, sigma) = c_skip(sigma) Z + c_out(sigma) f_theta(c_in(sigma) Z, X, c_noise(sigma)) with f_theta
    the (encoder, processor, decoder) model over the grid-to-mesh, k-hop mesh and mesh-to-grid graphs."""

    def __init__(self, grid_lon: np.ndarray, grid_lat: np.ndarray, input_features_dim: int, output_features_dim: int,
                 hidden_dims: list[int] = [512, 512], num_blocks: int = 16, num_heads: int = 4, splits: int = 6, num_hops: int = 6,
                 device: torch.device = torch.device("cpu"), sparse=False, use_edges_features: bool = True,
                 scale_factor: float = 1.0):
        super().__init__()
        self.num_lon = len(grid_lon)
        self.num_lat = len(grid_lat)
        self.input_features_dim = input_features_dim
        self.output_features_dim = output_features_dim
        self.use_edges_features = use_edges_features

        self.graphs = GraphBuilder(grid_lon=grid_lon, grid_lat=grid_lat, splits=splits, num_hops=num_hops, device=device,
                                   add_edge_features_to_khop=use_edges_features)
        self._register_graph()

        self.encoder = Encoder(grid_dim=output_features_dim + 2 * input_features_dim + self.graphs.grid_nodes_dim,
                               mesh_dim=self.graphs.mesh_nodes_dim, edge_dim=self.graphs.g2m_edges_dim, hidden_dims=hidden_dims,
                               activation_layer=torch.nn.SiLU, use_layer_norm=True, scale_factor=scale_factor)
        if sparse and use_edges_features:
            raise ValueError("Sparse processor don't support edges features.")
        self.processor = Processor(latent_dim=hidden_dims[-1], edges_dim=self.graphs.mesh_edges_dim if use_edges_features else None,
                                   hidden_dims=hidden_dims, num_blocks=num_blocks, num_heads=num_heads, num_frequencies=32,
                                   base_period=16, noise_emb_dim=16, activation_layer=torch.nn.SiLU, use_layer_norm=True, sparse=sparse)
        self.decoder = Decoder(edges_dim=self.graphs.m2g_edges_dim, output_dim=output_features_dim, hidden_dims=hidden_dims,
                               activation_layer=torch.nn.SiLU, use_layer_norm=True)
        self.precs = Preconditioner(sigma_data=1.0)

    def _check_shapes(self, corrupted_targets, prev_inputs, noise_levels):
        batch_size = prev_inputs.shape[0]
        exp_inputs_shape = (batch_size, self.num_lon, self.num_lat, 2 * self.input_features_dim)
        exp_targets_shape = (batch_size, self.num_lon, self.num_lat, self.output_features_dim)
        exp_noise_shape = (batch_size, 1)
        if not all([corrupted_targets.shape == exp_targets_shape, prev_inputs.shape == exp_inputs_shape,
                    noise_levels.shape == exp_noise_shape]):
            raise ValueError(
                "The shapes of the input tensors don't match with the initialization parameters: "
                f"expected {exp_inputs_shape} for prev_inputs, {exp_targets_shape} for targets and "
                f"{exp_noise_shape} for noise_levels."
            )

    def _check_noise(self, noise_levels):
        if noise_levels.is_cuda and torch.cuda.is_current_stream_capturing():
            return  # (the check reads the device)
        if not (noise_levels > 0).any():
            raise ValueError("All the noise levels must be strictly positive.")

    def forward(self, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor, noise_levels: torch.Tensor) -> torch.Tensor:
        """corrupted_targets [B, lon, lat, out], prev_inputs [B, lon, lat, 2 in] (the previous two timesteps side by side),
        noise_levels [B, 1] -> [B, lon, lat, out].  The two leading grid axes are flattened "b lon lat f -> b (lon lat) f" and
        paired row by row with the builder's latitude-major grid nodes, as the reference pairs them."""
        self._check_shapes(corrupted_targets, prev_inputs, noise_levels)
        self._check_noise(noise_levels)
        return self._forward_impl(corrupted_targets, prev_inputs, noise_levels)

    def _forward_impl(self, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor, noise_levels: torch.Tensor) -> torch.Tensor:
        """``forward`` without its checks (the positivity check reads the device): for callers such as ``Sampler`` whose shapes
        are checked once and whose noise levels are known positive on the host."""
        B, sd = int(prev_inputs.shape[0]), float(self.precs.sigma_data)
        z = corrupted_targets.reshape(-1, self.output_features_dim)
        x = prev_inputs.reshape(-1, 2 * self.input_features_dim)
        grid_in, c_noise = _PrecondInput.apply(z, x, noise_levels, self.g2m_grid_nodes, sd)
        latent_grid, latent_mesh = self.encoder._forward_shared(grid_in, self.g2m_mesh_nodes, self.g2m_edge_attr, self.g2m_edge_index, B)
        latent_mesh = self.processor._forward_shared(latent_mesh, self.khop_mesh_edge_index, c_noise,
                                                     self.khop_mesh_edge_attr if self.use_edges_features else None, B)
        preds = self.decoder._forward_shared(latent_mesh, latent_grid, self.m2g_edge_attr, self.m2g_edge_index, B)
        out = _PrecondOutput.apply(z, preds, noise_levels, sd)
        return out.reshape(B, self.num_lon, self.num_lat, self.output_features_dim)

    def _register_graph(self):
        g2m, m2g = self.graphs.g2m_graph, self.graphs.m2g_graph
        tables = dict(
            g2m_grid_nodes=g2m["grid_nodes"].x, g2m_mesh_nodes=g2m["mesh_nodes"].x,
            g2m_edge_attr=g2m["grid_nodes", "to", "mesh_nodes"].edge_attr, g2m_edge_index=g2m["grid_nodes", "to", "mesh_nodes"].edge_index,
            mesh_nodes=self.graphs.mesh_graph.x, mesh_edge_attr=self.graphs.mesh_graph.edge_attr,
            mesh_edge_index=self.graphs.mesh_graph.edge_index, khop_mesh_nodes=self.graphs.khop_mesh_graph.x,
            khop_mesh_edge_attr=self.graphs.khop_mesh_graph.edge_attr, khop_mesh_edge_index=self.graphs.khop_mesh_graph.edge_index,
            m2g_grid_nodes=m2g["grid_nodes"].x, m2g_mesh_nodes=m2g["mesh_nodes"].x,
            m2g_edge_attr=m2g["mesh_nodes", "to", "grid_nodes"].edge_attr, m2g_edge_index=m2g["mesh_nodes", "to", "grid_nodes"].edge_index)
        for name in _GRAPH_BUFFERS:  # (not part of the state: they move with the model and are rebuilt from the grid)
            self.register_buffer(name, tables[name], persistent=False)


def _forward_replicated(model: Denoiser, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor,
                       noise_levels: torch.Tensor) -> torch.Tensor:
    """``model``'s forward by the reference's route: the graph replicated with ``hetero_batch`` / ``batch``, the static features
    concatenated, the noise level repeated for every mesh node, the layers' public ``forward``s, the preconditioning as torch
    expressions.  For comparison and measurement; ``Denoiser.forward`` is the batch-shared route."""
    model._check_shapes(corrupted_targets, prev_inputs, noise_levels)
    B = prev_inputs.shape[0]
    z = corrupted_targets.reshape(B, -1, model.output_features_dim)
    x = prev_inputs.reshape(B, -1, 2 * model.input_features_dim)
    feats = torch.cat((model.precs.c_in(noise_levels)[:, :, None] * z, x), dim=-1)
    senders, receivers, index, attr = hetero_batch(model.g2m_grid_nodes, model.g2m_mesh_nodes, model.g2m_edge_index, model.g2m_edge_attr, B)
    latent_grid, latent_mesh = model.encoder(input_grid_nodes=torch.cat([feats.reshape(-1, feats.shape[-1]), senders], dim=-1),
                                             input_mesh_nodes=receivers, input_edge_attr=attr, edge_index=index)
    num_nodes = latent_mesh.shape[0] // B
    _, index, attr = batch(model.khop_mesh_nodes, model.khop_mesh_edge_index,
                           model.khop_mesh_edge_attr if model.use_edges_features else None, B)
    noise = model.precs.c_noise(noise_levels).repeat_interleave(num_nodes, dim=0)
    latent_mesh = model.processor(latent_mesh_nodes=latent_mesh, input_edge_attr=attr, edge_index=index, noise_levels=noise)
    _, _, index, attr = hetero_batch(model.m2g_mesh_nodes, model.m2g_grid_nodes, model.m2g_edge_index, model.m2g_edge_attr, B)
    preds = model.decoder(input_mesh_nodes=latent_mesh, input_grid_nodes=latent_grid, input_edge_attr=attr, edge_index=index)
    out = model.precs.c_skip(noise_levels)[:, :, None] * z + model.precs.c_out(noise_levels)[:, :, None] * preds.reshape(B, -1, z.shape[-1])
    return out.reshape(corrupted_targets.shape)
