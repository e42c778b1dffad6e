"""GenDA (graph_weather/models/genda/model.py of the reference): the GenCast ``Denoiser`` with two extra grid channels - a sensor
mask and sensor values - and classifier-free guidance, ``guided_forward`` = uncond + gamma (cond - uncond).

Same constructor arguments, defaults, attribute names, ``state_dict`` keys and order, the 14 non-persistent graph buffers and the
reference's error messages.  The layers are those of ``gencast``; the graphs come from ``gencast_graphs.GraphBuilder``.

``forward`` is the Denoiser's batch-shared route on ONE graph with the input assembly of csrc/gw_genda.hip
(``gw_genda_input_forward``: c_in(sigma) Z | X | mask | values | static grid features in one pass, with c_noise).

``guided_forward`` is where this file differs from the reference.  There the model runs twice on the same Z, X and sigma, the
second time with ``zeros_like`` conditioning, and three torch expressions combine the outputs.  Here it is ONE pass at batch 2 B:
the input kernel writes copy k = 0 (conditional) to the rows of sample b and copy k = 1 (zero conditioning) to those of sample
B + b from one read of its inputs, the layers' batch-shared forms run over 2 B samples of one graph, and
``gw_genda_guided_output_forward`` folds the output preconditioning of both halves and the combine.  Every row of the layers is
computed from its own sample alone, so the result is that of the two-pass composition up to the rounding order of the kernels.

``GenDA.guided(mask, values, gamma)`` is a view with the Denoiser's calling convention (``_check_shapes`` and ``_forward_impl`` of
three arguments) whose forward is the guided pass: the unchanged ``Sampler.sample`` then produces a sensor-guided analysis.

Deviations, on purpose:
  * when the number of conditioning tensors supplied differs from ``conditioning_dim`` a ``ValueError`` of this package is raised
    after the reference's own checks; the reference fails inside the encoder's first matmul with a shape error.
  * the training-time conditioning dropout is the reference's host draw (``torch.rand(1).item() < 0.1``, one per ``forward``, two
    per ``guided_forward``), but a hit is a flag of the input kernel: the conditioning columns are written as zeros, no
    ``zeros_like`` temporaries are made, and mask and values receive zero gradients.
  * the reference's ``assert not torch.isnan(...)`` after every stage are host synchronisations and are not reproduced; the
    "strictly positive" check is kept (with the reference's ``.any()``) and skipped while the stream is capturing.
  * ``wind_direction`` is accepted and ignored, as in the reference.  fp32 only; ``sparse="native"`` (with
    ``use_edges_features=False``) runs the processor on ``gencast_sparse.SparseTransformer`` blocks, ``sparse=True`` raises as the
    reference does without DGL.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from .gencast import Decoder, Encoder, Processor, _PrecondOutput, _sigma_rows
from .gencast_graphs import GraphBuilder
from .gencast_model import Denoiser, Preconditioner, PyTorchModelHubMixin, batch, hetero_batch
from .ops import on_device_of
from .wide import _L, _ld, _rows, _st

__all__ = ["GenDA", "GenDAConfig", "genda_input_forward", "genda_input_backward", "guided_output_forward", "guided_output_backward"]


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers (include/gw_amd.h: gw_genda_*)
# ---------------------------------------------------------------------------------------------------------------------
def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _column(t: Optional[torch.Tensor], rows: int, name: str):
    if t is None:
        return None
    t = _rows(t, name)
    if tuple(t.shape) != (rows, 1):
        raise RuntimeError("graph_weather_amd: %s must be one column of %d rows, got %s" % (name, rows, tuple(t.shape)))
    return t


def genda_input_forward(z: torch.Tensor, x: torch.Tensor, sigma: torch.Tensor, static: torch.Tensor, c0: Optional[torch.Tensor] = None,
                        c1: Optional[torch.Tensor] = None, copies: int = 1, drop: bool = False, sigma_data: float = 1.0):
    """The encoder's grid input rows of ``copies`` evaluations and the scaled noise levels: z [B G, wz], x [B G, wx], static
    [G, ws], c0, c1 [B G, 1] or None (views with a row stride are read in place), sigma [B] or [B, 1] ->
    ([copies B G, wz + wx + n_cond + ws], c_noise [copies B, 1]).  Row b G + g is (c_in(sigma_b) z | x | c0 | c1 | static[g]); with
    ``copies=2`` row (B + b) G + g is the same with zero conditioning.  ``drop`` writes zeros for the conditioning of copy 0 too."""
    z, x, static = _rows(z, "corrupted targets"), _rows(x, "previous inputs"), _rows(static, "static grid features")
    sigma, batch_size, G = _sigma_rows(sigma, int(z.shape[0]), "the GenDA input assembly")
    if int(x.shape[0]) != batch_size * G or int(static.shape[0]) != G:
        raise RuntimeError("graph_weather_amd: the GenDA input assembly expects %d rows of previous inputs and %d static rows, got %d "
                           "and %d" % (batch_size * G, G, int(x.shape[0]), int(static.shape[0])))
    if copies not in (1, 2):
        raise ValueError("graph_weather_amd: the GenDA input assembly writes 1 or 2 copies, got %r" % (copies,))
    c0, c1 = _column(c0, batch_size * G, "sensor_mask"), _column(c1, batch_size * G, "sensor_values")
    wz, wx, ws, nc = int(z.shape[1]), int(x.shape[1]), int(static.shape[1]), (c0 is not None) + (c1 is not None)
    width = wz + wx + nc + ws
    out = torch.empty((copies * batch_size * G, width), dtype=torch.float32, device=z.device)
    c_noise = torch.empty((copies * batch_size, 1), dtype=torch.float32, device=z.device)
    with on_device_of(out):
        _lib.check(_L().gw_genda_input_forward(batch_size, G, copies, 1 if drop else 0, wz, wx, ws, float(sigma_data), sigma.data_ptr(),
                                               z.data_ptr(), _ld(z), x.data_ptr(), _ld(x), _p(c0), 0 if c0 is None else _ld(c0), _p(c1),
                                               0 if c1 is None else _ld(c1), static.data_ptr(), _ld(static), out.data_ptr(), width,
                                               c_noise.data_ptr(), _st(out)), "gw_genda_input_forward")
    return out, c_noise


def genda_input_backward(dout: torch.Tensor, sigma: torch.Tensor, wz: int, wx: int, n_cond: int, copies: int = 1, drop: bool = False,
                         sigma_data: float = 1.0, want=(True, True, True, True)):
    """(dz, dx, d of conditioning column 0, d of column 1) of ``genda_input_forward``; an entry is None where ``want`` is False or
    the column does not exist."""
    dout = _rows(dout, "dout")
    sigma, batch_size, G = _sigma_rows(sigma, int(dout.shape[0]) // copies, "the GenDA input assembly")
    rows = batch_size * G
    if int(dout.shape[0]) != copies * rows:
        raise RuntimeError("graph_weather_amd: the GenDA input assembly's gradient expects %d rows, got %d" % (copies * rows, int(dout.shape[0])))
    widths = (wz, wx, 1 if n_cond >= 1 else 0, 1 if n_cond >= 2 else 0)
    outs = [torch.empty((rows, w), dtype=torch.float32, device=dout.device) if (k and (w or i < 2)) else None
            for i, (k, w) in enumerate(zip(want, widths))]
    if all(o is None or o.numel() == 0 for o in outs):  # nothing to compute
        return tuple(outs)
    dz, dx, dc0, dc1 = outs
    with on_device_of(dout):
        _lib.check(_L().gw_genda_input_backward(batch_size, G, copies, 1 if drop else 0, wz, wx, n_cond, float(sigma_data), sigma.data_ptr(),
                                                dout.data_ptr(), _ld(dout), _p(dz), wz, _p(dx), wx, _p(dc0), 1, _p(dc1), 1, _st(dout)),
                   "gw_genda_input_backward")
    return dz, dx, dc0, dc1


def guided_output_forward(z: torch.Tensor, preds: torch.Tensor, sigma: torch.Tensor, gamma: float, sigma_data: float = 1.0) -> torch.Tensor:
    """o_u + gamma (o_c - o_u) with o_c = c_skip z + c_out preds[b G + g] and o_u = c_skip z + c_out preds[(B + b) G + g]: z [B G, w],
    preds [2 B G, w] -> [B G, w]."""
    z, preds = _rows(z, "corrupted targets"), _rows(preds, "predictions")
    sigma, batch_size, G = _sigma_rows(sigma, int(z.shape[0]), "the guided output combine")
    if tuple(preds.shape) != (2 * int(z.shape[0]), int(z.shape[1])):
        raise RuntimeError("graph_weather_amd: the guided output combine expects predictions %s for targets %s, got %s"
                           % ((2 * int(z.shape[0]), int(z.shape[1])), tuple(z.shape), tuple(preds.shape)))
    width = int(z.shape[1])
    out = torch.empty((batch_size * G, width), dtype=torch.float32, device=z.device)
    with on_device_of(out):
        _lib.check(_L().gw_genda_guided_output_forward(batch_size, G, width, float(sigma_data), float(gamma), sigma.data_ptr(), z.data_ptr(),
                                                       _ld(z), preds.data_ptr(), _ld(preds), out.data_ptr(), width, _st(out)),
                   "gw_genda_guided_output_forward")
    return out


def guided_output_backward(dout: torch.Tensor, sigma: torch.Tensor, gamma: float, sigma_data: float = 1.0):
    """(dz [B G, w], dpreds [2 B G, w]) of ``guided_output_forward``."""
    dout = _rows(dout, "dout")
    sigma, batch_size, G = _sigma_rows(sigma, int(dout.shape[0]), "the guided output combine")
    width = int(dout.shape[1])
    dz = torch.empty((batch_size * G, width), dtype=torch.float32, device=dout.device)
    dp = torch.empty((2 * batch_size * G, width), dtype=torch.float32, device=dout.device)
    with on_device_of(dz):
        _lib.check(_L().gw_genda_guided_output_backward(batch_size, G, width, float(sigma_data), float(gamma), sigma.data_ptr(),
                                                        dout.data_ptr(), _ld(dout), dz.data_ptr(), width, dp.data_ptr(), width, _st(dz)),
                   "gw_genda_guided_output_backward")
    return dz, dp


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
class _GendaInput(Function):
    @staticmethod
    def forward(ctx, z, x, sigma, static, c0, c1, copies: int, drop: bool, sigma_data: float):
        out, c_noise = genda_input_forward(z, x, sigma, static, c0, c1, copies, drop, sigma_data)
        ctx.meta = (int(z.shape[1]), int(x.shape[1]), (c0 is not None) + (c1 is not None), copies, drop, sigma_data)
        ctx.have = (c0 is not None, c1 is not None)
        ctx.save_for_backward(sigma)
        ctx.mark_non_differentiable(c_noise)
        return out, c_noise

    @staticmethod
    def backward(ctx, dout, _):
        (sigma,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        # conditioning column j of the rows is the j-th tensor that was given
        slots = [i for i, h in zip((4, 5), ctx.have) if h]
        want = (need[0], need[1]) + tuple(j < len(slots) and need[slots[j]] for j in range(2))
        dz, dx, d0, d1 = genda_input_backward(dout, sigma, *ctx.meta, want=want)
        grads = [dz, dx, None, None, None, None, None, None, None]
        for j, d in enumerate((d0, d1)):
            if j < len(slots):
                grads[slots[j]] = d
        return tuple(grads)


class _GuidedOutput(Function):
    @staticmethod
    def forward(ctx, z, preds, sigma, gamma: float, sigma_data: float):
        ctx.meta = (gamma, sigma_data)
        ctx.save_for_backward(sigma)
        return guided_output_forward(z, preds, sigma, gamma, sigma_data)

    @staticmethod
    def backward(ctx, dout):
        (sigma,) = ctx.saved_tensors
        dz, dp = guided_output_backward(dout, sigma, *ctx.meta)
        return dz, dp, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# genda/model.py
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class GenDAConfig:
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

    def build(self) -> "GenDA":
        return GenDA(grid_lon=self.grid_lon, grid_lat=self.grid_lat, input_features_dim=self.input_features_dim,
                     output_features_dim=self.output_features_dim, hidden_dims=self.hidden_dims, num_blocks=self.num_blocks,
                     num_heads=self.num_heads, splits=self.splits, num_hops=self.num_hops, device=self.device, sparse=self.sparse,
                     use_edges_features=self.use_edges_features, scale_factor=self.scale_factor)


DROPOUT_P = 0.1  # the reference's conditioning dropout in training mode


class GenDA(torch.nn.Module, PyTorchModelHubMixin):
    """GenDA diffusion model with sensor conditioning: D(Z, X, sigma, mask, values) = c_skip(sigma) Z + c_out(sigma)
    f_theta(c_in(sigma) Z, X, mask, values, c_noise(sigma))."""

    def __init__(self, grid_lon: np.ndarray, grid_lat: np.ndarray, input_features_dim: int, output_features_dim: int,
                 hidden_dims: list[int] = [512, 512], num_blocks: int = 16, num_heads: int = 4, splits: int = 6, num_hops: int = 6,
                 device: torch.device = torch.device("cpu"), sparse=False, use_edges_features: bool = True,
                 scale_factor: float = 1.0, conditioning_dim: int = 2):
        super().__init__()
        self.num_lon = len(grid_lon)
        self.num_lat = len(grid_lat)
        self.input_features_dim = input_features_dim
        self.output_features_dim = output_features_dim
        self.use_edges_features = use_edges_features
        self._conditioning_dim = int(conditioning_dim)  # (the reference keeps it in the encoder's width only)

        self.graphs = GraphBuilder(grid_lon=grid_lon, grid_lat=grid_lat, splits=splits, num_hops=num_hops, device=device,
                                   add_edge_features_to_khop=use_edges_features)
        self._register_graph()

        self.encoder = Encoder(grid_dim=output_features_dim + 2 * input_features_dim + conditioning_dim + self.graphs.grid_nodes_dim,
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

    _register_graph = Denoiser._register_graph
    _check_noise = Denoiser._check_noise

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def _check_shapes(self, corrupted_targets, prev_inputs, noise_levels, sensor_mask=None, sensor_values=None):
        batch_size = prev_inputs.shape[0]
        expected_sensor_shape = (batch_size, self.num_lon, self.num_lat, 1)
        if sensor_mask is not None and sensor_mask.shape != expected_sensor_shape:
            raise ValueError(f"Expected sensor_mask shape {expected_sensor_shape}")
        if sensor_values is not None and sensor_values.shape != expected_sensor_shape:
            raise ValueError(f"Expected sensor_values shape {expected_sensor_shape}")
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

    def _check_conditioning(self, sensor_mask, sensor_values):
        given = (sensor_mask is not None) + (sensor_values is not None)
        if given != self._conditioning_dim:
            raise ValueError("graph_weather_amd: GenDA was built with conditioning_dim=%d but %d conditioning tensor(s) (sensor_mask, "
                             "sensor_values) were given" % (self._conditioning_dim, given))

    def _draw_dropout(self, sensor_mask, sensor_values) -> bool:
        """The reference's conditioning dropout: in training mode with both sensors given, one draw from the host generator."""
        return bool(self.training and sensor_mask is not None and sensor_values is not None and torch.rand(1).item() < DROPOUT_P)

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def forward(self, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor, noise_levels: torch.Tensor,
                sensor_mask: Optional[torch.Tensor] = None, sensor_values: Optional[torch.Tensor] = None,
                wind_direction: Optional[torch.Tensor] = None) -> torch.Tensor:
        """corrupted_targets [B, lon, lat, out], prev_inputs [B, lon, lat, 2 in], noise_levels [B, 1], sensor_mask and sensor_values
        [B, lon, lat, 1] -> [B, lon, lat, out].  ``wind_direction`` is ignored, as in the reference."""
        self._check_shapes(corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values)
        self._check_noise(noise_levels)
        self._check_conditioning(sensor_mask, sensor_values)
        drop = self._draw_dropout(sensor_mask, sensor_values)
        return self._forward_impl(corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values, drop)

    def _layers(self, grid_in, c_noise, B):
        latent_grid, latent_mesh = self.encoder._forward_shared(grid_in, self.g2m_mesh_nodes, self.g2m_edge_attr, self.g2m_edge_index, B)
        latent_mesh = self.processor._forward_shared(latent_mesh, self.khop_mesh_edge_index, c_noise,
                                                     self.khop_mesh_edge_attr if self.use_edges_features else None, B)
        return self.decoder._forward_shared(latent_mesh, latent_grid, self.m2g_edge_attr, self.m2g_edge_index, B)

    def _inputs(self, corrupted_targets, prev_inputs, sensor_mask, sensor_values):
        return (corrupted_targets.reshape(-1, self.output_features_dim), prev_inputs.reshape(-1, 2 * self.input_features_dim),
                None if sensor_mask is None else sensor_mask.reshape(-1, 1), None if sensor_values is None else sensor_values.reshape(-1, 1))

    def _forward_impl(self, corrupted_targets, prev_inputs, noise_levels, sensor_mask=None, sensor_values=None, drop: bool = False):
        """``forward`` without its checks and without the dropout draw (``drop`` is its outcome)."""
        B, sd = int(prev_inputs.shape[0]), float(self.precs.sigma_data)
        z, x, c0, c1 = self._inputs(corrupted_targets, prev_inputs, sensor_mask, sensor_values)
        grid_in, c_noise = _GendaInput.apply(z, x, noise_levels, self.g2m_grid_nodes, c0, c1, 1, drop, sd)
        out = _PrecondOutput.apply(z, self._layers(grid_in, c_noise, B), noise_levels, sd)
        return out.reshape(B, self.num_lon, self.num_lat, self.output_features_dim)

    # ---- guidance --------------------------------------------------------------------------------------------------------------
    def guided_forward(self, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor, noise_levels: torch.Tensor,
                       sensor_mask: torch.Tensor, sensor_values: torch.Tensor, gamma: float = 2.0) -> torch.Tensor:
        """Run conditional diffusion guidance: uncond + gamma (cond - uncond), both evaluations in one pass at batch 2 B."""
        if sensor_mask is None or sensor_values is None:
            raise ValueError("graph_weather_amd: guided_forward needs both sensor_mask and sensor_values")
        self._check_shapes(corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values)
        self._check_noise(noise_levels)
        self._check_conditioning(sensor_mask, sensor_values)
        drop = self._draw_dropout(sensor_mask, sensor_values)  # the conditional evaluation's draw
        self._draw_dropout(sensor_mask, sensor_values)  # the unconditional evaluation's: consumed, its conditioning is zero already
        return self._guided_impl(corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values, gamma, drop)

    def _guided_impl(self, corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values, gamma: float = 2.0,
                     drop: bool = False):
        """``guided_forward`` without its checks and draws.  Sample k B + b of the pass is copy k of sample b: k = 0 conditional,
        k = 1 with zero conditioning."""
        B, sd = int(prev_inputs.shape[0]), float(self.precs.sigma_data)
        z, x, c0, c1 = self._inputs(corrupted_targets, prev_inputs, sensor_mask, sensor_values)
        grid_in, c_noise = _GendaInput.apply(z, x, noise_levels, self.g2m_grid_nodes, c0, c1, 2, drop, sd)
        out = _GuidedOutput.apply(z, self._layers(grid_in, c_noise, 2 * B), noise_levels, float(gamma), sd)
        return out.reshape(B, self.num_lon, self.num_lat, self.output_features_dim)

    def guided(self, sensor_mask: torch.Tensor, sensor_values: torch.Tensor, gamma: float = 2.0) -> "_Guided":
        """A view of this model with the Denoiser's calling convention whose forward is the guided pass on the given sensors:
        ``Sampler().sample(model.guided(mask, values), prev_inputs)`` is a sensor-guided analysis."""
        return _Guided(self, sensor_mask, sensor_values, gamma)


class _Guided:
    """``GenDA.guided``: what ``Sampler.sample`` reads of a denoiser.  No conditioning dropout: sampling is inference."""

    def __init__(self, model: GenDA, sensor_mask: torch.Tensor, sensor_values: torch.Tensor, gamma: float):
        if sensor_mask is None or sensor_values is None:
            raise ValueError("graph_weather_amd: guided needs both sensor_mask and sensor_values")
        model._check_conditioning(sensor_mask, sensor_values)
        self.model, self.sensor_mask, self.sensor_values, self.gamma = model, sensor_mask, sensor_values, float(gamma)
        self.num_lon, self.num_lat, self.output_features_dim = model.num_lon, model.num_lat, model.output_features_dim

    def _check_shapes(self, corrupted_targets, prev_inputs, noise_levels):
        self.model._check_shapes(corrupted_targets, prev_inputs, noise_levels, self.sensor_mask, self.sensor_values)

    def _forward_impl(self, corrupted_targets, prev_inputs, noise_levels):
        return self.model._guided_impl(corrupted_targets, prev_inputs, noise_levels, self.sensor_mask, self.sensor_values, self.gamma)

    def __call__(self, corrupted_targets, prev_inputs, noise_levels):
        self._check_shapes(corrupted_targets, prev_inputs, noise_levels)
        self.model._check_noise(noise_levels)
        return self._forward_impl(corrupted_targets, prev_inputs, noise_levels)


def _forward_replicated(model: GenDA, corrupted_targets: torch.Tensor, prev_inputs: torch.Tensor, noise_levels: torch.Tensor,
                        sensor_mask: Optional[torch.Tensor] = None, sensor_values: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``model``'s forward by the reference's route: the graph replicated with ``hetero_batch`` / ``batch``, the conditioning and the
    static features concatenated, the noise level repeated for every mesh node, the layers' public ``forward``s, the preconditioning
    as torch expressions.  No dropout draw.  For comparison and measurement; ``GenDA.forward`` is the batch-shared route."""
    model._check_shapes(corrupted_targets, prev_inputs, noise_levels, sensor_mask, sensor_values)
    model._check_conditioning(sensor_mask, sensor_values)
    B = prev_inputs.shape[0]
    z = corrupted_targets.reshape(B, -1, model.output_features_dim)
    x = prev_inputs.reshape(B, -1, 2 * model.input_features_dim)
    cond = [c.reshape(B, -1, 1) for c in (sensor_mask, sensor_values) if c is not None]
    feats = torch.cat([model.precs.c_in(noise_levels)[:, :, None] * z, x] + cond, dim=-1)
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
