"""``PhysicalConstraintLayer`` (reference ``graph_weather/models/layers/constraint_layer.py``) on the HIP kernels of
``csrc/gw_constraint.hip``.

The reference moves the decoder output through the Python loops ``graph_to_grid`` / ``grid_to_graph`` (forecast.py:194-213)
around the constraint.  Those loops are gathers through the node -> grid-cell map ``pi(n) = row(n) * W + col(n)`` of
``node_to_grid``, with the last node of a cell winning every write.  The map is not a bijection on most regular grids (the
reference truncates ``(lat - min) / (max - min) * (H - 1)``; at 1 degree 57 800 of 64 800 cells are hit), and reproducing it
is what makes a reference-trained constrained model mean the same thing here.  With ``h = hr[pi(n)]``, ``l = lr[pi(n)]``:

    additive        out[n] = h + (l - mean_m hr[pi(m)])
    multiplicative  out[n] = h * (mean_m lr[pi(m)] / (mean_m hr[pi(m)] + 1e-8))
    softmax         out[n] = e * (l * (1 / e)),  e = exp(exp_factor * h)       (upsampling_factor f = 1)
                    out[n] = R[pi(n)],  R = E * kron(lr * (1 / (avgpool_f(E) * f^2)), ones(f, f)),  E = exp(a * y)   (f > 1)

Grid (4-D) inputs read through ``pi``; graph (3-D) inputs through ``sigma(n) = last(pi(n))``, the node whose write survives
``graph_to_grid``.  Two reference defects are left out on purpose: the layer holds its model without registering it as a
submodule (the reference's module cycle makes ``state_dict()`` recurse forever), and the output stays on the input's device
(the reference's loops allocate on the CPU).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import CONSTRAINT_TYPES, GwConstraintArgs
from .ops import _stream, on_device_of

TYPES = tuple(CONSTRAINT_TYPES)


def grid_maps(node_to_grid, grid_shape) -> Dict[str, np.ndarray]:
    """Host-side index maps of ``node_to_grid`` on an ``H x W`` grid (int64 numpy arrays):
    ``pi`` [N] cell of node n; ``sigma`` [N] the node whose write to cell pi(n) survives graph_to_grid (the last one);
    ``hit`` [H*W] nodes per cell.  Vectorised form of the loops in forecast.py:194-213."""
    H, W = int(grid_shape[0]), int(grid_shape[1])
    rc = np.asarray(node_to_grid, dtype=np.int64).reshape(-1, 2)
    if rc.size and (rc[:, 0].min() < 0 or rc[:, 0].max() >= H or rc[:, 1].min() < 0 or rc[:, 1].max() >= W):
        raise ValueError("node_to_grid holds cells outside the %d x %d grid" % (H, W))
    pi = rc[:, 0] * W + rc[:, 1]
    last = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(last, pi, np.arange(len(pi), dtype=np.int64))
    return {"pi": pi, "sigma": last[pi], "hit": np.bincount(pi, minlength=H * W)}


def inverse_csr(index: np.ndarray, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """CSR of the inverse of ``index`` (node -> row): ``ptr`` [rows + 1], ``nodes`` [N] (each row's nodes ascending)."""
    counts = np.bincount(index, minlength=rows)
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return ptr, np.argsort(index, kind="stable")


class ConstraintFunction(torch.autograd.Function):
    """out [B, N, C] = constraint(hr rows [B, K, C], first C columns of lr rows [B, K_lr, >= C]); both inputs differentiable.
    ``spec`` = (type code, f, grid_h, grid_w, graph_rows, exp_factor); ``maps`` = (map, inv_ptr, inv_idx) int32 on the device."""

    @staticmethod
    def forward(ctx, hr, lr, spec, maps):
        args = _args(hr, lr, spec, maps)
        out = torch.empty(int(hr.shape[0]), int(maps[0].numel()), int(hr.shape[2]), dtype=torch.float32, device=hr.device)
        L = _lib.lib()
        with on_device_of(hr):
            ws_bytes = L.gw_constraint_workspace_bytes(args)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=hr.device)
            _lib.check(L.gw_constraint_forward(args, ws.data_ptr(), ws_bytes, out.data_ptr(), int(out.shape[2]), _stream(out)),
                       "gw_constraint_forward")
        ctx.save_for_backward(hr, lr, *maps)
        ctx.spec = spec
        return out

    @staticmethod
    def backward(ctx, dout):
        hr, lr, *maps = ctx.saved_tensors
        want_hr, want_lr = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_hr or want_lr):
            return None, None, None, None
        dout = dout.contiguous()
        C = int(hr.shape[2])
        dhr = torch.empty_like(hr) if want_hr else None
        dlr = None
        if want_lr:  # only the first C columns of lr take part: the rest of its gradient is zero
            dlr = torch.empty_like(lr) if int(lr.shape[2]) == C else torch.zeros_like(lr)
        args = _args(hr, lr, ctx.spec, maps)
        L = _lib.lib()
        with on_device_of(hr):
            ws_bytes = L.gw_constraint_workspace_bytes(args)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=hr.device)
            _lib.check(L.gw_constraint_backward(args, dout.data_ptr(), int(dout.shape[2]), ws.data_ptr(), ws_bytes,
                                                None if dhr is None else dhr.data_ptr(), C,
                                                None if dlr is None else dlr.data_ptr(), int(lr.shape[2]), _stream(dout)),
                       "gw_constraint_backward")
        return dhr, dlr, None, None


def _args(hr, lr, spec, maps) -> GwConstraintArgs:
    code, f, gh, gw_, graph_rows, exp_factor = spec
    m, ptr, idx = maps
    B, K, C = (int(s) for s in hr.shape)
    return GwConstraintArgs(code, B, int(m.numel()), C, K, f, gh, gw_, graph_rows, float(exp_factor), hr.data_ptr(), C,
                            lr.data_ptr(), int(lr.shape[2]), m.data_ptr(), ptr.data_ptr(), idx.data_ptr())


def _check_rows(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError("graph_weather_amd: %s must be on a HIP device - there is no CPU path" % name)
    if t.dtype != torch.float32:
        raise RuntimeError("graph_weather_amd: %s must be float32" % name)


class PhysicalConstraintLayer(torch.nn.Module):
    """constraint_layer.py:11-205: same signature, 3-D (graph) or 4-D (grid) inputs, output always [B, N, C] in graph
    format.  ``model`` supplies ``node_to_grid``; it is held, not registered as a submodule."""

    def __init__(self, model, grid_shape, upsampling_factor, constraint_type="none", exp_factor=1.0):
        super().__init__()
        object.__setattr__(self, "model", model)  # unregistered: no module cycle in state_dict() / .to() / named_modules()
        self.constraint_type = constraint_type
        self.grid_shape = (int(grid_shape[0]), int(grid_shape[1]))
        self.exp_factor = float(exp_factor)
        self.upsampling_factor = int(upsampling_factor)
        f = self.upsampling_factor
        if f < 1:
            raise ValueError("upsampling_factor must be >= 1, got %d" % f)
        if f > 1 and constraint_type in ("additive", "multiplicative"):
            raise ValueError("the %s constraint needs upsampling_factor 1 (the reference indexes out of range for %d)"
                             % (constraint_type, f))
        H, W = self.grid_shape
        if f > 1 and (H % f or W % f):
            raise ValueError("grid %d x %d is not made of whole %d x %d blocks" % (H, W, f, f))
        n = len(model.node_to_grid)
        if n != H * W:
            raise ValueError("PhysicalConstraintLayer: %d nodes do not fill the %d x %d grid (%d cells); the reference's "
                             "grid reshape needs one node per cell" % (n, H, W, H * W))
        self._host = grid_maps(model.node_to_grid, self.grid_shape)
        self._dev: Dict[Tuple[str, str], Tuple[torch.Tensor, ...]] = {}

    def maps(self, kind: str, device: torch.device) -> Tuple[torch.Tensor, ...]:
        """(map, inv_ptr, inv_idx) as int32 on ``device``, built once per kind ("pi" / "sigma") and device."""
        key = (kind, str(device))
        hit = self._dev.get(key)
        if hit is None:
            m = self._host[kind]
            ptr, idx = inverse_csr(m, self.grid_shape[0] * self.grid_shape[1])
            hit = tuple(torch.from_numpy(a.astype(np.int32)).to(device) for a in (m, ptr, idx))
            self._dev[key] = hit
        return hit

    def _spec(self, graph_rows: int):
        if self.constraint_type not in CONSTRAINT_TYPES:
            raise ValueError(f"Unknown constraint type: {self.constraint_type}")
        H, W = self.grid_shape
        return (CONSTRAINT_TYPES[self.constraint_type], self.upsampling_factor, H, W, graph_rows, self.exp_factor)

    def apply_rows(self, hr: torch.Tensor, lr: torch.Tensor) -> torch.Tensor:
        """The forecaster's call: ``hr`` [B, H*W, C] is the decoder output read as grid rows (forecast.py:235's rearrange),
        ``lr`` [B, H*W, >= C] the input features, whose first C channels are the low-resolution reference (read in place)."""
        _check_rows(hr, "hr")
        return ConstraintFunction.apply(hr.contiguous(), lr.contiguous(), self._spec(0), self.maps("pi", hr.device))

    def forward(self, hr_graph: torch.Tensor, lr_graph: torch.Tensor) -> torch.Tensor:
        spec_rows = 1
        if hr_graph.dim() == 3:
            if self.upsampling_factor > 1:
                raise ValueError("upsampling_factor > 1 needs grid (4-D) inputs: graph inputs hold no low-resolution grid")
            if lr_graph.dim() != 3 or lr_graph.shape != hr_graph.shape:
                raise ValueError("lr_graph must match hr_graph's shape %s, got %s" % (tuple(hr_graph.shape), tuple(lr_graph.shape)))
            kind, hr_rows, lr_rows = "sigma", hr_graph, lr_graph
        elif hr_graph.dim() == 4:
            _, _, H, W = hr_graph.shape
            if (H, W) != self.grid_shape:
                raise ValueError(f"Expected spatial dimensions {self.grid_shape}, got {(H, W)}")
            f = self.upsampling_factor
            want = (hr_graph.shape[0], hr_graph.shape[1], H // f, W // f)
            if tuple(lr_graph.shape) != want:
                raise ValueError("lr_graph must be %s, got %s" % (want, tuple(lr_graph.shape)))
            kind, spec_rows = "pi", 0
            hr_rows = hr_graph.permute(0, 2, 3, 1).reshape(hr_graph.shape[0], H * W, hr_graph.shape[1])
            lr_rows = lr_graph.permute(0, 2, 3, 1).reshape(lr_graph.shape[0], want[2] * want[3], lr_graph.shape[1])
        else:
            raise ValueError("Input tensor must be either 3D (graph) or 4D (grid).")
        _check_rows(hr_rows, "hr_graph")
        _check_rows(lr_rows, "lr_graph")
        spec = self._spec(spec_rows)
        return ConstraintFunction.apply(hr_rows.contiguous(), lr_rows.contiguous(), spec, self.maps(kind, hr_rows.device))
