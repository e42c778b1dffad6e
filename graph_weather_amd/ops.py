"""Tensor-level wrappers over the C ABI (``include/gw_amd.h``).  PyTorch is used only to own device memory
and to name the current HIP stream; every arithmetic operation of the hot path happens inside libgw_amd.so."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GwActivationSave, GwMlpWeights, GwOperand


class KernelTimer:
    """Optional HIP-event bracket around tagged C-ABI calls (used by bench.py for the live roofline figure).
    Events are recorded on the stream the kernels are launched on (torch's current stream)."""

    def __init__(self, tags):
        self.tags = set(tags)
        self.events = {t: [] for t in self.tags}
        self.units = {t: [] for t in self.tags}  # batch elements each timed launch processed (per-sample streams: 1)

    def start(self, tag):
        if tag not in self.tags:
            return None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        return ev

    def stop(self, tag, ev, units: int = 1):
        if ev is not None:
            ev[1].record()
            self.events[tag].append(ev)
            self.units[tag].append(int(units))

    def mean_units(self, tag) -> float:
        u = self.units[tag]
        return sum(u) / max(1, len(u))

    def mean_ms(self, tag) -> float:
        evs = self.events[tag]
        return sum(a.elapsed_time(b) for a, b in evs) / max(1, len(evs))


TIMER: Optional[KernelTimer] = None

EDGE_STREAM = True
"""float32 inference: the decoder's edge update runs without the per-edge residual on the decoder-form kernel of
csrc/gw_edge_stream.hip (the segment sums of the batch-shared edge embedding enter the node update as a cached product).
``False`` forces the per-edge residual route on ``edge_kernel`` (csrc/gw_edge.hip).  Read on every ``decode``."""

ENCODER_FUSED = True
"""float32 inference: the encoder's node encoder and edge update run as ONE launch (csrc/gw_encoder_fused.hip) that keeps the
grid rows in registers and adds no per-edge residual (the segment sums of the batch-shared edge embedding enter the node update
as a cached product).  ``False`` keeps the two launches (``chain_kernel`` + ``elds_kernel``).  Read on every ``encode``."""


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device_of(t: torch.Tensor):
    """Context that makes ``t``'s GPU the current HIP device for the C-ABI call inside it: kernels are launched on the
    stream of ``t.device`` and a launch on a stream of a non-current device fails.  Free when it already is current."""
    idx = t.device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(idx)


def _require(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(f"graph_weather_amd: {name} must live on a HIP device (no CPU path exists)")
    if t.dtype != dtype:
        raise RuntimeError(f"graph_weather_amd: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"graph_weather_amd: {name} must be contiguous")


@dataclass
class Operand:
    """A row table feeding an MLP input slice.  ``tensor`` is [rows, ld]; ``rows_per_batch`` = 0 means the table
    is shared by all batch elements; ``index`` (int32) maps a column to a row within its batch element."""

    tensor: Optional[torch.Tensor]
    rows_per_batch: int
    k: int
    index: Optional[torch.Tensor] = None
    projected: bool = False  # rows are X . W1_slice^T (see project_forward): gather-added, no MFMA pass
    tiles: bool = False  # ``tensor`` is a byte buffer of bf16 edge tiles (include/gw_amd.h: GW_LAYOUT_EDGE_TILES_BF16)

    def c(self) -> GwOperand:
        if self.k == 0 or self.tensor is None:
            return GwOperand(None, None, 0, 0, 0, 0, 0)
        if self.tiles:
            _require(self.tensor, "edge tiles", torch.uint8)
            # rows_per_batch: n_edges = one tile set per batch element, 0 = one set shared by the batch
            return GwOperand(self.tensor.data_ptr(), None, int(self.rows_per_batch), 256, 256, 0, _lib.LAYOUT_EDGE_TILES_BF16)
        if self.tensor.dtype == torch.bfloat16:  # an aggregate as bf16 rows in K order (include/gw_amd.h: GW_LAYOUT_ROWS_BF16K)
            if self.projected or self.index is not None or self.k != 256:
                raise RuntimeError("graph_weather_amd: bf16 rows (K order) are a format of raw 256-wide aggregates only")
            _require(self.tensor, "operand", torch.bfloat16)
            return GwOperand(self.tensor.data_ptr(), None, int(self.rows_per_batch), int(self.tensor.stride(0)), 256, 0,
                             _lib.LAYOUT_ROWS_BF16K)
        if self.tensor.dtype == torch.float16:  # layer-1 node products as fp16 rows (include/gw_amd.h: GW_LAYOUT_ROWS_F16)
            if not self.projected or self.index is not None:
                raise RuntimeError("graph_weather_amd: fp16 rows are a format of projected (layer-1 product) operands only")
            _require(self.tensor, "operand", torch.float16)
            return GwOperand(self.tensor.data_ptr(), None, int(self.rows_per_batch), int(self.tensor.stride(0)), int(self.k), 1,
                             _lib.LAYOUT_ROWS_F16)
        _require(self.tensor, "operand")
        if self.index is not None:
            _require(self.index, "operand index", torch.int32)
        return GwOperand(self.tensor.data_ptr(), None if self.index is None else self.index.data_ptr(),
                         int(self.rows_per_batch), int(self.tensor.stride(0)), int(self.k), 1 if self.projected else 0, 0)


ZERO = Operand(None, 0, 0)


class SavedActivations:
    """Buffers a forward call fills for its backward (include/gw_amd.h: gw_activation_save): the relu outputs of
    every Linear but the last, and the pre-LayerNorm output."""

    def __init__(self, pm: "PackedMLP", n_rows: int, device):
        self.hidden = torch.empty((pm.n_mid + 1, n_rows, pm.hidden), dtype=torch.float32, device=device)
        # heads (n_out <= 80) are saved as zero-padded 80-column rows (the 5-tile kernel variant stores whole tiles)
        width = pm.n_out if pm.n_out == 256 else 80
        self.pre_norm = torch.empty((n_rows, width), dtype=torch.float32, device=device) if pm.gamma is not None else None

    def c(self) -> GwActivationSave:
        return GwActivationSave(self.hidden.data_ptr(), int(self.hidden.stride(0)), int(self.hidden.stride(1)),
                                None if self.pre_norm is None else self.pre_norm.data_ptr())


def pack_many(weight_dtype: int, mats, vecs, stream: int) -> None:
    """gw_pack_many over any number of items.  mats: (w_ptr, stride_f, stride_k, n_out, kseg, out_ptr[, rows]); vecs: (v_ptr, n,
    out_ptr[, n_out]) - rows / n_out: size of the packed item when it is larger than the source (zero rows of an output head)."""
    L = _lib.lib()
    M = _lib.PACK_MAX_ITEMS
    mi = vi = 0
    while mi < len(mats) or vi < len(vecs):
        mc, vc = mats[mi:mi + M], vecs[vi:vi + M]
        ma = (_lib.GwPackItem * max(len(mc), 1))()
        for k, it in enumerate(mc):
            w, sf, sk, n_out, kseg, out = it[:6]
            ma[k] = _lib.GwPackItem(w, sf, sk, n_out, kseg, it[6] if len(it) > 6 else 0, 0, out)
        va = (_lib.GwPadItem * max(len(vc), 1))()
        for k, it in enumerate(vc):
            va[k] = _lib.GwPadItem(it[0], it[1], it[3] if len(it) > 3 else 0, it[2])
        _lib.check(L.gw_pack_many(weight_dtype, len(mc), ma, len(vc), va, stream), "gw_pack_many")
        mi += len(mc)
        vi += len(vc)


BF16X3 = "bf16x3"
"""Compute-dtype name of the split-operand mode (include/gw_amd.h: GW_DTYPE_BF16X3): every matrix product as three bf16 MFMAs on
hi / lo operand pairs with fp32 accumulation - the reference's fp32 results to ~1e-5 at 5.3 x the fp32 matrix rate.  torch has no
dtype for it, hence a name; ``set_compute_dtype(model, "bf16x3")``."""

# torch dtype of a packed weight stream per GW_DTYPE_* (the split stream is typed int16: 2-byte elements no arithmetic is done on,
# and distinct from the bf16 stream, so the dtype of a packed slice names its format)
_STREAM_TORCH_DTYPE = {_lib.DTYPE_F32: torch.float32, _lib.DTYPE_BF16: torch.bfloat16, _lib.DTYPE_BF16X3: torch.int16}
_STREAM_GW_DTYPE = {v: k for k, v in _STREAM_TORCH_DTYPE.items()}


def gw_dtype_of(compute_dtype) -> int:
    if compute_dtype == torch.float32:
        return _lib.DTYPE_F32
    if compute_dtype == torch.bfloat16:
        return _lib.DTYPE_BF16
    if isinstance(compute_dtype, str) and compute_dtype.lower() in (BF16X3, "bf16x3", "split"):
        return _lib.DTYPE_BF16X3
    raise RuntimeError("graph_weather_amd: compute dtype must be torch.float32, torch.bfloat16 or \"bf16x3\"")


class PackedMLP:
    """Device-resident packed form of one reference ``MLP`` (graph_net_block.py:45-61)."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                 ln: Optional[Tuple[torch.Tensor, torch.Tensor]], splits: Sequence[Tuple[int, int]],
                 compute_dtype=torch.float32, ln_width: int = 0):
        L = _lib.lib()
        self.weight_dtype = gw_dtype_of(compute_dtype)
        n_lin = len(weights)
        if n_lin < 2:
            raise RuntimeError("graph_weather_amd: MLP needs at least one hidden layer")
        dev = weights[0].device
        self.hidden = int(weights[0].shape[0])
        self.n_out = int(weights[-1].shape[0])
        self.n_mid = n_lin - 2
        self.in_dim = int(weights[0].shape[1])
        self.ln_width = int(ln_width) if (ln is not None and 0 < ln_width < self.n_out) else 0  # 0: all n_out features
        for w in weights[1:-1]:
            if tuple(w.shape) != (self.hidden, self.hidden):
                raise RuntimeError("graph_weather_amd: hidden layers must be square")
        st = torch.cuda.current_stream(dev).cuda_stream
        guard = on_device_of(weights[0])
        guard.__enter__()  # every packing launch below runs with the weights' GPU current (released at the end of __init__)

        # Every slice and vector of the MLP goes through ONE gw_pack_many launch (27 MLPs x ~10 packing launches per weight
        # version otherwise: the bulk of a forward right after an optimizer step).  Items address the parameters in place.
        wd = self.weight_dtype
        mats, vecs, keep = [], [], []

        def src(t):
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.contiguous().float()
            keep.append(t)
            return t

        def out_for(n_out, kseg):
            if wd == _lib.DTYPE_BF16:
                return torch.empty(L.gw_packed_bytes_bf16(n_out, 0, kseg) // 2, dtype=torch.bfloat16, device=dev)
            if wd == _lib.DTYPE_BF16X3:
                return torch.empty(L.gw_packed_bytes_bf16x3(n_out, 0, kseg) // 2, dtype=torch.int16, device=dev)
            return torch.empty(L.gw_packed_floats(n_out, 0, kseg), dtype=torch.float32, device=dev)

        def pack(w, k_lo, k_hi, out=None, rows=0):
            w = src(w)
            n_out, k_total = int(w.shape[0]), int(w.shape[1])
            if out is None:
                out = out_for(max(n_out, rows), k_hi - k_lo)
            mats.append((w.data_ptr() + 4 * k_lo, k_total, 1, n_out, k_hi - k_lo, out.data_ptr(), rows))
            return out

        def pad(v, out=None, n_out=0):
            v = src(v)
            if out is None:
                out = torch.empty(L.gw_padded_n(max(int(v.shape[0]), n_out)), dtype=torch.float32, device=dev)
            vecs.append((v.data_ptr(), int(v.shape[0]), out.data_ptr(), n_out))
            return out

        self.w1 = [pack(weights[0], lo, hi) for lo, hi in splits]
        self.b1 = pad(biases[0])
        if self.n_mid:
            one = out_for(self.hidden, self.hidden)
            nb = int(L.gw_padded_n(self.hidden))
            self.w_mid = torch.empty(self.n_mid * one.numel(), dtype=one.dtype, device=dev)
            self.b_mid = torch.empty(self.n_mid * nb, dtype=torch.float32, device=dev)
            for l, (w, b) in enumerate(zip(weights[1:-1], biases[1:-1])):
                pack(w, 0, self.hidden, out=self.w_mid[l * one.numel():(l + 1) * one.numel()])
                pad(b, out=self.b_mid[l * nb:(l + 1) * nb])
        else:
            self.w_mid = self.b_mid = None
        # output heads (n_out < 80) run on a fixed 5-tile (80 row) kernel variant: the last Linear, its bias and a LayerNorm on
        # the head are packed as 80 rows (rows n_out..79 zero; n_out itself still masks the stores)
        head = 80 if self.n_out < 80 else 0
        self.k_in, self.out_rows = int(weights[0].shape[1]), head  # (what fixed-size consumers check: include/gw_amd.h v15)
        self.w_out = pack(weights[-1], 0, self.hidden, rows=head)
        self.b_out = pad(biases[-1], n_out=head)
        self.gamma = pad(ln[0], n_out=head) if ln is not None else None
        self.beta = pad(ln[1], n_out=head) if ln is not None else None
        pack_many(self.weight_dtype, mats, vecs, st)
        del keep
        guard.__exit__(None, None, None)

    def c(self, active: Sequence[bool] = (True, True, True)) -> GwMlpWeights:
        w = GwMlpWeights()
        for i in range(3):
            w.w1[i] = self.w1[i].data_ptr() if i < len(self.w1) and active[i] else None
        w.b1 = self.b1.data_ptr()
        w.w_mid = self.w_mid.data_ptr() if self.w_mid is not None else None
        w.b_mid = self.b_mid.data_ptr() if self.b_mid is not None else None
        w.w_out = self.w_out.data_ptr()
        w.b_out = self.b_out.data_ptr()
        w.ln_gamma = self.gamma.data_ptr() if self.gamma is not None else None
        w.ln_beta = self.beta.data_ptr() if self.beta is not None else None
        w.hidden, w.n_mid, w.n_out = self.hidden, self.n_mid, self.n_out
        w.weight_dtype = self.weight_dtype
        w.ln_width = self.ln_width
        w.k_in, w.out_rows = self.k_in, self.out_rows
        return w


def mlp_forward(pm: PackedMLP, x: Operand, n_rows: int, rows_per_batch: int, residual: Optional[Operand] = None,
                out: Optional[torch.Tensor] = None, save: Optional[SavedActivations] = None) -> torch.Tensor:
    """graph_net_block.py:63-77 on ``n_rows`` rows (+ optional residual add)."""
    dev = x.tensor.device
    if out is None:
        out = torch.empty((n_rows, pm.n_out), dtype=torch.float32, device=dev)
    _require(out, "out")
    xc = x.c()
    wc = pm.c()
    rc = residual.c() if residual is not None else None
    if rc is not None:
        rc.k = pm.n_out
    with on_device_of(out):
        _lib.check(_lib.lib().gw_mlp_forward(n_rows, max(1, rows_per_batch), xc, wc, rc, out.data_ptr(), int(out.stride(0)),
                                             None if save is None else save.c(), _stream(out)), "gw_mlp_forward")
    return out


def mlp_post_forward(pm: PackedMLP, x: Operand, n_rows: int, rows_per_batch: int, post_w: Sequence[torch.Tensor],
                     post_half: bool = False, want_out: bool = False, out: Optional[torch.Tensor] = None,
                     post_out: Optional[Sequence[torch.Tensor]] = None):
    """graph_net_block.py:63-77 on ``n_rows`` rows, then the products of the output rows with packed [256, 256] slices in the same
    launch (include/gw_amd.h: gw_mlp_post_forward).  Returns (out or None, [products]); ``out`` / ``post_out``: caller's buffers."""
    import ctypes

    dev = x.tensor.device
    if out is None and want_out:
        out = torch.empty((n_rows, 256), dtype=torch.float32, device=dev)
    n_post = len(post_w)
    outs = (list(post_out) if post_out is not None else
            [torch.empty((n_rows, 256), dtype=torch.float16 if post_half else torch.float32, device=dev) for _ in range(n_post)])
    for o_ in outs:
        _require(o_, "post product rows", torch.float16 if post_half else torch.float32)
    wp = (ctypes.c_void_p * n_post)(*[w_.data_ptr() for w_ in post_w])
    op = (ctypes.c_void_p * n_post)(*[o_.data_ptr() for o_ in outs])
    with on_device_of(outs[0]):
        _lib.check(_lib.lib().gw_mlp_post_forward(n_rows, max(1, rows_per_batch), x.c(), pm.c(), None if out is None else out.data_ptr(),
                                                  256, n_post, wp, op, _lib.LAYOUT_ROWS_F16 if post_half else _lib.LAYOUT_ROWS_F32,
                                                  _stream(outs[0])), "gw_mlp_post_forward")
    return out, outs


def project_forward(w_slices: Sequence[torch.Tensor], x: Operand, n_rows: int, rows_per_batch: int,
                    weight_dtype: Optional[int] = None, relu_mask: Optional[torch.Tensor] = None,
                    zero_rows: Optional[torch.Tensor] = None, out_half: bool = False) -> List[torch.Tensor]:
    """out_s = x . W_s^T for up to four packed [256, 256] layer-1 slices in one launch (layer-1 split of
    graph_net_block.py:131-134 / :189: products over node tables are shared by all incident edges)."""
    import ctypes

    dev = x.tensor.device
    n = len(w_slices)
    outs = [torch.empty((n_rows, 256), dtype=torch.float16 if out_half else torch.float32, device=dev) for _ in range(n)]
    wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in w_slices])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    if weight_dtype is None:
        weight_dtype = _STREAM_GW_DTYPE[w_slices[0].dtype]
    with on_device_of(outs[0]):
        _lib.check(_lib.lib().gw_project_forward(n_rows, max(1, rows_per_batch), x.c(), n, wp, op, 256,
                                                 _lib.LAYOUT_ROWS_F16 if out_half else _lib.LAYOUT_ROWS_F32, weight_dtype,
                                                 None if relu_mask is None else relu_mask.data_ptr(),
                                                 None if zero_rows is None else zero_rows.data_ptr(), _stream(outs[0])),
                   "gw_project_forward")
    return outs


def edge_tiles_bytes(batch: int, n_edges: int) -> int:
    return int(_lib.lib().gw_edge_tiles_bytes(batch, n_edges))


def edge_rows_to_tiles(rows: torch.Tensor, batch: int, n_edges: int, rows_per_batch: int) -> torch.Tensor:
    """fp32 edge rows [batch * n_edges (or n_edges when shared), >= 256] -> bf16 edge tiles (byte buffer)."""
    _require(rows, "edge rows")
    tiles = torch.empty(edge_tiles_bytes(batch, n_edges), dtype=torch.uint8, device=rows.device)
    with on_device_of(rows):
        _lib.check(_lib.lib().gw_edge_rows_to_tiles(batch, n_edges, rows.data_ptr(), rows_per_batch, int(rows.stride(0)),
                                                    tiles.data_ptr(), _stream(rows)), "gw_edge_rows_to_tiles")
    return tiles


def edge_update_forward(pm: PackedMLP, batch: int, src: torch.Tensor, dst: torch.Tensor, x_src: Operand, x_dst: Operand,
                        e_in: Operand, e_res: Operand, n_dst: int, agg: torch.Tensor, e_out: Optional[torch.Tensor],
                        tag: Optional[str] = None, save: Optional[SavedActivations] = None, deterministic: bool = False,
                        segment_tiles: bool = False, segment_split: bool = False) -> None:
    """graph_net_block.py:131-137 (EdgeProcessor) fused with the scatter_sum of :188.  ``agg`` must be zeroed.
    ``e_out``: None, fp32 rows [batch * n_edges, 256], or a uint8 buffer of ``edge_tiles_bytes`` (bf16 edge tiles).
    ``deterministic``: bitwise reproducible segment sums (carry records + a fix-up launch instead of atomics).
    ``segment_tiles``: ``src`` / ``dst`` are the padded arrays of segment-aligned tiles (include/gw_amd.h:
    GW_EDGE_SEGMENT_TILES; ``GraphPlan.seg_tiles()``): ``agg`` rows are written with plain stores and need no zero fill when every
    destination has an edge; a bfloat16 ``agg`` is written as bf16 rows in K order (GW_EDGE_AGG_BF16K).  ``segment_split``: the
    padded list splits runs longer than a tile over several tiles (``SegTiles.split``; zero-filled fp32 ``agg``)."""
    _require(src, "src", torch.int32)
    _require(dst, "dst", torch.int32)
    agg_bf16 = agg.dtype == torch.bfloat16
    if agg_bf16 and not segment_tiles:
        raise RuntimeError("graph_weather_amd: a bf16 aggregate comes with segment-aligned tiles")
    _require(agg, "agg", torch.bfloat16 if agg_bf16 else torch.float32)
    e_out_layout = _lib.LAYOUT_ROWS_F32
    if e_out is not None:
        if e_out.dtype == torch.uint8:
            _require(e_out, "e_out tiles", torch.uint8)
            e_out_layout = _lib.LAYOUT_EDGE_TILES_BF16
        else:
            _require(e_out, "e_out")
    n_edges = int(src.shape[0])
    wc = pm.c((x_src.k > 0 and not x_src.projected, x_dst.k > 0 and not x_dst.projected, e_in.k > 0 and not e_in.projected))
    xs, xd, ei = x_src.c(), x_dst.c(), e_in.c()
    flags = _lib.EDGE_DETERMINISTIC if deterministic else 0
    if segment_tiles:
        flags |= _lib.EDGE_SEGMENT_TILES | (_lib.EDGE_AGG_BF16K if agg_bf16 else 0) | (_lib.EDGE_SEGMENT_SPLIT if segment_split else 0)
    ws, ws_bytes = None, 0
    if save is None:  # scratch for the kernel the library would like to use (the library never allocates)
        ws_bytes = int(_lib.lib().gw_edge_update_workspace_bytes(batch, n_edges, xs, xd, ei, wc, flags))
        if ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=agg.device)
    ev = TIMER.start(tag) if TIMER is not None else None
    with on_device_of(agg):
        _lib.check(_lib.lib().gw_edge_update_forward(batch, n_edges, src.data_ptr(), dst.data_ptr(), xs, xd, ei,
                                                     e_res.c(), wc, None if e_out is None else e_out.data_ptr(), e_out_layout,
                                                     agg.data_ptr(), n_dst, None if save is None else save.c(),
                                                     None if ws is None else ws.data_ptr(), ws_bytes, flags, _stream(agg)),
                   "gw_edge_update_forward")
    if ev is not None:
        TIMER.stop(tag, ev, batch)


def encoder_fused_forward(pm_node: PackedMLP, pm_edge: PackedMLP, batch: int, src: torch.Tensor, dst: torch.Tensor,
                          features: Operand, x_dst: Operand, e_in: Operand, e_res: Operand, n_dst: int, agg: torch.Tensor,
                          tag: Optional[str] = None, save: Optional[SavedActivations] = None, deterministic: bool = False) -> None:
    """Node encoder (graph_net_block.py:63-77 on ``features[b, src[k]]``) and the encoder's edge update with the scatter_sum of
    :188 in one launch (include/gw_amd.h: gw_encoder_fused_forward); the encoded rows are never written.  ``agg`` must be zeroed.
    ``e_res``: fp32 rows of the edge features, or ``ZERO`` (no residual).  ``save`` / ``deterministic``: not implemented by this
    launch - the library refuses them (there is no fall-back inside: the caller routes such calls to the two launches)."""
    _require(src, "src", torch.int32)
    _require(dst, "dst", torch.int32)
    _require(agg, "agg")
    n_edges = int(src.shape[0])
    wn = pm_node.c()
    we = pm_edge.c((True, False, False))
    ev = TIMER.start(tag) if TIMER is not None else None
    with on_device_of(agg):
        _lib.check(_lib.lib().gw_encoder_fused_forward(batch, n_edges, src.data_ptr(), dst.data_ptr(), features.c(), wn, x_dst.c(),
                                                       e_in.c(), e_res.c(), we, agg.data_ptr(), n_dst,
                                                       None if save is None else save.c(),
                                                       _lib.EDGE_DETERMINISTIC if deterministic else 0, _stream(agg)),
                   "gw_encoder_fused_forward")
    if ev is not None:
        TIMER.stop(tag, ev, batch)


def node_update_forward(pm: PackedMLP, n_rows: int, rows_per_batch: int, x: Operand, x_res: Operand, agg: Operand,
                        out: Optional[torch.Tensor] = None, save: Optional[SavedActivations] = None,
                        post_w: Optional[Sequence[torch.Tensor]] = None, zero_rows: Optional[torch.Tensor] = None,
                        post_half: bool = False):
    """graph_net_block.py:189-191 (NodeProcessor after aggregation).  With ``post_w`` (packed [256, 256] slices of the NEXT
    block's layer-1 weight) the products of the new rows with them are computed in the same launch: returns
    (x_new, [products]); ``zero_rows`` [n_rows, 256] is zero-filled on the side (the next block's aggregate)."""
    import ctypes

    dev = agg.tensor.device
    if out is None:
        out = torch.empty((n_rows, pm.n_out), dtype=torch.float32, device=dev)
    _require(out, "out")
    wc = pm.c((x.k > 0 and not x.projected, True, False))
    n_post = 0 if post_w is None else len(post_w)
    outs, wp, op = [], None, None
    if n_post:
        outs = [torch.empty((n_rows, 256), dtype=torch.float16 if post_half else torch.float32, device=dev) for _ in range(n_post)]
        wp = (ctypes.c_void_p * n_post)(*[w_.data_ptr() for w_ in post_w])
        op = (ctypes.c_void_p * n_post)(*[o_.data_ptr() for o_ in outs])
    with on_device_of(out):
        _lib.check(_lib.lib().gw_node_update_forward(n_rows, rows_per_batch, x.c(), x_res.c(), agg.c(), wc, out.data_ptr(),
                                                     int(out.stride(0)), None if save is None else save.c(), n_post, wp, op,
                                                     _lib.LAYOUT_ROWS_F16 if (post_half and n_post) else _lib.LAYOUT_ROWS_F32,
                                                     None if zero_rows is None else zero_rows.data_ptr(), _stream(out)),
                   "gw_node_update_forward")
    return (out, outs) if post_w is not None else out


def node_update_head_forward(pm: PackedMLP, head: PackedMLP, n_rows: int, rows_per_batch: int, x: Operand, agg: Operand,
                             residual: Optional[Operand], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """graph_net_block.py:189-191 followed by the output head (+ residual) in one launch: include/gw_amd.h:
    gw_node_update_head_forward.  Returns [n_rows, head.n_out]."""
    if out is None:
        out = torch.empty((n_rows, head.n_out), dtype=torch.float32, device=agg.tensor.device)
    _require(out, "out")
    wc = pm.c((x.k > 0 and not x.projected, True, False))
    rc = residual.c() if residual is not None else None
    if rc is not None:
        rc.k = head.n_out
    with on_device_of(out):
        _lib.check(_lib.lib().gw_node_update_head_forward(n_rows, rows_per_batch, x.c(), agg.c(), wc, head.c(), rc, out.data_ptr(),
                                                          int(out.stride(0)), _stream(out)), "gw_node_update_head_forward")
    return out


def normalized_mse_forward(pred: torch.Tensor, target: torch.Tensor, lat_weights: torch.Tensor,
                           inv_var: Optional[torch.Tensor]) -> torch.Tensor:
    """losses.py:66-94."""
    _require(pred, "pred")
    _require(target, "target")
    _require(lat_weights, "lat_weights")
    if pred.shape != target.shape or pred.dim() < 3:
        raise RuntimeError("graph_weather_amd: pred/target must both be [B, nodes..., C]")
    b = int(pred.shape[0])
    c = int(pred.shape[-1])
    nodes = pred.numel() // (b * c)
    full = 0
    if inv_var is not None:
        _require(inv_var, "inv_var")
        if inv_var.numel() == pred.numel():
            full = 1
        elif inv_var.numel() != c:
            raise RuntimeError("graph_weather_amd: 1 / feature_variance must be per channel [C] or shaped like pred")
    loss = torch.zeros((), dtype=torch.float32, device=pred.device)
    with on_device_of(pred):
        _lib.check(_lib.lib().gw_normalized_mse_forward(pred.data_ptr(), target.data_ptr(),
                                                        None if inv_var is None else inv_var.data_ptr(), full, lat_weights.data_ptr(),
                                                        int(lat_weights.numel()), b, nodes, c, loss.data_ptr(), _stream(pred)),
                   "gw_normalized_mse_forward")
    return loss


_AMSE_TABLES: dict = {}


def amse_tables(nlat: int, nlon: int, device: torch.device):
    """Device tables of the spherical-harmonic transform (``sht_tables.device_tables``), built once per
    ``(nlat, nlon, device)`` on the host in float64 and uploaded as float32."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(nlat), int(nlon), device)
    hit = _AMSE_TABLES.get(key)
    if hit is None:
        from . import sht_tables

        need = sht_tables.table_bytes(nlat, nlon)
        free, _ = torch.cuda.mem_get_info(device)
        if need > free:
            raise RuntimeError("graph_weather_amd: the spherical-harmonic tables of a %d x %d grid need %d bytes of device memory, "
                               "%d are free" % (nlat, nlon, need, free))
        dft, leg = sht_tables.device_tables(nlat, nlon)
        hit = (torch.from_numpy(dft).to(device), torch.from_numpy(leg).to(device))
        _AMSE_TABLES[key] = hit
    return hit


def amse_forward(pred: torch.Tensor, target: torch.Tensor, variance: torch.Tensor, epsilon: float, save: bool = False,
                 clear: bool = False):
    """``AMSENormalizedLoss.forward`` (losses.py:142-195) on [B, C, H, W] fields.  Returns the scalar loss, and with
    ``save`` also the coefficients [4, mmax, lmax, B * C] (pred re / im, target re / im; ``clear`` zeroes the entries with
    l < m, which the kernels neither write nor read) and the two gradient factors [2, lmax, B * C] the backward reads."""
    _require(pred, "pred")
    _require(target, "target")
    _require(variance, "feature_variance")
    b, c, nlat, nlon = (int(s) for s in pred.shape)
    if variance.numel() != c:
        raise RuntimeError("graph_weather_amd: feature_variance must hold one value per channel (%d), got %d" % (c, variance.numel()))
    L = _lib.lib()
    n = b * c
    dft, leg = amse_tables(nlat, nlon, pred.device)
    ws = torch.empty(L.gw_amse_workspace_bytes(n, nlat, nlon, 0), dtype=torch.uint8, device=pred.device)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    coeff = gfac = None
    if save:
        mmax = L.gw_amse_mmax(nlat, nlon)
        coeff = (torch.zeros if clear else torch.empty)((4, mmax, nlat, n), dtype=torch.float32, device=pred.device)
        gfac = torch.empty((2, nlat, n), dtype=torch.float32, device=pred.device)
    with on_device_of(pred):
        _lib.check(L.gw_amse_forward(n, c, nlat, nlon, pred.data_ptr(), target.data_ptr(), dft.data_ptr(), leg.data_ptr(),
                                     variance.data_ptr(), float(epsilon), ws.data_ptr(), ws.numel(),
                                     None if coeff is None else coeff.data_ptr(), None if gfac is None else gfac.data_ptr(),
                                     loss.data_ptr(), _stream(pred)), "gw_amse_forward")
    return (loss, coeff, gfac) if save else loss


def amse_backward(coeff: torch.Tensor, gfac: torch.Tensor, dloss: torch.Tensor, shape) -> torch.Tensor:
    """Gradient of ``amse_forward`` with respect to ``pred`` ([B, C, H, W] dense)."""
    b, c, nlat, nlon = (int(s) for s in shape)
    _require(coeff, "coeff")
    _require(gfac, "gfac")
    _require(dloss, "dloss")
    L = _lib.lib()
    n = b * c
    dft, leg = amse_tables(nlat, nlon, coeff.device)
    ws = torch.empty(L.gw_amse_workspace_bytes(n, nlat, nlon, 1), dtype=torch.uint8, device=coeff.device)
    dpred = torch.empty((b, c, nlat, nlon), dtype=torch.float32, device=coeff.device)
    with on_device_of(coeff):
        _lib.check(L.gw_amse_backward(n, nlat, nlon, coeff.data_ptr(), gfac.data_ptr(), dloss.data_ptr(), dft.data_ptr(),
                                      leg.data_ptr(), ws.data_ptr(), ws.numel(), dpred.data_ptr(), _stream(coeff)),
                   "gw_amse_backward")
    return dpred


_ISHT_TABLES: dict = {}


def isht_tables(nlat: int, nlon: int, device: torch.device):
    """Device tables of the inverse spherical-harmonic transform (``sht_tables.isht_device_tables``), built once per
    ``(nlat, nlon, device)`` on the host in float64 and uploaded as float32."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(nlat), int(nlon), device)
    hit = _ISHT_TABLES.get(key)
    if hit is None:
        from . import sht_tables

        need = sht_tables.isht_table_bytes(nlat, nlon)
        free, _ = torch.cuda.mem_get_info(device)
        if need > free:
            raise RuntimeError("graph_weather_amd: the inverse spherical-harmonic tables of a %d x %d grid need %d bytes of device "
                               "memory, %d are free" % (nlat, nlon, need, free))
        syn, leg = sht_tables.isht_device_tables(nlat, nlon)
        hit = (torch.from_numpy(syn).to(device), torch.from_numpy(leg).to(device))
        _ISHT_TABLES[key] = hit
    return hit


def isht_forward(coeffs: torch.Tensor, nlat: int, nlon: int, channels: int, scale: float = 1.0) -> torch.Tensor:
    """``scale * torch_harmonics.InverseRealSHT(nlat, nlon, lmax, lmax + 1, grid="equiangular")(coeffs)`` for complex64
    ``coeffs`` [fields, lmax, lmax + 1], written as [fields / channels, nlon, nlat, channels] (field ``b * channels + ch``)."""
    _require(coeffs, "coeffs", torch.complex64)
    L = _lib.lib()
    lmax = L.gw_isht_lmax(int(nlat), int(nlon))
    if not lmax or coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (lmax, lmax + 1) or coeffs.shape[0] < 1 or coeffs.shape[0] % channels:
        raise RuntimeError("graph_weather_amd: the inverse transform of a %d x %d grid expects coefficients [fields, lmax, lmax + 1] with "
                           "fields a multiple of %d, got %s" % (nlon, nlat, channels, tuple(coeffs.shape)))
    n = int(coeffs.shape[0])
    syn, leg = isht_tables(nlat, nlon, coeffs.device)
    ws = torch.empty(L.gw_isht_workspace_bytes(n, nlat, nlon), dtype=torch.uint8, device=coeffs.device)
    out = torch.empty((n // channels, nlon, nlat, channels), dtype=torch.float32, device=coeffs.device)
    with on_device_of(coeffs):
        _lib.check(L.gw_isht_forward(n, int(channels), int(nlat), int(nlon), torch.view_as_real(coeffs).data_ptr(), syn.data_ptr(),
                                     leg.data_ptr(), float(scale), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(coeffs)),
                   "gw_isht_forward")
    return out


def sampler_combine(out: torch.Tensor, a: float, x: Optional[torch.Tensor], b: float = 0.0, y: Optional[torch.Tensor] = None,
                    c: float = 0.0, z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = a x + b y + c z`` with host scalars (csrc/gw_gencast.hip); an operand that is None is skipped, ``out`` may be ``x``."""
    _require(out, "out")
    for name, t in (("x", x), ("y", y), ("z", z)):
        if t is not None:
            _require(t, name)
            if t.numel() != out.numel() or t.device != out.device:
                raise RuntimeError("graph_weather_amd: sampler_combine operands must have out's size and device")
    if x is None and y is None and z is None:
        raise RuntimeError("graph_weather_amd: sampler_combine needs at least one operand")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with on_device_of(out):
        _lib.check(_lib.lib().gw_gencast_sampler_combine(out.numel(), float(a), ptr(x), float(b), ptr(y), float(c), ptr(z), out.data_ptr(),
                                                         _stream(out)), "gw_gencast_sampler_combine")
    return out


def _wmse_operands(pred, target, sigma, area_weights, features_weights):
    _require(pred, "pred")
    _require(target, "target")
    _require(sigma, "noise_level")
    b, nlon, nlat, nvar = (int(v) for v in pred.shape)
    for name, w, size in (("area_weights", area_weights, nlat), ("features_weights", features_weights, nvar)):
        if w is not None:
            _require(w, name)
            if w.numel() != size:
                raise RuntimeError("graph_weather_amd: %s must hold %d values, got %d" % (name, size, w.numel()))
    return b, nlon, nlat, nvar


def weighted_mse_forward(pred: torch.Tensor, target: torch.Tensor, sigma: torch.Tensor, area_weights: Optional[torch.Tensor],
                         features_weights: Optional[torch.Tensor], sigma_data: float = 1.0):
    """``WeightedMSELoss.forward`` (weighted_mse_loss.py) on [B, lon, lat, var]: (scalar loss, int32 flag [1] that a squared residual
    was NaN), both on the device."""
    b, nlon, nlat, nvar = _wmse_operands(pred, target, sigma, area_weights, features_weights)
    L = _lib.lib()
    ws = torch.empty(L.gw_gencast_weighted_mse_workspace_bytes(b, nlon, nlat, nvar), dtype=torch.uint8, device=pred.device)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    flag = torch.empty(1, dtype=torch.int32, device=pred.device)
    with on_device_of(pred):
        _lib.check(L.gw_gencast_weighted_mse_forward(b, nlon, nlat, nvar, float(sigma_data), pred.data_ptr(), target.data_ptr(),
                                                     sigma.data_ptr(), None if area_weights is None else area_weights.data_ptr(),
                                                     None if features_weights is None else features_weights.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), loss.data_ptr(), flag.data_ptr(), _stream(pred)),
                   "gw_gencast_weighted_mse_forward")
    return loss, flag


def weighted_mse_backward(pred: torch.Tensor, target: torch.Tensor, sigma: torch.Tensor, area_weights: Optional[torch.Tensor],
                          features_weights: Optional[torch.Tensor], dloss: torch.Tensor, sigma_data: float = 1.0) -> torch.Tensor:
    b, nlon, nlat, nvar = _wmse_operands(pred, target, sigma, area_weights, features_weights)
    _require(dloss, "dloss")
    dpred = torch.empty_like(pred)
    with on_device_of(pred):
        _lib.check(_lib.lib().gw_gencast_weighted_mse_backward(b, nlon, nlat, nvar, float(sigma_data), pred.data_ptr(), target.data_ptr(),
                                                               sigma.data_ptr(), None if area_weights is None else area_weights.data_ptr(),
                                                               None if features_weights is None else features_weights.data_ptr(),
                                                               dloss.data_ptr(), dpred.data_ptr(), _stream(pred)),
                   "gw_gencast_weighted_mse_backward")
    return dpred


CRPS_REDUCTIONS = {"mean": _lib.CRPS_MEAN, "none": _lib.CRPS_NONE}
CRPS_REGISTER_MEMBERS = 16
"""Ensemble sizes up to this keep the members in registers (``kCrpsRegMax`` of csrc/gw_crps.hip); larger ones, up to 1024, take the
general kernels, which re-read the members through the cache."""


def _crps_operands(pred, target, area_weights, features_weights, reduction):
    _require(pred, "pred")
    _require(target, "target")
    if pred.dim() != 5 or tuple(target.shape) != (pred.shape[0],) + tuple(pred.shape[2:]) or target.device != pred.device:
        raise RuntimeError("graph_weather_amd: ensemble_crps expects pred [B, N, lon, lat, C] and target [B, lon, lat, C] on one device, "
                           "got %s and %s" % (tuple(pred.shape), tuple(target.shape)))
    if reduction not in CRPS_REDUCTIONS:
        raise RuntimeError("graph_weather_amd: ensemble_crps reduction must be 'mean' or 'none', got %r" % (reduction,))
    b, n, nlon, nlat, nvar = (int(v) for v in pred.shape)
    for name, w, size in (("area_weights", area_weights, nlat), ("features_weights", features_weights, nvar)):
        if w is not None:
            _require(w, name)
            if w.numel() != size or w.device != pred.device:
                raise RuntimeError("graph_weather_amd: %s must hold %d values on pred's device, got %d" % (name, size, w.numel()))
    return b, n, nlon, nlat, nvar


def ensemble_crps_forward(pred: torch.Tensor, target: torch.Tensor, area_weights: Optional[torch.Tensor],
                          features_weights: Optional[torch.Tensor], alpha: float = 1.0, reduction: str = "mean") -> torch.Tensor:
    """The (almost) fair CRPS of pred [B, N, lon, lat, C] against target [B, lon, lat, C] (csrc/gw_crps.hip), weighted by
    ``area_weights`` [lat] and ``features_weights`` [C] (each may be None): the scalar mean or, with ``reduction="none"``, the
    field [B, lon, lat, C].  Nothing of ensemble size is written."""
    b, n, nlon, nlat, nvar = _crps_operands(pred, target, area_weights, features_weights, reduction)
    L = _lib.lib()
    mean = reduction == "mean"
    ws = torch.empty(L.gw_ensemble_crps_workspace_bytes(b, n, nlon, nlat, nvar) if mean else 0, dtype=torch.uint8, device=pred.device)
    out = torch.empty(() if mean else tuple(target.shape), dtype=torch.float32, device=pred.device)
    with on_device_of(pred):
        _lib.check(L.gw_ensemble_crps_forward(b, n, nlon, nlat, nvar, float(alpha), CRPS_REDUCTIONS[reduction], pred.data_ptr(),
                                              target.data_ptr(), None if area_weights is None else area_weights.data_ptr(),
                                              None if features_weights is None else features_weights.data_ptr(),
                                              ws.data_ptr() if mean else None, ws.numel(), out.data_ptr(), _stream(pred)),
                   "gw_ensemble_crps_forward")
    return out


def ensemble_crps_backward(pred: torch.Tensor, target: torch.Tensor, area_weights: Optional[torch.Tensor],
                           features_weights: Optional[torch.Tensor], dout: torch.Tensor, alpha: float = 1.0,
                           reduction: str = "mean") -> torch.Tensor:
    """dpred of ``ensemble_crps_forward`` for the upstream gradient ``dout``: one value ("mean") or the field [B, lon, lat, C]."""
    b, n, nlon, nlat, nvar = _crps_operands(pred, target, area_weights, features_weights, reduction)
    _require(dout, "dout")
    if dout.numel() != (1 if reduction == "mean" else target.numel()) or dout.device != pred.device:
        raise RuntimeError("graph_weather_amd: ensemble_crps_backward: dout must hold %s on pred's device"
                           % ("one value" if reduction == "mean" else "target's %d values" % target.numel()))
    dpred = torch.empty_like(pred)
    with on_device_of(pred):
        _lib.check(_lib.lib().gw_ensemble_crps_backward(b, n, nlon, nlat, nvar, float(alpha), CRPS_REDUCTIONS[reduction], pred.data_ptr(),
                                                        target.data_ptr(), None if area_weights is None else area_weights.data_ptr(),
                                                        None if features_weights is None else features_weights.data_ptr(),
                                                        dout.data_ptr(), dpred.data_ptr(), _stream(pred)),
                   "gw_ensemble_crps_backward")
    return dpred


def _modulate_rows(x: torch.Tensor) -> Tuple[int, int, int]:
    """(rows, channels, spatial) of a dense [B, C, *spatial] tensor as csrc/gw_modulate.hip reads it."""
    rows, channels = int(x.shape[0]) * int(x.shape[1]), int(x.shape[1])
    return rows, channels, (x.numel() // rows if rows else 0)


def sdl_key(device) -> torch.Tensor:
    """A fresh 64-bit noise key in device memory, drawn from torch's own generator of ``device``: ``torch.manual_seed``
    fixes it, successive draws differ, a captured graph draws a new one on every replay, and the host never reads it."""
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=device)


def sdl_noise(key: torch.Tensor, shape) -> torch.Tensor:
    """eps(key, i) of include/gw_amd.h for the flat indices of a dense tensor of ``shape``: the values the stochastic
    decomposition layer draws under ``key`` (one int64 on the device)."""
    _require(key, "key", torch.int64)
    out = torch.empty(tuple(int(s) for s in shape), dtype=torch.float32, device=key.device)
    if out.numel():
        with on_device_of(out):
            _lib.check(_lib.lib().gw_sdl_forward(out.numel(), 1, 1, None, None, None, key.data_ptr(), None, out.data_ptr(),
                                                 _stream(out)), "gw_sdl_forward")
    return out


def sdl_forward(x: torch.Tensor, style: torch.Tensor, alpha: torch.Tensor, key: Optional[torch.Tensor],
                noise: Optional[torch.Tensor]) -> torch.Tensor:
    """stochastic_decomposition.py:56-68: x + (alpha[c] * style[b, c]) * eps, eps = ``noise`` or eps(key, flat index)."""
    _require(x, "x")
    _require(style, "style")
    _require(alpha, "alpha")
    rows, channels, spatial = _modulate_rows(x)
    if style.numel() != rows or alpha.numel() != channels:
        raise RuntimeError("graph_weather_amd: style must be [B, C] and alpha hold C values for x [B, C, ...]")
    if noise is not None:
        _require(noise, "noise")
        if noise.shape != x.shape:
            raise RuntimeError("graph_weather_amd: noise must be shaped like x")
    else:
        _require(key, "key", torch.int64)
    out = torch.empty_like(x)
    if x.numel():
        with on_device_of(x):
            _lib.check(_lib.lib().gw_sdl_forward(rows, channels, spatial, x.data_ptr(), style.data_ptr(), alpha.data_ptr(),
                                                 None if key is None else key.data_ptr(),
                                                 None if noise is None else noise.data_ptr(), out.data_ptr(), _stream(x)),
                       "gw_sdl_forward")
    return out


def sdl_backward(dy: torch.Tensor, style: torch.Tensor, alpha: torch.Tensor, key: Optional[torch.Tensor],
                 noise: Optional[torch.Tensor], want_style: bool, want_alpha: bool):
    """(d_style [B, C], d_alpha shaped like alpha) of ``sdl_forward``; the gradient of x is ``dy`` itself."""
    _require(dy, "dy")
    rows, channels, spatial = _modulate_rows(dy)
    d_style = torch.empty_like(style) if want_style else None
    d_alpha = torch.empty_like(alpha) if want_alpha else None
    if (want_style or want_alpha) and dy.numel():
        L = _lib.lib()
        ws = torch.empty(L.gw_modulate_workspace_bytes(rows, spatial), dtype=torch.uint8, device=dy.device)
        with on_device_of(dy):
            _lib.check(L.gw_sdl_backward(rows, channels, spatial, dy.data_ptr(), style.data_ptr(), alpha.data_ptr(),
                                         None if key is None else key.data_ptr(), None if noise is None else noise.data_ptr(),
                                         ws.data_ptr(), ws.numel(), None if d_style is None else d_style.data_ptr(),
                                         None if d_alpha is None else d_alpha.data_ptr(), _stream(dy)), "gw_sdl_backward")
    return d_style, d_alpha


def film_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """film.py:72-75: x * gamma[b, c] + beta[b, c] over every trailing dimension of x [B, C, ...]."""
    _require(x, "x")
    _require(gamma, "gamma")
    _require(beta, "beta")
    rows, _, spatial = _modulate_rows(x)
    if gamma.numel() != rows or beta.numel() != rows:
        raise RuntimeError("graph_weather_amd: gamma and beta must be [B, C] for x [B, C, ...]")
    out = torch.empty_like(x)
    if x.numel():
        with on_device_of(x):
            _lib.check(_lib.lib().gw_film_forward(rows, spatial, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                                  _stream(x)), "gw_film_forward")
    return out


def film_backward(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, want_x: bool, want_gamma: bool, want_beta: bool):
    """(dx, d_gamma, d_beta) of ``film_forward``."""
    _require(dy, "dy")
    rows, _, spatial = _modulate_rows(dy)
    dx = torch.empty_like(dy) if want_x else None
    d_gamma = torch.empty_like(gamma) if want_gamma else None
    d_beta = torch.empty_like(gamma) if want_beta else None
    if (want_x or want_gamma or want_beta) and dy.numel():
        L = _lib.lib()
        ws = torch.empty(L.gw_modulate_workspace_bytes(rows, spatial), dtype=torch.uint8, device=dy.device)
        with on_device_of(dy):
            _lib.check(L.gw_film_backward(rows, spatial, dy.data_ptr(), None if x is None else x.data_ptr(), gamma.data_ptr(), ws.data_ptr(), ws.numel(),
                                          None if dx is None else dx.data_ptr(), None if d_gamma is None else d_gamma.data_ptr(),
                                          None if d_beta is None else d_beta.data_ptr(), _stream(dy)), "gw_film_backward")
    return dx, d_gamma, d_beta
