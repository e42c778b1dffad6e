"""The FengWu-GHR models of the reference (``graph_weather/models/fengwu_ghr/layers.py``): ``ImageMetaModel`` (a ViT on
sincos position embeddings), ``MetaModel`` (knn_interpolate onto a regular image and back around it) and the two wrappers
that run a trained model on ``scale_factor`` times the resolution with an extra window attention per layer.

Same keyword-only constructors, attribute names and ``state_dict`` keys as the reference; the Sequential / ModuleList
positions that hold an ``einops`` ``Rearrange`` there hold a parameterless ``Layout`` here (einops is not imported).  Every
arithmetic operation is a HIP kernel: LayerNorm, Linear, residual adds are the wide path's C-ABI calls and autograd nodes
(``wide.py``); softmax attention, ``knn_interpolate`` and the exact GELU are ``csrc/gw_fengwu.hip``.  Layout changes
(patchify, the wrappers' batcher / debatcher, the window partition) are torch reshapes and permutes - data movement only.
fp32 only; there is no CPU path.

Neighbour assignment.  The reference takes it from ``torch_cluster``'s kd-tree, whose order among equidistant sources is not
pinned (integer-cast positions tie all the time).  Here it is a graph array like the h3 mesh: the built-in provider picks,
per target, the 4 sources smallest by (squared distance in exact integer or float64 arithmetic, source index);
``torch_geometric``'s ``knn`` is used instead when it can be imported, and ``model.knn_provider`` says which.  Parity with
the reference is defined as for the mesh: same assignment + same weights + same inputs -> same outputs.

``LoRAModule`` is not provided: its layer computes ``B @ A @ x``, which only type-checks when tokens = in = out features.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .ops import on_device_of
from .wide import _Add, _L, _LayerNorm, _Linear, _rows, _st

MAX_DIM_HEAD = 128
KNN_K = 4


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


def _need_hip(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"graph_weather_amd: {name} must live on a HIP device (no CPU path exists)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"graph_weather_amd: {name} must be float32, got {t.dtype}")


# ---------------------------------------------------------------------------------------------------------------------
# host tables
# ---------------------------------------------------------------------------------------------------------------------
def posemb_sincos_2d(h, w, dim, temperature: int = 10000, dtype=torch.float32):
    """layers.py:34-43 as written: (x.sin, x.cos, y.sin, y.cos) with x the column index."""
    assert (dim % 4) == 0, "feature dimension must be multiple of 4 for sincos emb"
    if dim == 4:
        raise ValueError("posemb_sincos_2d: dim = 4 gives omega = arange(1) / 0 (a division by zero in the reference); "
                         "channels * patch_height * patch_width must be at least 8")
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    omega = torch.arange(dim // 4) / (dim // 4 - 1)
    omega = 1.0 / (temperature**omega)
    y = y.flatten()[:, None] * omega[None, :]
    x = x.flatten()[:, None] * omega[None, :]
    pe = torch.cat((x.sin(), x.cos(), y.sin(), y.cos()), dim=1)
    return pe.type(dtype)


def builtin_knn(pos_x: torch.Tensor, pos_y: torch.Tensor, k: int = KNN_K, slab: int = 256) -> torch.Tensor:
    """For every row of ``pos_y`` the ``k`` rows of ``pos_x`` smallest by (squared distance, index): [n_y, k] int64, nearest
    first.  Distances are int64 (exact) when both position sets are integers, float64 otherwise.  Brute force in slabs of
    targets, the squared distance accumulated coordinate by coordinate: one [slab, n_x] array at a time (133 MB at 64 800
    sources), not the [slab, n_x, 2] differences."""
    n_x = int(pos_x.shape[0])
    if n_x < k:
        raise ValueError("knn_interpolate needs at least %d source points, got %d" % (k, n_x))
    integer = not (pos_x.is_floating_point() or pos_y.is_floating_point())
    px = pos_x.to(torch.int64) if integer else pos_x.to(torch.float64)
    py = pos_y.to(torch.int64) if integer else pos_y.to(torch.float64)
    out = torch.empty((int(pos_y.shape[0]), k), dtype=torch.int64)
    for lo in range(0, int(pos_y.shape[0]), slab):
        d2 = None
        for c in range(int(px.shape[1])):
            diff = py[lo:lo + slab, c, None] - px[None, :, c]
            d2 = diff * diff if d2 is None else d2.add_(diff.mul_(diff))
        if integer:  # one exact key: distance first, index second
            key = d2 * n_x + torch.arange(n_x, dtype=torch.int64)[None, :]
            out[lo:lo + slab] = torch.topk(key, k, dim=1, largest=False, sorted=True).values % n_x
        else:
            out[lo:lo + slab] = torch.sort(d2, dim=1, stable=True).indices[:, :k]
    return out


def _provider():
    try:
        from torch_geometric.nn.pool import knn  # noqa: F401

        return "torch_geometric", knn
    except Exception:  # not installed, or installed without torch_cluster
        return "builtin", None


class KnnTable:
    """The assignment of ``knn_interpolate(x, pos_x, pos_y)`` (layers.py:13-31) as host arrays: per target the k source rows
    and weights 1 / max(d^2, 1e-16) (computed with the reference's own expression in the positions' dtype), and the CSR of the
    transposed assignment (per source: the targets that read it and weight / (the target's weight sum)) for the backward."""

    def __init__(self, pos_x: torch.Tensor, pos_y: torch.Tensor, provider: Optional[str] = None):
        name, knn = _provider() if provider is None else (provider, None)
        if name == "torch_geometric" and knn is None:
            from torch_geometric.nn.pool import knn
        self.provider = name
        self.n_src, self.n_tgt = int(pos_x.shape[0]), int(pos_y.shape[0])
        if name == "builtin":
            x_idx = builtin_knn(pos_x, pos_y).reshape(-1)
            y_idx = torch.arange(self.n_tgt, dtype=torch.int64).repeat_interleave(KNN_K)
        else:
            assign = knn(pos_x, pos_y, KNN_K)
            y_idx, x_idx = assign[0], assign[1]
            if int(y_idx.numel()) != self.n_tgt * KNN_K or not bool((y_idx.reshape(-1, KNN_K) == torch.arange(self.n_tgt)[:, None]).all()):
                raise RuntimeError("knn returned an assignment that is not %d sources per target in target order" % KNN_K)
        diff = pos_x[x_idx] - pos_y[y_idx]
        squared_distance = (diff * diff).sum(dim=-1, keepdim=True)
        weights = 1.0 / torch.clamp(squared_distance, min=1e-16)
        self.idx = x_idx.reshape(self.n_tgt, KNN_K).to(torch.int32).contiguous()
        self.w = weights.reshape(self.n_tgt, KNN_K).to(torch.float32).contiguous()
        # transposed CSR, entries of a source in (target, slot) order
        flat = self.idx.reshape(-1).to(torch.int64)
        order = torch.sort(flat, stable=True).indices
        counts = torch.bincount(flat, minlength=self.n_src)
        self.src_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)
        self.src_tgt = (order // KNN_K).to(torch.int32).contiguous()
        den = self.w[:, 0:1]
        for j in range(1, KNN_K):  # the order the forward kernel adds in
            den = den + self.w[:, j:j + 1]
        self.src_w = (self.w / den).reshape(-1)[order].contiguous()
        self._dev: Dict[torch.device, Tuple[torch.Tensor, ...]] = {}

    def on(self, device: torch.device):
        """(idx, w, src_ptr, src_tgt, src_w) on ``device``, uploaded once."""
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(a.to(device) for a in (self.idx, self.w, self.src_ptr, self.src_tgt, self.src_w))
        return t


# ---------------------------------------------------------------------------------------------------------------------
# kernel wrappers and autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
def _check_dim_head(dim_head: int) -> None:
    if dim_head > MAX_DIM_HEAD:
        raise NotImplementedError("graph_weather_amd: attention kernels take dim_head <= %d, got %d" % (MAX_DIM_HEAD, dim_head))


def attention_forward(qkv: torch.Tensor, batch: int, heads: int, n: int, dim_head: int, scale: float):
    """softmax(scale q k^T) v on the [batch * n, 3 * heads * dim_head] rows of to_qkv, read in place -> (out [batch * n, heads *
    dim_head] in "b n (h d)" order, log-sum-exp [2, batch * heads, n]: row maximum, and log sum exp(s - maximum))."""
    _check_dim_head(dim_head)
    qkv = _rows(qkv, "qkv")
    inner = heads * dim_head
    if int(qkv.shape[0]) != batch * n or int(qkv.shape[1]) != 3 * inner:
        raise RuntimeError("graph_weather_amd: qkv must be [%d, %d], got %s" % (batch * n, 3 * inner, tuple(qkv.shape)))
    out = torch.empty((batch * n, inner), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((2, batch * heads, n), dtype=torch.float32, device=qkv.device)
    p, ld = qkv.data_ptr(), int(qkv.stride(0)) if qkv.shape[0] > 1 else 3 * inner
    with on_device_of(out):
        _lib.check(_L().gw_attention_forward(batch, heads, n, dim_head, p, p + 4 * inner, p + 8 * inner, ld, float(scale), out.data_ptr(),
                                             inner, lse.data_ptr(), _st(out)), "gw_attention_forward")
    return out, lse


def attention_backward(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, batch: int, heads: int, n: int,
                       dim_head: int, scale: float) -> torch.Tensor:
    """Gradient of ``attention_forward`` with respect to qkv, laid out like qkv."""
    qkv, dout = _rows(qkv, "qkv"), _rows(dout, "dout")
    inner = heads * dim_head
    dqkv = torch.empty((batch * n, 3 * inner), dtype=torch.float32, device=qkv.device)
    delta = torch.empty((batch * heads, n), dtype=torch.float32, device=qkv.device)
    p, ld = qkv.data_ptr(), int(qkv.stride(0)) if qkv.shape[0] > 1 else 3 * inner
    g = dqkv.data_ptr()
    with on_device_of(dqkv):
        _lib.check(_L().gw_attention_backward(batch, heads, n, dim_head, p, p + 4 * inner, p + 8 * inner, ld, float(scale), out.data_ptr(),
                                              inner, dout.data_ptr(), int(dout.stride(0)) if dout.shape[0] > 1 else inner, lse.data_ptr(),
                                              delta.data_ptr(), g, g + 4 * inner, g + 8 * inner, 3 * inner, _st(dqkv)),
                   "gw_attention_backward")
    return dqkv


class _Attention(Function):
    @staticmethod
    def forward(ctx, qkv, batch: int, heads: int, n: int, dim_head: int, scale: float):
        out, lse = attention_forward(qkv, batch, heads, n, dim_head, scale)
        ctx.meta = (batch, heads, n, dim_head, scale)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return attention_backward(qkv, out, lse, dout, *ctx.meta), None, None, None, None, None


def gelu_forward(x: torch.Tensor) -> torch.Tensor:
    _need_hip(x, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    with on_device_of(y):
        _lib.check(_L().gw_gelu_forward(x.numel(), x.data_ptr(), y.data_ptr(), _st(y)), "gw_gelu_forward")
    return y


def gelu_backward(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    x, dy = x.contiguous(), dy.contiguous()
    dx = torch.empty_like(x)
    with on_device_of(dx):
        _lib.check(_L().gw_gelu_backward(x.numel(), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), _st(dx)), "gw_gelu_backward")
    return dx


class _Gelu(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return gelu_forward(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return gelu_backward(x, dy)


def _strides(shape, to_image: bool):
    """(batch, row, channel) strides in floats of a contiguous [B, rows, c] tensor, or of a [B, c, h, w] image whose (h w) are
    the rows."""
    if to_image:
        b, c, h, w = shape
        return c * h * w, 1, h * w
    b, n, c = shape
    return n * c, c, 1


def knn_interpolate_forward(x: torch.Tensor, table: KnnTable, x_is_image: bool, out_shape) -> torch.Tensor:
    """``knn_interpolate`` of layers.py:13-31 without its ``n (b c)`` rearranges: x is [B, n_src, c] rows (-> a [B, c, h, w] image)
    or a [B, c, h, w] image (-> [B, n_tgt, c] rows), read and written through strides."""
    _need_hip(x, "x")
    x = x.contiguous()
    idx, w, _, _, _ = table.on(x.device)
    batch = int(x.shape[0])
    channels = int(x.shape[1]) if x_is_image else int(x.shape[2])
    n_src = int(x.shape[2] * x.shape[3]) if x_is_image else int(x.shape[1])
    if n_src != table.n_src:
        raise RuntimeError("graph_weather_amd: knn_interpolate expects %d source points, got %d" % (table.n_src, n_src))
    y = torch.empty(tuple(out_shape), dtype=torch.float32, device=x.device)
    xs, ys = _strides(x.shape, x_is_image), _strides(y.shape, not x_is_image)
    with on_device_of(y):
        _lib.check(_L().gw_knn_interpolate_forward(batch, table.n_tgt, channels, KNN_K, idx.data_ptr(), w.data_ptr(), x.data_ptr(), *xs,
                                                   y.data_ptr(), *ys, _st(y)), "gw_knn_interpolate_forward")
    return y


def knn_interpolate_backward(dy: torch.Tensor, table: KnnTable, x_is_image: bool, x_shape) -> torch.Tensor:
    dy = dy.contiguous()
    _, _, ptr, tgt, cw = table.on(dy.device)
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    batch = int(dx.shape[0])
    channels = int(dx.shape[1]) if x_is_image else int(dx.shape[2])
    xs, ys = _strides(dx.shape, x_is_image), _strides(dy.shape, not x_is_image)
    with on_device_of(dx):
        _lib.check(_L().gw_knn_interpolate_backward(batch, table.n_src, channels, ptr.data_ptr(), tgt.data_ptr(), cw.data_ptr(),
                                                    dy.data_ptr(), *ys, dx.data_ptr(), *xs, _st(dx)), "gw_knn_interpolate_backward")
    return dx


class _Knn(Function):
    @staticmethod
    def forward(ctx, x, table: KnnTable, x_is_image: bool, out_shape):
        ctx.table, ctx.x_is_image, ctx.x_shape = table, x_is_image, tuple(x.shape)
        return knn_interpolate_forward(x, table, x_is_image, out_shape)

    @staticmethod
    def backward(ctx, dy):
        return knn_interpolate_backward(dy, ctx.table, ctx.x_is_image, ctx.x_shape), None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
class Layout(nn.Module):
    """Parameterless stand-in at a position where the reference has an einops ``Rearrange``: keeps the numbering of the
    Sequential / ModuleList (and so the ``state_dict`` keys); the layout change itself is done by the owning module."""

    def __init__(self, pattern: str):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self) -> str:
        return repr(self.pattern)


def _ln(norm: nn.LayerNorm, x2: torch.Tensor, res: Optional[torch.Tensor] = None, res_period: int = 0) -> torch.Tensor:
    if abs(norm.eps - 1e-5) > 0:
        raise RuntimeError("graph_weather_amd: LayerNorm eps must be 1e-5")
    return _LayerNorm.apply(x2, norm.weight, norm.bias, res, res_period)


class FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim):
        super().__init__()
        self.net = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, dim))

    def forward(self, x):
        shape = x.shape
        return self.rows(x.reshape(-1, shape[-1]), None).reshape(shape)

    def rows(self, x2: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """net(x) (+ residual) on [rows, dim]."""
        _need_hip(x2, "x")
        h = _ln(self.net[0], x2)
        h = _Linear.apply(h, self.net[1].weight, self.net[1].bias, False)
        h = _Gelu.apply(h)
        h = _Linear.apply(h, self.net[3].weight, self.net[3].bias, False)
        return h if residual is None else _Add.apply(h, residual)


class Attention(nn.Module):
    def __init__(self, dim, heads=8, dim_head=64):
        super().__init__()
        _check_dim_head(dim_head)
        inner_dim = dim_head * heads
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head**-0.5
        self.norm = nn.LayerNorm(dim)
        self.attend = nn.Softmax(dim=-1)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Linear(inner_dim, dim, bias=False)

    def forward(self, x):
        b, n, d = x.shape
        return self.rows(x.reshape(b * n, d), b, n, None).reshape(b, n, d)

    def rows(self, x2: torch.Tensor, batch: int, n: int, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """to_out(attention(to_qkv(norm(x)))) (+ residual) on [batch * n, dim]."""
        _need_hip(x2, "x")
        h = _ln(self.norm, x2)
        qkv = _Linear.apply(h, self.to_qkv.weight, None, False)
        o = _Attention.apply(qkv, batch, self.heads, n, self.dim_head, self.scale)
        y = _Linear.apply(o, self.to_out.weight, None, False)
        return y if residual is None else _Add.apply(y, residual)


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim, res=False, image_size=None, scale_factor=None):
        super().__init__()
        self.depth = depth
        self.res = res
        self.norm = nn.LayerNorm(dim)
        self.layers = nn.ModuleList([])
        self.res_layers = nn.ModuleList([])
        self._window = None
        for _ in range(self.depth):
            self.layers.append(nn.ModuleList([Attention(dim, heads=heads, dim_head=dim_head), FeedForward(dim, mlp_dim)]))
            if self.res:
                assert image_size is not None and scale_factor is not None, "If res=True, you must provide h, w and scale_factor"
                h, w = pair(image_size)
                s_h, s_w = pair(scale_factor)
                self._window = (h, w, s_h, s_w)
                self.res_layers.append(nn.ModuleList([
                    Layout("(b s_h s_w) (h w) d -> (b h w) (s_h s_w) d"),
                    Attention(dim, heads=heads, dim_head=dim_head),
                    Layout("(b h w) (s_h s_w) d -> (b s_h s_w) (h w) d"),
                ]))

    def forward(self, x):
        bt, n, d = x.shape
        x2 = x.reshape(bt * n, d)
        for i in range(self.depth):
            attn, ff = self.layers[i]
            x2 = attn.rows(x2, bt, n, x2)
            x2 = ff.rows(x2, x2)
            if self.res:
                h, w, s_h, s_w = self._window
                if n != h * w or bt % (s_h * s_w) != 0:
                    raise RuntimeError("graph_weather_amd: window attention expects (b %d %d) x (%d %d) tokens, got %d x %d"
                                       % (s_h, s_w, h, w, bt, n))
                b = bt // (s_h * s_w)
                # (b s_h s_w) (h w) d -> (b h w) (s_h s_w) d: the window partition, a copy
                xw = x2.reshape(b, s_h, s_w, h, w, d).permute(0, 3, 4, 1, 2, 5).reshape(b * h * w * s_h * s_w, d)
                xw = self.res_layers[i][1].rows(xw, b * h * w, s_h * s_w, xw)
                x2 = xw.reshape(b, h, w, s_h, s_w, d).permute(0, 3, 4, 1, 2, 5).reshape(bt * n, d)
        return _ln(self.norm, x2).reshape(bt, n, d)


class ImageMetaModel(nn.Module):
    def __init__(self, *, image_size, patch_size, depth, heads, mlp_dim, channels, dim_head, res=False, scale_factor=None, **kwargs):
        super().__init__()
        self.image_size = image_size
        self.patch_size = patch_size
        self.depth = depth
        self.heads = heads
        self.mlp_dim = mlp_dim
        self.channels = channels
        self.dim_head = dim_head
        self.res = res
        self.scale_factor = scale_factor

        self.image_height, self.image_width = pair(image_size)
        self.patch_height, self.patch_width = pair(patch_size)
        s_h, s_w = pair(scale_factor)
        if res:
            assert scale_factor is not None, "If res=True, you must provide scale_factor"
        assert (self.image_height % self.patch_height == 0 and self.image_width % self.patch_width == 0), \
            "Image dimensions must be divisible by the patch size."
        _check_dim_head(dim_head)

        patch_dim = channels * self.patch_height * self.patch_width
        dim = patch_dim
        self.to_patch_embedding = nn.Sequential(
            Layout("b c (h p_h) (w p_w) -> b (h w) (p_h p_w c)"),
            nn.LayerNorm(patch_dim),
            nn.Linear(patch_dim, dim),
            nn.LayerNorm(dim),
        )
        self.pos_embedding = posemb_sincos_2d(h=self.image_height // self.patch_height, w=self.image_width // self.patch_width, dim=dim)
        self._pos_dev: Dict[torch.device, torch.Tensor] = {}
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, res=res,
                                       image_size=(self.image_height // self.patch_height, self.image_width // self.patch_width),
                                       scale_factor=(s_h, s_w))
        self.reshaper = nn.Sequential(Layout("b (h w) (p_h p_w c) -> b c (h p_h) (w p_w)"))

    def constructor_args(self) -> dict:
        """The keyword arguments this model was built with (what the wrappers rebuild it from)."""
        return {k: getattr(self, k) for k in ("image_size", "patch_size", "depth", "heads", "mlp_dim", "channels", "dim_head", "res",
                                              "scale_factor")}

    def _pos(self, device: torch.device) -> torch.Tensor:
        t = self._pos_dev.get(device)
        if t is None:
            t = self._pos_dev[device] = self.pos_embedding.to(device=device, dtype=torch.float32).contiguous()
        return t

    def forward(self, x):
        assert x.shape[1] == self.channels, "Wrong number of channels"
        _need_hip(x, "x")
        b, c = int(x.shape[0]), self.channels
        p_h, p_w = self.patch_height, self.patch_width
        h, w = self.image_height // p_h, self.image_width // p_w
        if tuple(x.shape[2:]) != (self.image_height, self.image_width):
            raise RuntimeError("graph_weather_amd: image must be %d x %d, got %s" % (self.image_height, self.image_width, tuple(x.shape[2:])))
        # b c (h p_h) (w p_w) -> b (h w) (p_h p_w c)
        x2 = x.reshape(b, c, h, p_h, w, p_w).permute(0, 2, 4, 3, 5, 1).reshape(b * h * w, p_h * p_w * c)
        emb = self.to_patch_embedding
        x2 = _ln(emb[1], x2)
        x2 = _Linear.apply(x2, emb[2].weight, emb[2].bias, False)
        x2 = _ln(emb[3], x2, self._pos(x.device), h * w)  # + pos_embedding: the batch-shared residual of the LayerNorm launch
        y = self.transformer(x2.reshape(b, h * w, -1))
        # b (h w) (p_h p_w c) -> b c (h p_h) (w p_w)
        return y.reshape(b, h, w, p_h, p_w, c).permute(0, 5, 1, 3, 2, 4).reshape(b, c, h * p_h, w * p_w)


def _batch(x: torch.Tensor, s_h: int, s_w: int) -> torch.Tensor:
    """b c (h s_h) (w s_w) -> (b s_h s_w) c h w"""
    b, c, hh, ww = x.shape
    h, w = hh // s_h, ww // s_w
    return x.reshape(b, c, h, s_h, w, s_w).permute(0, 3, 5, 1, 2, 4).reshape(b * s_h * s_w, c, h, w)


def _debatch(x: torch.Tensor, s_h: int, s_w: int) -> torch.Tensor:
    """(b s_h s_w) c h w -> b c (h s_h) (w s_w)"""
    bt, c, h, w = x.shape
    b = bt // (s_h * s_w)
    return x.reshape(b, s_h, s_w, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(b, c, h * s_h, w * s_w)


def _rebuild_with_windows(image_meta_model: ImageMetaModel, scale_factor) -> ImageMetaModel:
    """An ImageMetaModel with res=True built from the wrapped model's constructor attributes, carrying its weights (the window
    attentions are new: strict=False, as in the reference).  The wrapped model itself is left as it is."""
    args = image_meta_model.constructor_args()
    args.update({"res": True, "scale_factor": scale_factor})
    model = ImageMetaModel(**args)
    model.load_state_dict(image_meta_model.state_dict(), strict=False)
    return model


class WrapperImageModel(nn.Module):
    def __init__(self, image_meta_model: ImageMetaModel, scale_factor):
        super().__init__()
        self.scale = pair(scale_factor)
        self.batcher = Layout("b c (h s_h) (w s_w) -> (b s_h s_w) c h w")
        self.image_meta_model = _rebuild_with_windows(image_meta_model, scale_factor)
        self.debatcher = Layout("(b s_h s_w) c h w -> b c (h s_h) (w s_w)")

    def forward(self, x):
        _need_hip(x, "x")
        s_h, s_w = self.scale
        return _debatch(self.image_meta_model(_batch(x, s_h, s_w)), s_h, s_w)


def _image_positions(i_h: int, i_w: int) -> torch.Tensor:
    return torch.cartesian_prod((torch.arange(-i_h / 2, i_h / 2, 1) / i_h * 180).to(torch.long),
                                (torch.arange(0, i_w, 1) / i_w * 360).to(torch.long))


class _Interpolated(nn.Module):
    """knn_interpolate onto the image, the image model, knn_interpolate back (the shared forward of the two MetaModels)."""

    def _tables(self):
        self._to_image = KnnTable(self.pos_x, self.pos_y)
        self._to_rows = KnnTable(self.pos_y, self.pos_x)
        self.knn_provider = self._to_image.provider

    def _interpolated(self, x, image_fn):
        if x.dim() != 3:
            raise RuntimeError("graph_weather_amd: x must be [batch, nodes, channels]")
        _need_hip(x, "x")
        b, n, c = (int(s) for s in x.shape)
        img = _Knn.apply(x, self._to_image, False, (b, c, self.i_h, self.i_w))
        img = image_fn(img)
        return _Knn.apply(img, self._to_rows, True, (b, n, c))


class MetaModel(_Interpolated):
    def __init__(self, lat_lons: list, *, image_size, patch_size, depth, heads, mlp_dim, channels, dim_head=64):
        super().__init__()
        self.i_h, self.i_w = pair(image_size)
        self.pos_x = torch.tensor(lat_lons).to(torch.long)
        self.pos_y = _image_positions(self.i_h, self.i_w)
        self._tables()
        self.image_meta_model = ImageMetaModel(image_size=image_size, patch_size=patch_size, depth=depth, heads=heads, mlp_dim=mlp_dim,
                                               channels=channels, dim_head=dim_head)

    def forward(self, x):
        return self._interpolated(x, self.image_meta_model)


class WrapperMetaModel(_Interpolated):
    def __init__(self, lat_lons: list, meta_model: MetaModel, scale_factor):
        super().__init__()
        s_h, s_w = pair(scale_factor)
        self.scale = (s_h, s_w)
        self.i_h, self.i_w = meta_model.i_h * s_h, meta_model.i_w * s_w
        self.pos_x = torch.tensor(lat_lons)  # not cast to long, as in the reference
        self.pos_y = _image_positions(self.i_h, self.i_w)
        self._tables()
        self.batcher = Layout("b c (h s_h) (w s_w) -> (b s_h s_w) c h w")
        self.image_meta_model = _rebuild_with_windows(meta_model.image_meta_model, scale_factor)
        self.debatcher = Layout("(b s_h s_w) c h w -> b c (h s_h) (w s_w)")

    def forward(self, x):
        s_h, s_w = self.scale
        return self._interpolated(x, lambda img: _debatch(self.image_meta_model(_batch(img, s_h, s_w)), s_h, s_w))
