"""What tests/test_gpu_row_kernels.py and tests/test_row_kernels_host.py share: the dispatch of the shared row-op kernels
(csrc/gw_wide.hip, the any-width entry points of csrc/gw_train.hip, the elementwise kernels of csrc/gw_aurora.hip) restated in
Python, the case tables with the branch each case is there for, the inputs of every case, and one small reference per operation
that is evaluated in the dtype of its arguments (float64: the reference; float32 on the CPU: the yardstick).

Sums over rows have two float32 forms: ``x.sum(0)`` (torch adds pairwise, its error grows like log K) and ``ordered_sum``, which
adds the rows in turn, one float32 rounding per row, as the kernels do; the second is the yardstick of column and segment sums.
(``torch.cumsum(x, 0)[-1]`` is not that sum: on the CPU torch accumulates a float32 cumsum in double and rounds once, so it errs
less than any float32 kernel; numpy's cumsum stays in the dtype of its input.  tests/test_row_kernels_host.py holds both ordered
forms against an explicit float32 loop.)

Integer-exact inputs hold small integers (|v| <= 4 for the factors of a product, <= 8 for the terms of a sum) and are sized so
that every partial sum stays below 2^24 in magnitude: then every order of summation gives the same float32 bit pattern and a
kernel is compared with ``torch.equal``.

Seeds.  Every input comes from ``gen(tag, ...)``; a case's ``seed`` field (0 unless stated) is the first for which the
preconditions of the issue hold (no masked pre-activation with 0 < |h| < 1e-5, no LayerNorm row with variance < 1e-3 other than
the planted ones); tests/test_row_kernels_host.py checks them for the committed values with no case excluded.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

U32 = 2.0 ** -24  # unit roundoff of float32
EXACT_LIMIT = 2 ** 24


def gen(*key) -> torch.Generator:
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, bound: int) -> torch.Tensor:
    """Integer-valued float32 in [-bound, bound]."""
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# dispatch restatements
# ---------------------------------------------------------------------------------------------------------------------
def eff_ld(nrows: int, width: int, ld: int) -> int:
    """The row stride a wrapper passes (wide.py:52-53 ``_ld``): a one-row operand is passed with ld = its width."""
    return ld if nrows > 1 else width


def row_blocks(n: int) -> int:
    """gw_wide.hip:355."""
    return (n if n > 0 else 1) if n < 65536 else 65536


def linear_entry(k: int, ldx: int, ldw: int, x_ptr: int, w_ptr: int) -> str:
    """gw_wide.hip:404 - "aligned", or the first condition that sends the call to gemm_nt_kernel<false>."""
    if k % 4:
        return "k"
    if ldx % 4:
        return "ldx"
    if ldw % 4:
        return "ldw"
    if x_ptr & 15:
        return "x"
    if w_ptr & 15:
        return "w"
    return "aligned"


def linear_aligned(k: int, ldx: int, ldw: int, x_ptr: int, w_ptr: int) -> bool:
    return linear_entry(k, ldx, ldw, x_ptr, w_ptr) == "aligned"


def linear_kernel(k: int, ldx: int = 0, ldw: int = 0, x_ptr: int = 0, w_ptr: int = 0) -> str:
    """gw_wide.hip:398-409."""
    if k == 0:
        return "gather_sum_kernel"
    return "gemm_nt_kernel<true>" if linear_aligned(k, ldx, ldw, x_ptr, w_ptr) else "gemm_nt_kernel<false>"


def linear_grid(rows: int, n: int, k: int):
    """(row blocks, column blocks, K chunks): gw_wide.hip:399,403 and :96 (16-deep chunks, double buffered)."""
    if k == 0:
        return row_blocks(rows), cdiv(n, 256), 0
    return cdiv(rows, 128), cdiv(n, 128), cdiv(k, 16)


def ln_nj(width: int) -> Optional[int]:
    """Columns per lane of ln_fwd_wide_kernel / ln_bwd_wide_kernel (gw_wide.hip:358-363); None: refused (:371, :446)."""
    if width > 4096:
        return None
    for lim, nj in ((512, 8), (1024, 16), (2048, 32)):
        if width <= lim:
            return nj
    return 64


def ln_bwd_route(rows: int, width: int, lds):
    """gw_train.hip:902-916, gw_wide.hip:372-373 -> (route, strip, blocks, rows in the last block); ``lds`` = (ld_dn, ld_y, ld_dy)."""
    if width > 256:
        route, strip = "wide", 256
    else:
        strip = min(cdiv(cdiv(rows, 1024), 16) * 16, 512)
        route = "256" if width == 256 and all(ld % 4 == 0 for ld in lds) else "narrow"
    blocks = cdiv(rows, strip)
    return route, strip, blocks, rows - (blocks - 1) * strip


def relu_bwd_route(rows: int, width: int, has_db: bool):
    """gw_train.hip:886-893 -> ("relu_bwd_kernel", strip); gw_wide.hip:385 -> ("relu_mask_wide_kernel", row blocks)."""
    if width > 256:
        return "relu_mask_wide_kernel", (min(max(rows, 1), 2048) if has_db else row_blocks(rows))
    return "relu_bwd_kernel", min(cdiv(cdiv(rows, 1024), 16) * 16, 256)


ELEMENTWISE_CAP = 16384  # gw_aurora.hip:286-289 (grid_for) and :515-516: blocks of 256 threads, one element per thread and turn


def elementwise_blocks(n: int) -> int:
    return min(max(cdiv(n, 256), 1), ELEMENTWISE_CAP)


def past_elementwise_cap(n: int) -> bool:
    return n > ELEMENTWISE_CAP * 256


ADAMW_CAP = 4096  # gw_train.hip:974-975: blocks of 256 threads, one element per thread and turn


def past_adamw_cap(n: int) -> bool:
    return n > ADAMW_CAP * 256


# ---------------------------------------------------------------------------------------------------------------------
# references (evaluated in the dtype of their arguments)
# ---------------------------------------------------------------------------------------------------------------------
def ordered_sum(x: torch.Tensor) -> torch.Tensor:
    """Column sums added in row order, one rounding per row."""
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1:], dtype=x.dtype)
    return torch.from_numpy(np.cumsum(x.detach().numpy(), axis=0)[-1].copy())


def linear(x, w, b, relu: bool, addends=()):
    """(pre-activation, act(x . w^T + b + sum of addend rows)); ``addends``: [rows, n] tensors already gathered."""
    h = x @ w.t() if x is not None else torch.zeros_like(addends[0])
    for a in addends:
        h = h + a
    if b is not None:
        h = h + b
    return h, (torch.relu(h) if relu else h)


def gather(table, rows_pb: int, idx, batch: int, n_idx: int):
    """out[b * n_idx + i] = table[b * rows_pb + idx[i]] (idx None: i)."""
    i = torch.arange(n_idx) if idx is None else idx.long()
    b = torch.arange(batch).repeat_interleave(n_idx)
    return table[b * rows_pb + i.repeat(batch)]


def layernorm(y, gamma, beta, res=None, eps: float = 1e-5):
    mean = y.mean(-1, keepdim=True)
    d = y - mean
    var = (d * d).mean(-1, keepdim=True)
    out = d / torch.sqrt(var + eps) * gamma + beta
    return out if res is None else out + res


def row_variance(y):
    return ((y - y.mean(-1, keepdim=True)) ** 2).mean(-1)


def layernorm_backward(dn, y, gamma, ordered: bool, eps: float = 1e-5):
    """(dy, dgamma, dbeta) of out = LayerNorm(y) gamma + beta for upstream dn."""
    d = y - y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    g = dn * gamma
    dy = (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)) * rstd
    s = ordered_sum if ordered else (lambda t: t.sum(0))
    return dy, s(dn * xh), s(dn)


def relu_backward(dh, h, ordered: bool):
    """(dz, db): dz = dh where h > 0 else 0 (h None: dh), db = column sums of dz."""
    dz = dh if h is None else torch.where(h > 0, dh, torch.zeros_like(dh))
    return dz, (ordered_sum(dz) if ordered else dz.sum(0))


def segment_terms(batch: int, batch_out: int, rows_pb: int, ptr, perm):
    """(source row, output row) of every term of a segment sum, in the order gw_wide.hip:334-350 adds them."""
    ptr = [int(v) for v in ptr]
    src, dst = [], []
    for bo in range(batch_out):
        group = range(batch) if batch_out == 1 and batch > 1 else [bo]
        for n in range(len(ptr) - 1):
            seg = torch.arange(ptr[n], ptr[n + 1])
            if perm is not None:
                seg = perm.long()[seg]
            for b in group:
                src.append(b * rows_pb + seg)
                dst.append(torch.full((len(seg),), bo * (len(ptr) - 1) + n, dtype=torch.long))
    return torch.cat(src), torch.cat(dst)


def segment_terms_short(rows_pb: int, ptr):
    """``segment_terms`` for one sample without perm, vectorised (tens of thousands of segments)."""
    ptr = ptr.long()
    return torch.arange(int(ptr[-1])), torch.repeat_interleave(torch.arange(len(ptr) - 1), ptr[1:] - ptr[:-1])


def segment_sum(rows, n_out: int, src, dst, ordered: bool):
    """``ordered``: the terms are added one by one in the order given (index_add_ on the CPU walks the index in turn);
    otherwise every segment is padded to the longest and summed by torch (pairwise)."""
    out = torch.zeros((n_out, rows.shape[1]), dtype=rows.dtype)
    if ordered:
        return out.index_add_(0, dst, rows[src])
    counts = torch.bincount(dst, minlength=n_out)
    longest = int(counts.max()) if len(dst) else 0
    first = torch.cumsum(counts, 0) - counts
    order = torch.argsort(dst, stable=True)
    pos = torch.arange(len(dst)) - first[dst[order]]
    pad = torch.zeros((n_out, max(longest, 1), rows.shape[1]), dtype=rows.dtype)
    pad[dst[order], pos] = rows[src[order]]
    return pad.sum(1)


def f32(v: float) -> float:
    """The value a float parameter of the C ABI receives."""
    return float(torch.tensor(v, dtype=torch.float32).item())


def adamw_step64(p, g, m, v, lr, beta1, beta2, eps, wd, step: int):
    """torch.optim.AdamW (decoupled decay, bias corrected, amsgrad off) on float64 tensors, in place."""
    p.mul_(1.0 - lr * wd)
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p.addcdiv_(m, v.sqrt() / math.sqrt(bc2) + eps, value=-lr / bc1)


def token_mean(x, batch: int, tokens: int):
    return x.reshape(batch, tokens, -1).mean(1)


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def figures(got, ref64, yard32, depth: int = 1):
    """(error, yardstick, bar, maximum, ratio): bar = max(4 yardstick, floor maximum), floor = max(1e-6, 2^-24 sqrt(depth));
    ratio = error / max(yardstick, bar floor / 4), so that the bar reads as ratio 4."""
    ref64 = ref64.detach().double()
    got64 = got.detach().cpu().double().reshape(ref64.shape)
    scale = ref64.abs().max().item() if ref64.numel() else 0.0
    yard = (yard32.detach().double().reshape(ref64.shape) - ref64).abs().max().item() if ref64.numel() else 0.0
    err = (got64 - ref64).abs().max().item() if ref64.numel() else 0.0
    floor = max(1e-6, U32 * math.sqrt(depth)) * scale
    bar = max(4.0 * yard, floor)
    ratio = err / max(yard, floor / 4.0) if max(yard, floor) > 0 else (0.0 if err == 0 else math.inf)
    return err, yard, bar, scale, ratio


# ---------------------------------------------------------------------------------------------------------------------
# case tables.  ``branch``: what the case is in the table for; tests/test_row_kernels_host.py derives it again from the
# restatements above.  A strided operand is columns [off, off + width) of a NaN-filled buffer ``ld`` floats wide.
# ---------------------------------------------------------------------------------------------------------------------
def _al(k: int) -> int:
    return cdiv(k, 4) * 4 + 8


Lin = namedtuple("Lin", "rows n k relu bias offx ldx offw ldw branch seed")


def _lin(rows, n, k, relu, bias, branch, offx=4, ldx=None, offw=4, ldw=None, seed=0):
    return Lin(rows, n, k, relu, bias, offx, _al(k) if ldx is None else ldx, offw, _al(k) if ldw is None else ldw, branch, seed)


# entry / K chunks; rows, n in {1, 127, 128, 129, 300}; k in {1, 3, 4, 15, 16, 17, 32, 33, 100}; all four of relu x bias
LINEAR = [
    _lin(1, 1, 1, False, False, "k/1"),
    _lin(129, 129, 33, True, True, "k/3"),
    _lin(127, 300, 3, False, True, "k/1"),
    _lin(128, 127, 4, True, False, "aligned/1"),
    _lin(300, 128, 15, True, True, "k/1"),
    _lin(129, 1, 16, False, False, "aligned/1"),
    _lin(1, 129, 17, True, True, "k/2"),
    _lin(127, 128, 32, False, True, "aligned/2"),
    _lin(300, 300, 100, True, True, "aligned/7", seed=1),  # seed 0: one pre-activation of 4.2e-7
    _lin(128, 129, 100, True, False, "aligned/7"),
]
# the four ways into gemm_nt_kernel<false> with k % 4 == 0, and the aligned call on the same values (LINEAR_TWIN)
LINEAR_TWIN = _lin(129, 127, 32, True, True, "aligned/2", ldx=40, ldw=40)
LINEAR_UNALIGNED = [
    _lin(129, 127, 32, True, True, "ldx/2", ldx=45, ldw=40),
    _lin(129, 127, 32, True, True, "ldw/2", ldx=40, ldw=45),
    _lin(129, 127, 32, True, True, "x/2", offx=1, ldx=40, ldw=40),
    _lin(129, 127, 32, True, True, "w/2", ldx=40, offw=1, ldw=40),
]
LINEAR_LDO = _lin(129, 127, 17, True, True, "k/2")  # out with ldo = n + 3, through the C entry point


def linear_branch(c: Lin) -> str:
    """The case's branch from the restatements, for operands whose buffers start on 16 bytes."""
    ldx, ldw = eff_ld(c.rows, c.k, c.ldx), eff_ld(c.n, c.k, c.ldw)
    return "%s/%d" % (linear_entry(c.k, ldx, ldw, 4 * c.offx, 4 * c.offw), linear_grid(c.rows, c.n, c.k)[2])


def linear_inputs(c: Lin, exact: bool, tag: int = 1):
    g = gen(tag, c.rows, c.n, c.k, int(c.relu), int(c.bias), int(exact), c.seed)
    if exact:
        x, w, b = ints(g, (c.rows, c.k), 4), ints(g, (c.n, c.k), 4), ints(g, (c.n,), 8)
    else:
        x = torch.randn(c.rows, c.k, generator=g)
        w = torch.randn(c.n, c.k, generator=g) / math.sqrt(c.k)
        b = 0.1 * torch.randn(c.n, generator=g)
    return x, w, (b if c.bias else None)


# linear + gathered row tables.  tables: (kind, ld - n) with kind "per" (per-sample table, index), "shared" (one table, rows_pb
# 0, index), "ident" (NULL index, per-sample rows), "ident0" (NULL index, one table shared by the batch)
Gat = namedtuple("Gat", "batch rpb k n tables relu bias branch seed")
GATHER_LINEAR = [
    Gat(5, 50, 20, 70, (("per", 0), ("shared", 0), ("ident", 5)), True, True, "gemm/tile-of-3-samples", 0),
    Gat(2, 128, 16, 130, (("shared", 0),), False, True, "gemm/tile-per-sample", 0),
    Gat(3, 333, 33, 40, (("per", 3), ("ident0", 0)), True, False, "gemm/ragged", 0),
    Gat(3, 50, 0, 300, (("per", 0), ("shared", 2), ("ident", 0)), True, True, "gather_sum/2-slabs", 0),
    Gat(1, 65537 + 50, 0, 4, (("shared", 0), ("ident", 3)), False, True, "gather_sum/past-cap", 0),
]
TABLE_ROWS = 37  # rows of an indexed table (per sample)


def gather_linear_branch(c: Gat) -> str:
    rows = c.batch * c.rpb
    if c.k == 0:
        rb, cb, _ = linear_grid(rows, c.n, 0)
        assert linear_kernel(0) == "gather_sum_kernel"
        return "gather_sum/" + ("past-cap" if rows > rb else "%d-slabs" % cb)
    if c.rpb < 128 and 128 // c.rpb >= 2:
        return "gemm/tile-of-%d-samples" % (cdiv(128, c.rpb))
    return "gemm/tile-per-sample" if c.rpb % 128 == 0 else "gemm/ragged"


def gather_linear_inputs(c: Gat, exact: bool):
    """x, w, b and per table (table [rows, n], idx or None, rows_pb)."""
    g = gen(2, c.batch, c.rpb, c.k, c.n, int(exact), c.seed)
    rows = c.batch * c.rpb
    x = w = None
    if c.k:
        x = ints(g, (rows, c.k), 4) if exact else torch.randn(rows, c.k, generator=g)
        w = ints(g, (c.n, c.k), 4) if exact else torch.randn(c.n, c.k, generator=g) / math.sqrt(c.k)
    b = None
    if c.bias:
        b = ints(g, (c.n,), 8) if exact else 0.1 * torch.randn(c.n, generator=g)
    tabs = []
    for kind, _ in c.tables:
        if kind in ("per", "shared"):
            trows = TABLE_ROWS * (c.batch if kind == "per" else 1)
            idx = torch.randint(0, TABLE_ROWS, (c.rpb,), generator=g, dtype=torch.int32)
            rows_pb = TABLE_ROWS if kind == "per" else 0
        else:
            trows, idx, rows_pb = (rows, None, c.rpb) if kind == "ident" else (c.rpb, None, 0)
        t = ints(g, (trows, c.n), 8) if exact else torch.randn(trows, c.n, generator=g)
        tabs.append((t, idx, rows_pb))
    return x, w, b, tabs


# LayerNorm forward: res "none" | "row" (per row, ld_res > width) | "shared" (res_period rows shared by the batch);
# special "mean1e3" (row mean 1e3, unit spread) | "const" (row 1 holds one value: variance exactly 0) | None
LnF = namedtuple("LnF", "rows width res period special branch seed")
LN_FORWARD = []
for _i, _w in enumerate([1, 63, 64, 65, 512, 513, 1024, 1025, 2048, 2049, 4096]):
    for _j, _r in enumerate([1, 5]):
        _special = {(1025, 5): "mean1e3", (513, 5): "const", (64, 5): "const"}.get((_w, _r))
        LN_FORWARD.append(LnF(_r, _w, ("none", "row")[(_i + _j) % 2], 0, _special, "NJ%d" % ln_nj(_w), 0))
LN_FORWARD += [LnF(3, 300, "shared", 1, "const", "NJ8", 0), LnF(4, 300, "shared", 2, "mean1e3", "NJ8", 0)]
LN_REFUSED_WIDTH = 4097


def ln_y(g, rows: int, width: int, special: Optional[str]) -> torch.Tensor:
    if special == "mean1e3":
        return torch.randn(rows, width, generator=g) + 1e3
    y = torch.randn(rows, width, generator=g) * (0.5 + torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    if special == "const":
        y[min(1, rows - 1)] = 2.0
    return y


def ln_forward_inputs(c: LnF):
    g = gen(3, c.rows, c.width, c.seed)
    y = ln_y(g, c.rows, c.width, c.special)
    gamma = 1.0 + 0.1 * torch.randn(c.width, generator=g)
    beta = 0.1 * torch.randn(c.width, generator=g)
    res = None
    if c.res == "row":
        res = torch.randn(c.rows, c.width, generator=g)
    elif c.res == "shared":
        res = torch.randn(c.period, c.width, generator=g)
    return y, gamma, beta, res


def planted_constant_rows(rows: int, width: int, special: Optional[str]):
    """Rows whose variance is 0 on purpose: every row of a width-1 input, and row 1 (or the only row) of a "const" input."""
    if width == 1:
        return list(range(rows))
    return [min(1, rows - 1)] if special == "const" else []


# LayerNorm backward: lds = (ld_dn, ld_y, ld_dy), offs = column offsets of the three operands in their buffers
LnB = namedtuple("LnB", "rows width lds offs null branch seed")
LN_BACKWARD = []
for _r in [1, 3, 4, 5, 15, 16, 17, 33, 16385, 40000]:
    LN_BACKWARD.append(LnB(_r, 256, (260, 264, 268), (4, 4, 8), _r == 17, "256", 0))
for _w in [1, 63, 64, 65, 200, 255]:
    for _r in [1, 5, 17]:
        LN_BACKWARD.append(LnB(_r, _w, (_w + 3, _w + 2, _w + 5), (1, 2, 3), (_w, _r) == (65, 5), "narrow", 0))
LN_BACKWARD.append(LnB(5, 256, (260, 257, 264), (4, 1, 8), False, "narrow", 0))        # width 256, odd ld_y
LN_BACKWARD.append(LnB(524289, 8, (9, 10, 11), (1, 2, 3), False, "narrow", 0))        # strip at its cap of 512
for _w in [257, 512, 513, 1024, 1025, 2048, 2049, 4096]:
    for _r in [1, 257]:
        LN_BACKWARD.append(LnB(_r, _w, (_w + 3, _w + 1, _w + 2), (1, 0, 2), (_w, _r) == (513, 257), "wide", 0))
for _r in [255, 256, 513]:
    LN_BACKWARD.append(LnB(_r, 300, (303, 301, 302), (1, 0, 2), False, "wide", 0))


def ln_backward_inputs(c: LnB):
    """dn, y, gamma and the non-zero values dgamma / dbeta start from."""
    g = gen(4, c.rows, c.width, c.lds[1], c.seed)
    y = ln_y(g, c.rows, c.width, None)
    dn = torch.randn(c.rows, c.width, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(c.width, generator=g)
    return dn, y, gamma, torch.randn(c.width, generator=g), torch.randn(c.width, generator=g)


# ReLU backward: form "mask_dz_db" | "mask_dz" | "colsum" (h NULL, dz NULL) | "inplace" (dz == dh, with db)
Relu = namedtuple("Relu", "rows width form branch seed")
RELU_FORMS = ("mask_dz_db", "mask_dz", "colsum", "inplace")
RELU_BACKWARD = []
for _i, _r in enumerate([1, 7, 8, 9, 15, 16, 17, 16385]):
    for _j, _w in enumerate([1, 200, 256]):
        RELU_BACKWARD.append(Relu(_r, _w, RELU_FORMS[(_i + _j) % 4], "relu_bwd_kernel/%d" % (32 if _r == 16385 else 16), 0))
RELU_BACKWARD.append(Relu(262145, 5, "mask_dz_db", "relu_bwd_kernel/256", 0))
for _i, _w in enumerate([257, 512, 513]):
    for _j, _r in enumerate([1, 300]):
        RELU_BACKWARD.append(Relu(_r, _w, RELU_FORMS[(_i + _j) % 3], "relu_mask_wide_kernel/%d" % _r, 0))
RELU_BACKWARD.append(Relu(300, 513, "inplace", "relu_mask_wide_kernel/300", 0))  # as autograd.relu_backward calls every wide Linear + ReLU
RELU_BACKWARD.append(Relu(2049 + 7, 257, "mask_dz_db", "relu_mask_wide_kernel/2048", 0))
RELU_BACKWARD.append(Relu(65537 + 3, 257, "mask_dz", "relu_mask_wide_kernel/65536", 0))


def relu_has_db(form: str) -> bool:
    return form != "mask_dz"


def relu_branch(c: Relu) -> str:
    return "%s/%d" % relu_bwd_route(c.rows, c.width, relu_has_db(c.form))


def relu_backward_inputs(c: Relu, exact: bool):
    """dh, h (None for "colsum") and the value db starts from.  |h| >= 0.01 except the planted +0.0 / -0.0 entries."""
    g = gen(5, c.rows, c.width, int(exact), c.seed)
    dh = ints(g, (c.rows, c.width), 8) if exact else torch.randn(c.rows, c.width, generator=g)
    db0 = ints(g, (c.width,), 8) if exact else torch.randn(c.width, generator=g)
    if c.form == "colsum":
        return dh, None, db0
    h = torch.randn(c.rows, c.width, generator=g)
    h = h + torch.where(h < 0, -0.01, 0.01)
    flat = h.reshape(-1)
    flat[0::7] = 0.0   # the gradient of an exact zero of either sign is 0
    flat[3::11] = -0.0
    return dh, h, db0


# gw_add_rows / gw_gather_rows_wide: kind "per" | "shared" | "ident"
Rows = namedtuple("Rows", "batch n_idx width kind branch")
ROWS_CASES = []
for _i, _w in enumerate([1, 256, 257, 600]):
    ROWS_CASES.append(Rows(1, 1, _w, ("per", "shared", "ident")[_i % 3], "%d-slabs" % cdiv(_w, 256)))
    ROWS_CASES.append(Rows(3, 111, _w, ("shared", "ident", "per")[_i % 3], "%d-slabs" % cdiv(_w, 256)))
ROWS_CASES.append(Rows(2, 32770, 4, "per", "past-cap"))


def rows_branch(c: Rows) -> str:
    total = c.batch * c.n_idx
    return "past-cap" if total > row_blocks(total) else "%d-slabs" % cdiv(c.width, 256)


# gw_segment_sum_rows_wide
SEGMENT_LENGTHS = [3, 0, 1, 9, 2, 1001, 4, 5, 7, 8]
Seg = namedtuple("Seg", "batch batch_out width perm branch")
SEGMENT = [Seg(3, _bo, _w, _p, "unroll+tail") for _w in (1, 257) for _bo in (3, 1) for _p in (False, True)]
SEGMENT_CAP = Seg(1, 1, 4, False, "past-cap")
SEGMENT_CAP_COUNT = 70000


def segment_ptr(c: Seg) -> torch.Tensor:
    if c is SEGMENT_CAP:
        lengths = torch.randint(0, 3, (SEGMENT_CAP_COUNT,), generator=gen(6, 1))
    else:
        lengths = torch.tensor(SEGMENT_LENGTHS)
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lengths, 0)]).to(torch.int32)


def segment_inputs(c: Seg, exact: bool):
    """rows [batch * rows_pb, width], rows_pb, ptr, perm or None."""
    ptr = segment_ptr(c)
    rows_pb = int(ptr[-1])
    g = gen(7, c.batch, c.batch_out, c.width, int(c.perm), int(exact))
    rows = ints(g, (c.batch * rows_pb, c.width), 8) if exact else torch.randn(c.batch * rows_pb, c.width, generator=g)
    perm = torch.randperm(rows_pb, generator=g).to(torch.int32) if c.perm else None
    return rows, rows_pb, ptr, perm


def segment_depth(c: Seg, ptr) -> int:
    """Terms of the longest sum: longest segment x samples summed."""
    longest = int((ptr[1:] - ptr[:-1]).max())
    return longest * (c.batch if c.batch_out == 1 else 1)


# gw_gather_rows (256 floats a row): (batch, n_idx, shared table, add)
GATHER256 = [(1, 1, False, False), (1, 1, True, True), (1, 5, False, True), (5, 1, True, False), (3, 333, False, True), (3, 333, True, False)]

# gw_adamw_step: (n, weight_decay, parameter scale)
ADAMW_N = [1, 255, 256, 257, 1025, 4194304 + 1025]
ADAMW = [(n, wd, scale) for i, n in enumerate(ADAMW_N) for wd, scale in (((0.01, 1.0), (0.0, 0.0)) if i % 2 == 0 else ((0.0, 1e-3), (0.01, 0.0)))]
ADAMW_LONG = (257, 0.01, 1.0, 1000)  # one state advanced step by step to step 1000
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def adamw_inputs(n: int, scale: float, steps: int, tag: int = 8):
    g = gen(tag, n, int(scale * 1e6))
    return scale * torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]


# Aurora elementwise: (batch, tokens, width)
TOKEN_MEAN = [(1, 1, 1), (2, 7, 255), (3, 5, 256), (2, 3, 257), (1, 5000, 3)]
TOKEN_MEAN_BACKWARD = TOKEN_MEAN + [(2, 2049, 1025)]
RELU_FORWARD_SHAPES = [(1, 1), (1, 257), (8, (4194304 + 1000) // 8)]
ROW_SCALE = [(1, 1), (7, 255), (300, 257), (16400, 257)]

# every route the tables must reach, by the names the host test derives from the restatements
REACH = {
    "linear": {"aligned", "k", "ldx", "ldw", "x", "w"},
    "linear_chunks": {1, 2, 3, 7},
    "gather_linear": {"gemm/tile-of-3-samples", "gemm/tile-per-sample", "gemm/ragged", "gather_sum/2-slabs", "gather_sum/past-cap"},
    "ln_forward": {"NJ8", "NJ16", "NJ32", "NJ64"},
    "ln_backward": {"256", "narrow", "narrow@256", "wide/NJ8", "wide/NJ16", "wide/NJ32", "wide/NJ64"},
    "ln_backward_strips": {("256", 16), ("256", 32), ("256", 48), ("narrow", 16), ("narrow", 512)},
    "relu_backward": {"relu_bwd_kernel/16", "relu_bwd_kernel/32", "relu_bwd_kernel/256", "relu_mask_wide_kernel/2048",
                      "relu_mask_wide_kernel/65536"},
    "rows": {"1-slabs", "2-slabs", "3-slabs", "past-cap"},
}
