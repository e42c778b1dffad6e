"""The training kernels of csrc/gw_train.hip (and the loss forward of csrc/gw_kernels.hip) at the sizes where their dispatch
branches: the 1 degree training step reaches code paths that the 10 degree tests never do (two-round weight-gradient GEMMs,
capped slabs, segment sums shared by 4 or 16 waves, loss kernels whose grid-stride loops iterate).  Every shape below is chosen
from the dispatch formula of its entry point, the branch it reaches is printed, and every reference is fp64 (torch on the
device, in chunks where k is large)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from graph_weather_amd import _lib  # noqa: E402
from graph_weather_amd.utils import regular_lat_lons  # noqa: E402
from oracle import reference_math as om  # noqa: E402

DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-9)).item()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---- gw_gemm_f32, TN ------------------------------------------------------------------------------------------------------
def _tn_branch(x3, m, n, k, a_ptr, b_ptr, lda, ldb):
    """The dispatch of gw_gemm_f32's TN mode (csrc/gw_train.hip, gw_gemm_f32: `one_round`, `target`, `cap`, `k_slab`, kernel
    choice), restated: which kernel runs, in how many slabs of how many rows."""
    tiles = ((m + 127) // 128) * ((n + 127) // 128)
    one_round = x3 and k * tiles < 1024 * 1024
    target, cap = (512 if one_round else 1024), (16384 if x3 else 4096)
    k_slab = (k * tiles + target - 1) // target
    k_slab = max(256, min(cap, (k_slab + 63) // 64 * 64))
    if x3:
        kern = "gemm_tn_x3_kernel<%s>" % ("false" if m % 128 == 0 and n % 128 == 0 else "true")
    elif m % 128 == 0 and n % 128 == 0 and lda % 4 == 0 and ldb % 4 == 0 and a_ptr % 16 == 0 and b_ptr % 16 == 0:
        kern = "gemm_tn_lds_kernel"
    else:
        kern = "gemm_tn_kernel"
    return dict(kernel=kern, one_round=one_round, target=target, k_slab=k_slab, capped=k_slab == cap, slabs=(k + k_slab - 1) // k_slab)


def _tn_reference(a, b, m, n, chunk=1 << 20):
    """sum_k A[k][:m]^T B[k][:n] and sum_k A[k][:m] in fp64, on the device, chunk by chunk over k."""
    prod = torch.zeros(m, n, dtype=torch.float64, device=DEV)
    cs = torch.zeros(m, dtype=torch.float64, device=DEV)
    for k0 in range(0, a.shape[0], chunk):
        ad = a[k0:k0 + chunk, :m].double()
        prod += ad.t() @ b[k0:k0 + chunk, :n].double()
        cs += ad.sum(0)
    return prod, cs


# (m, n, k, a/b pointer offset in floats, modes, why): each row names the branch of gw_gemm_f32 it is there for
TN_SHAPES = [
    (256, 256, (1 << 18) - 1, 0, "fx", "k*tiles = 2^20 - 1: last size of the x3 one-round branch (target 512)"),
    (256, 256, 1 << 18, 0, "fx", "k*tiles = 2^20: first size of the x3 two-round branch (target 1024)"),
    (256, 256, 905000, 0, "fx", "decoder edge MLP weight gradient at 1 degree, batch 2 (905 k edge rows)"),
    (256, 102, 905000, 0, "fx", "decoder shapes: 102-wide operand, ragged tile"),
    (256, 78, 905000, 0, "fx", "decoder shapes: 78-wide operand, ragged tile"),
    (256, 256, 1100000, 0, "f", "fp32: k_slab past its 4096-row cap (k > 1.05 M at 4 tiles)"),
    (256, 256, 4300000, 0, "x", "x3: k_slab past its 16384-row cap (k > 4.19 M at 4 tiles)"),
    (256, 256, 100000, 1, "fx", "operands one float off 16-byte alignment: the fp32 call takes gemm_tn_kernel, not the LDS kernel"),
]
TN_CASES = [(x3, m, n, k, off, why) for m, n, k, off, modes, why in TN_SHAPES for x3 in (False, True) if "fx"[x3] in modes]


@pytest.mark.parametrize("x3,m,n,k,off,why", TN_CASES,
                         ids=[f"{'x3' if c[0] else 'fp32'}-{c[1]}x{c[2]}x{c[3]}{'+1' if c[4] else ''}" for c in TN_CASES])
def test_gemm_tn_at_training_sizes(x3, m, n, k, off, why):
    """C[m][n] += sum_k A[k][m] B[k][n] (and the fused column sums of A) at k up to 4.3 M rows, with the error measures of
    tests/test_gpu_train_kernels.py: fp32 max |C - ref| / max |ref| < 1e-5; x3 (rows of A scaled over four decades, as there)
    max |C - ref| / max |product| < 5e-5; column sums 1e-5."""
    g = _gen(k + n + off)
    buf_a = torch.randn(k * m + off, device=DEV, generator=g)
    buf_b = torch.randn(k * n + off, device=DEV, generator=g)
    a = buf_a[off:].view(k, m)
    b = buf_b[off:].view(k, n)
    if x3:
        a *= 10.0 ** (torch.rand(k, 1, device=DEV, generator=g) * 4 - 2)
    c0 = torch.randn(m, n, device=DEV, generator=g)
    c = c0.clone()
    cs = torch.ones(m, device=DEV)
    br = _tn_branch(x3, m, n, k, a.data_ptr(), b.data_ptr(), m, n)
    L = _lib.lib()
    _lib.check(L.gw_gemm_f32(_lib.GEMM_TN_BF16X3 if x3 else _lib.GEMM_TN, m, n, k, a.data_ptr(), m, b.data_ptr(), n, c.data_ptr(), n,
                             cs.data_ptr(), _st()), "gemm tn")
    prod, cs_ref = _tn_reference(a, b, m, n)
    if x3:
        err = ((c.double() - c0.double() - prod).abs().max() / prod.abs().max()).item()
        bar = 5e-5
    else:
        err = _rel(c, c0.double() + prod)
        bar = 1e-5
    err_cs = _rel(cs, 1.0 + cs_ref)
    print(f"[gemm tn {'x3' if x3 else 'fp32'}] m={m} n={n} k={k} off={off}: {br} ({why}); err {err:.2e} (bar {bar:.0e}), "
          f"colsum {err_cs:.2e}")
    assert br["kernel"] != "gemm_tn_lds_kernel" or off == 0
    if off:
        assert br["kernel"] in ("gemm_tn_kernel", "gemm_tn_x3_kernel<false>")
    assert err < bar
    assert err_cs < 1e-5


@pytest.mark.parametrize("mode", [_lib.GEMM_TN, _lib.GEMM_TN_BF16X3], ids=["fp32", "bf16x3"])
def test_gemm_tn_column_sums_without_a_product(mode):
    """n == 0: no product to add, but colsum_a[m] += sum_k A[k][m] is still owed (Linear_0's bias gradient arrives only this way);
    C is not touched.  m = 300 > 256 also takes the wide column-sum launch."""
    L = _lib.lib()
    for m, k in ((256, 5000), (78, 3), (300, 70001)):
        a = torch.randn(k, m + 2, device=DEV, generator=_gen(m + k))
        c = torch.full((4,), 7.0, device=DEV)
        cs = torch.ones(m, device=DEV)
        _lib.check(L.gw_gemm_f32(mode, m, 0, k, a.data_ptr(), m + 2, a.data_ptr(), 1, c.data_ptr(), 1, cs.data_ptr(), _st()), "colsum")
        err = _rel(cs, 1.0 + a[:, :m].double().sum(0))
        print(f"[gemm tn n=0] m={m} k={k}: colsum err {err:.2e}")
        assert err < 1e-5
        assert torch.all(c == 7.0)
        # k == 0 and m == 0: nothing to do, nothing written
        cs_before = cs.clone()
        _lib.check(L.gw_gemm_f32(mode, m, 0, 0, a.data_ptr(), m + 2, a.data_ptr(), 1, c.data_ptr(), 1, cs.data_ptr(), _st()), "k=0")
        _lib.check(L.gw_gemm_f32(mode, 0, 0, k, a.data_ptr(), m + 2, a.data_ptr(), 1, c.data_ptr(), 1, cs.data_ptr(), _st()), "m=0")
        assert torch.equal(cs, cs_before) and torch.all(c == 7.0)


# ---- gw_segment_sum_rows --------------------------------------------------------------------------------------------------
def _seg_waves(batch, batch_out, n_seg, rows_pb_in):
    """gw_segment_sum_rows: waves per segment from the average rows per output segment (<= 12: 1, <= 128: 4, more: 16)."""
    per_seg = (max(rows_pb_in, 1) * (batch if batch_out == 1 else 1)) // n_seg
    return 1 if per_seg <= 12 else (4 if per_seg <= 128 else 16), per_seg


def _lengths(rs, n_seg, mean, w):
    """Segment lengths around ``mean``: some empty, most not multiples of 4 W (the unrolled loop's stride), a few exactly 4 W
    and 4 W +- 1."""
    lens = rs.randint(0, 2 * mean + 1, size=n_seg)
    lens[rs.choice(n_seg, size=max(1, n_seg // 10), replace=False)] = 0
    edge = rs.choice(n_seg, size=min(n_seg, 6), replace=False)
    lens[edge] = [4 * w, 4 * w - 1, 4 * w + 1, 8 * w, 1, 3 * w][:edge.size]
    return lens


def _segment_case(lens, batch, batch_out, use_perm, accumulate, seed):
    rs = np.random.RandomState(seed)
    n_seg = lens.size
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    E = int(ptr[-1])
    g = _gen(seed)
    rows = torch.randn(batch * E, 256, device=DEV, generator=g)
    perm = torch.from_numpy(rs.permutation(E).astype(np.int32)).to(DEV) if use_perm else None
    out0 = torch.randn(batch_out * n_seg, 256, device=DEV, generator=g)
    out = out0.clone()
    w, per_seg = _seg_waves(batch, batch_out, n_seg, E)
    L = _lib.lib()
    _lib.check(L.gw_segment_sum_rows(batch, batch_out, n_seg, rows.data_ptr(), E, None if perm is None else perm.data_ptr(),
                                     torch.from_numpy(ptr).to(DEV).data_ptr(), out.data_ptr(), accumulate, _st()), "segsum")
    seg = torch.repeat_interleave(torch.arange(n_seg, device=DEV), torch.from_numpy(lens.astype(np.int64)).to(DEV))
    src = perm.long() if perm is not None else torch.arange(E, device=DEV)
    r = rows.view(batch, E, 256).double()[:, src]  # row i of segment order, per sample
    ref = torch.zeros(batch, n_seg, 256, dtype=torch.float64, device=DEV)
    for b in range(batch):
        ref[b].index_add_(0, seg, r[b])
    if batch_out == 1:
        ref = ref.sum(0, keepdim=True)
    ref = ref.reshape(batch_out * n_seg, 256)
    if accumulate:
        ref += out0.double()
    return _rel(out, ref), w, per_seg, E


# (segments, mean length): W = 1 / 4 / 16 at batch_out == batch; batch_out == 1 doubles the rows per segment at batch 2, so
# the means are halved there to stay in the same range
SEG_RANGES = {1: (2000, 6), 4: (600, 60), 16: (40, 400)}


@pytest.mark.parametrize("w_want", [1, 4, 16])
@pytest.mark.parametrize("batch_out", ["batch", 1])
@pytest.mark.parametrize("use_perm", [True, False], ids=["perm", "identity"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_segment_sum_in_every_wave_range(w_want, batch_out, use_perm, accumulate):
    batch = 2
    bo = batch if batch_out == "batch" else 1
    n_seg, mean = SEG_RANGES[w_want]
    if bo == 1:
        mean //= 2
    rs = np.random.RandomState(w_want * 10 + bo)
    lens = _lengths(rs, n_seg, mean, w_want)
    err, w, per_seg, E = _segment_case(lens, batch, bo, use_perm, accumulate, seed=w_want + 7 * bo + 3 * use_perm + accumulate)
    print(f"[segsum] W={w} (rows/segment {per_seg}, {E} rows, {n_seg} segments, {int((lens == 0).sum())} empty), batch_out={bo}, "
          f"perm={use_perm}, accumulate={accumulate}: err {err:.2e}")
    assert w == w_want, "the shape no longer reaches the branch it is there for"
    assert err < 1e-5


@pytest.mark.parametrize("batch_out", [2, 1])
def test_segment_sum_polar_cell(batch_out):
    """One segment of ~3 000 rows (the grid points of a polar mesh cell at 0.25 degree) among short ones, through a permutation."""
    rs = np.random.RandomState(11)
    lens = rs.randint(0, 40, size=10)
    lens[[3, 7]] = 0
    lens[5] = 3001
    err, w, per_seg, E = _segment_case(lens, 2, batch_out, True, 1, seed=11 + batch_out)
    print(f"[segsum] polar cell: W={w} (rows/segment {per_seg}, longest {lens.max()}), batch_out={batch_out}: err {err:.2e}")
    assert w == 16
    assert err < 1e-5


# ---- NormalizedMSELoss forward / backward ---------------------------------------------------------------------------------
def _lat_weights(lat_lons):
    lats = sorted(set(lat for lat, _ in lat_lons))
    return torch.tensor([np.cos(lat * np.pi / 180.0) for lat in lats], dtype=torch.float32, device=DEV), len(lats)


@pytest.mark.parametrize("grid,batch", [(1.0, 2), (0.25, 1)], ids=["1deg_B2", "0.25deg_B1"])
@pytest.mark.parametrize("var_kind", ["none", "channel", "full"])
def test_normalized_mse_forward_and_backward_at_grid_size(grid, batch, var_kind):
    """gw_normalized_mse_forward (grid capped at 2048 blocks, csrc/gw_kernels.hip) and gw_normalized_mse_backward (4096 blocks,
    csrc/gw_train.hip) at 10.1 M and 81 M elements, where both grid-stride loops iterate, against om.normalized_mse_loss and its
    autograd in fp64: loss 1e-5 relative, gradient (dloss = 2.5) 1e-5 of its largest entry."""
    lat_lons = regular_lat_lons(grid)
    N, C = len(lat_lons), 78
    total = batch * N * C
    g = _gen(int(grid * 100) + batch)
    pred = torch.randn(batch, N, C, device=DEV, generator=g)
    target = torch.randn(batch, N, C, device=DEV, generator=g)
    inv_var = None
    if var_kind == "channel":
        inv_var = 1.0 / (torch.rand(C, device=DEV, generator=g) + 0.5)
    elif var_kind == "full":
        inv_var = 1.0 / (torch.rand(batch, N, C, device=DEV, generator=g) + 0.5)
    w, n_lat = _lat_weights(lat_lons)
    L = _lib.lib()
    loss = torch.zeros(1, device=DEV)
    iv_ptr = None if inv_var is None else inv_var.data_ptr()
    full = int(var_kind == "full")
    _lib.check(L.gw_normalized_mse_forward(pred.data_ptr(), target.data_ptr(), iv_ptr, full, w.data_ptr(), n_lat, batch, N, C,
                                           loss.data_ptr(), _st()), "nmse forward")
    dl = torch.full((1,), 2.5, device=DEV)
    dp = torch.empty_like(pred)
    _lib.check(L.gw_normalized_mse_backward(pred.data_ptr(), target.data_ptr(), iv_ptr, full, w.data_ptr(), n_lat, batch, N, C,
                                            dl.data_ptr(), dp.data_ptr(), _st()), "nmse backward")
    p64 = pred.double().requires_grad_(True)
    var64 = None if inv_var is None else 1.0 / inv_var.double()
    with torch.device(DEV):  # (the oracle builds its latitude weights with torch.tensor: on the device here)
        ref = om.normalized_mse_loss(p64, target.double(), lat_lons, var64, normalize=inv_var is not None)
    ref.backward(torch.tensor(2.5, dtype=torch.float64, device=DEV))
    err_l = abs(loss.item() - ref.item()) / abs(ref.item())
    err_g = _rel(dp, p64.grad)
    fwd_blocks, bwd_blocks = min((total + 1023) // 1024, 2048), min((total + 1023) // 1024, 4096)
    print(f"[nmse] {grid}deg B={batch} ({total} elements) inv_var {var_kind}: forward {fwd_blocks} blocks x256 "
          f"({total / (fwd_blocks * 256):.0f} elements per thread), backward {bwd_blocks} blocks "
          f"({total / (bwd_blocks * 256):.0f} per thread); loss err {err_l:.2e}, gradient err {err_g:.2e}")
    assert total > 2048 * 1024 and total > 4096 * 1024, "both grid-stride loops must iterate"
    assert err_l < 1e-5
    assert err_g < 1e-5
