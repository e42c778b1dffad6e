"""The conditions of tests/test_gpu_row_kernels.py that need no GPU: every case of tests/row_oracle.py reaches the branch it is
named for (through the restatements of the dispatch code), the tables together reach every route, every integer-exact case is
exact in float32 on the CPU (pairwise and row-order sums alike), and the preconditions on the float inputs hold for the committed
seeds with no case excluded."""
import pytest
import torch

from . import row_oracle as ro

F32, F64 = torch.float32, torch.float64


def _to(dt, *ts):
    return tuple(None if t is None else t.to(dt) for t in ts)


# ---------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------
def test_restatements():
    assert [ro.row_blocks(n) for n in (0, 1, 65535, 65536, 70000)] == [1, 1, 65535, 65536, 65536]
    assert ro.linear_entry(32, 40, 40, 16, 16) == "aligned" and ro.linear_aligned(32, 40, 40, 0, 256)
    assert [ro.linear_entry(*a) for a in ((33, 40, 40, 0, 0), (32, 45, 40, 0, 0), (32, 40, 45, 0, 0), (32, 40, 40, 4, 0),
                                          (32, 40, 40, 0, 4))] == ["k", "ldx", "ldw", "x", "w"]
    assert ro.linear_kernel(0) == "gather_sum_kernel" and ro.linear_kernel(33) == "gemm_nt_kernel<false>"
    assert [ro.ln_nj(w) for w in (1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)] == [8, 8, 16, 16, 32, 32, 64, 64, None]
    assert ro.ln_bwd_route(16385, 256, (260, 264, 268)) == ("256", 32, 513, 1)
    assert ro.ln_bwd_route(40000, 256, (256, 256, 256)) == ("256", 48, 834, 16)
    assert ro.ln_bwd_route(5, 256, (260, 257, 264))[0] == "narrow"
    assert ro.ln_bwd_route(524289, 8, (9, 10, 11)) == ("narrow", 512, 1025, 1)
    assert ro.ln_bwd_route(257, 300, (300, 300, 300)) == ("wide", 256, 2, 1)
    assert ro.relu_bwd_route(262145, 5, True) == ("relu_bwd_kernel", 256)
    assert ro.relu_bwd_route(2056, 257, True) == ("relu_mask_wide_kernel", 2048)
    assert ro.relu_bwd_route(65540, 257, False) == ("relu_mask_wide_kernel", 65536)
    assert ro.elementwise_blocks(1) == 1 and ro.elementwise_blocks(4194304 + 1000) == 16384
    assert ro.past_elementwise_cap(4194304 + 1) and not ro.past_elementwise_cap(4194304)
    assert ro.past_adamw_cap(4194304 + 1025) and not ro.past_adamw_cap(1025)


# ---------------------------------------------------------------------------------------------------------------------
# branches and reach
# ---------------------------------------------------------------------------------------------------------------------
def test_linear_cases_reach_their_branches():
    cases = ro.LINEAR + [ro.LINEAR_TWIN, ro.LINEAR_LDO] + ro.LINEAR_UNALIGNED
    kernels = set()
    for c in cases:
        assert ro.linear_branch(c) == c.branch, c
        assert c.ldx >= c.offx + c.k and c.ldw >= c.offw + c.k
        kernels.add(ro.linear_kernel(c.k, ro.eff_ld(c.rows, c.k, c.ldx), ro.eff_ld(c.n, c.k, c.ldw), 4 * c.offx, 4 * c.offw))
        assert ("<true>" in ro.linear_kernel(c.k, ro.eff_ld(c.rows, c.k, c.ldx), ro.eff_ld(c.n, c.k, c.ldw), 4 * c.offx, 4 * c.offw)) == c.branch.startswith("aligned")
    kernels |= {ro.linear_kernel(c.k, 4, 4) for c in ro.GATHER_LINEAR}
    assert kernels == {"gemm_nt_kernel<true>", "gemm_nt_kernel<false>", "gather_sum_kernel"}
    entries = {c.branch.split("/")[0] for c in cases}
    assert entries == ro.REACH["linear"]
    assert {int(c.branch.split("/")[1]) for c in cases} == ro.REACH["linear_chunks"]
    assert [c.branch.split("/")[0] for c in ro.LINEAR_UNALIGNED] == ["ldx", "ldw", "x", "w"]
    assert all(c.k % 4 == 0 and c[:5] == ro.LINEAR_TWIN[:5] for c in ro.LINEAR_UNALIGNED)
    for vals, field in (({1, 127, 128, 129, 300}, "rows"), ({1, 127, 128, 129, 300}, "n"), ({1, 3, 4, 15, 16, 17, 32, 33, 100}, "k")):
        assert {getattr(c, field) for c in ro.LINEAR} == vals
    assert {(c.relu, c.bias) for c in ro.LINEAR} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.rows, c.n, c.k) for c in ro.LINEAR} >= {(129, 129, 33), (1, 1, 1)}
    # more than one block along rows and along columns, a ragged last block along both
    assert any(ro.linear_grid(c.rows, c.n, c.k)[:2] == (3, 3) for c in ro.LINEAR)


def test_gather_linear_cases_reach_their_branches():
    for c in ro.GATHER_LINEAR:
        assert ro.gather_linear_branch(c) == c.branch, c
        assert 1 <= len(c.tables) <= 3
    assert {c.branch for c in ro.GATHER_LINEAR} == ro.REACH["gather_linear"]
    assert {len(c.tables) for c in ro.GATHER_LINEAR} == {1, 2, 3}
    assert {k for c in ro.GATHER_LINEAR for k, _ in c.tables} == {"per", "shared", "ident", "ident0"}
    assert any(pad > 0 for c in ro.GATHER_LINEAR for _, pad in c.tables)
    assert {c.rpb for c in ro.GATHER_LINEAR if c.k} == {50, 128, 333}


def test_layernorm_cases_reach_their_branches():
    for c in ro.LN_FORWARD:
        assert "NJ%d" % ro.ln_nj(c.width) == c.branch, c
    assert {c.branch for c in ro.LN_FORWARD} == ro.REACH["ln_forward"]
    assert {c.res for c in ro.LN_FORWARD} == {"none", "row", "shared"}
    assert {c.special for c in ro.LN_FORWARD} == {None, "mean1e3", "const"}
    assert ro.ln_nj(ro.LN_REFUSED_WIDTH) is None
    reached, strips, nulls = set(), set(), set()
    for c in ro.LN_BACKWARD:
        route, strip, blocks, last = ro.ln_bwd_route(c.rows, c.width, c.lds)
        assert route == c.branch, c
        assert all(ld >= off + c.width for ld, off in zip(c.lds, c.offs))
        if route == "256":  # float4 accesses: every operand starts on 16 bytes
            assert all(off % 4 == 0 for off in c.offs)
        reached.add("wide/NJ%d" % ro.ln_nj(c.width) if route == "wide" else ("narrow@256" if (route, c.width) == ("narrow", 256) else route))
        strips.add((route, strip))
        if c.null:
            nulls.add(route)
    assert reached == ro.REACH["ln_backward"]
    assert strips >= ro.REACH["ln_backward_strips"]
    assert nulls == {"256", "narrow", "wide"}
    # the four-row interleave of ln_bwd_kernel ends a block on 1, 3 and 5 rows (and on a whole group of 4)
    assert {ro.ln_bwd_route(c.rows, 256, c.lds)[3] for c in ro.LN_BACKWARD if c.branch == "256"} >= {1, 3, 4, 5, 15, 16}


def test_relu_cases_reach_their_branches():
    for c in ro.RELU_BACKWARD:
        assert ro.relu_branch(c) == c.branch, c
    assert {c.branch for c in ro.RELU_BACKWARD} >= ro.REACH["relu_backward"]
    assert {c.form for c in ro.RELU_BACKWARD} == set(ro.RELU_FORMS)
    for kernel in ("relu_bwd_kernel", "relu_mask_wide_kernel"):
        assert {c.form for c in ro.RELU_BACKWARD if c.branch.startswith(kernel)} >= {"mask_dz_db", "mask_dz", "colsum"}
    # relu_bwd_kernel: a strip shorter than, equal to and one past its 8-row unroll, and past two
    assert {c.rows for c in ro.RELU_BACKWARD if c.branch == "relu_bwd_kernel/16"} >= {1, 7, 8, 9, 15, 16, 17}
    # the wide kernel's row loop iterates under both caps
    assert any(c.rows > 2048 and ro.relu_has_db(c.form) and c.width > 256 for c in ro.RELU_BACKWARD)
    assert any(c.rows > 65536 and not ro.relu_has_db(c.form) and c.width > 256 for c in ro.RELU_BACKWARD)


def test_row_copy_and_segment_cases():
    for c in ro.ROWS_CASES:
        assert ro.rows_branch(c) == c.branch, c
    assert {c.branch for c in ro.ROWS_CASES} == ro.REACH["rows"]
    assert {c.kind for c in ro.ROWS_CASES} == {"per", "shared", "ident"}
    assert set(ro.SEGMENT_LENGTHS) >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 1001}
    assert {(c.batch_out, c.width, c.perm) for c in ro.SEGMENT} == {(bo, w, p) for bo in (3, 1) for w in (1, 257) for p in (False, True)}
    ptr = ro.segment_ptr(ro.SEGMENT_CAP)
    assert len(ptr) - 1 > ro.row_blocks(len(ptr) - 1) and int((ptr[1:] - ptr[:-1]).max()) <= 2
    assert {b * n for b, n, _, _ in ro.GATHER256} == {1, 5, 999}
    assert {(s, a) for _, _, s, a in ro.GATHER256} == {(False, False), (False, True), (True, False), (True, True)}


def test_capped_kernels_run_past_their_caps():
    assert any(ro.past_adamw_cap(n) for n, _, _ in ro.ADAMW) and {n for n, _, _ in ro.ADAMW} == set(ro.ADAMW_N)
    assert {wd for _, wd, _ in ro.ADAMW} == {0.0, 0.01} and {s for _, _, s in ro.ADAMW} == {0.0, 1e-3, 1.0}
    assert any(ro.past_elementwise_cap(b * t * w) for b, t, w in ro.TOKEN_MEAN_BACKWARD)
    assert any(ro.past_elementwise_cap(r * w) for r, w in ro.RELU_FORWARD_SHAPES)
    assert any(ro.past_elementwise_cap(r * w) for r, w in ro.ROW_SCALE)
    assert not any(ro.past_elementwise_cap(b * t * w) for b, t, w in ro.TOKEN_MEAN)
    sizes = [b * t * w for b, t, w in ro.TOKEN_MEAN_BACKWARD] + [r * w for r, w in ro.RELU_FORWARD_SHAPES + ro.ROW_SCALE]
    # below the cap a launch has one thread per element; past it the grid stays at the cap and the loop takes more than one turn
    assert all((ro.elementwise_blocks(n) == ro.ELEMENTWISE_CAP and n > 256 * ro.ELEMENTWISE_CAP) or ro.elementwise_blocks(n) * 256 >= n for n in sizes)
    assert {ro.elementwise_blocks(n) for n in sizes} >= {1, 2, ro.ELEMENTWISE_CAP}


# ---------------------------------------------------------------------------------------------------------------------
# integer-exact cases are exact on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
def _assert_exact(a32, a64, what):
    assert a64.abs().max().item() < ro.EXACT_LIMIT, what
    assert torch.equal(a32.double(), a64), what


def test_exact_linear():
    for c in ro.LINEAR + [ro.LINEAR_TWIN, ro.LINEAR_LDO]:
        x, w, b = ro.linear_inputs(c, True)
        assert x.abs().max() <= 4 and w.abs().max() <= 4 and 16 * c.k + 8 < ro.EXACT_LIMIT
        _assert_exact(ro.linear(*_to(F32, x, w, b), c.relu)[1], ro.linear(*_to(F64, x, w, b), c.relu)[1], c)
        # and the int64 product itself
        ref = x.long() @ w.long().t() + (0 if b is None else b.long())
        assert torch.equal(ro.linear(*_to(F64, x, w, b), False)[0], ref.double())


def _gathered(c, tabs, dt):
    return [ro.gather(t.to(dt), rows_pb, idx, c.batch, c.rpb) for t, idx, rows_pb in tabs]


def test_exact_gather_linear():
    for c in ro.GATHER_LINEAR:
        x, w, b, tabs = ro.gather_linear_inputs(c, True)
        assert 16 * c.k + 8 * (len(tabs) + 1) < ro.EXACT_LIMIT
        r32 = ro.linear(*_to(F32, x, w, b), c.relu, _gathered(c, tabs, F32))[1]
        r64 = ro.linear(*_to(F64, x, w, b), c.relu, _gathered(c, tabs, F64))[1]
        _assert_exact(r32, r64, c)


def test_exact_relu_backward():
    for c in ro.RELU_BACKWARD:
        dh, h, db0 = ro.relu_backward_inputs(c, True)
        assert 8 * (c.rows + 1) < ro.EXACT_LIMIT
        dz64, db64 = ro.relu_backward(*_to(F64, dh, h), False)
        for ordered in (False, True):
            dz32, db32 = ro.relu_backward(*_to(F32, dh, h), ordered)
            _assert_exact(dz32, dz64, c)
            _assert_exact(db32 + db0, db64 + db0.double(), c)


def test_exact_segment_sum():
    for c in ro.SEGMENT + [ro.SEGMENT_CAP]:
        rows, rows_pb, ptr, perm = ro.segment_inputs(c, True)
        src, dst = ro.segment_terms_short(rows_pb, ptr) if c is ro.SEGMENT_CAP else ro.segment_terms(c.batch, c.batch_out, rows_pb, ptr, perm)
        n_out = c.batch_out * (len(ptr) - 1)
        assert 8 * ro.segment_depth(c, ptr) < ro.EXACT_LIMIT
        r64 = ro.segment_sum(rows.double(), n_out, src, dst, True)
        assert torch.equal(r64, ro.segment_sum(rows.double(), n_out, src, dst, False))
        for ordered in (False, True):
            _assert_exact(ro.segment_sum(rows, n_out, src, dst, ordered), r64, c)


def test_ordered_sums_add_in_row_order():
    """``ordered_sum`` and the ordered ``segment_sum`` round once per row, in turn: both equal an explicit float32 loop."""
    x = torch.randn(1001, 3, generator=ro.gen(9))
    s = torch.zeros(3)
    for r in range(x.shape[0]):
        s = s + x[r]
    assert torch.equal(ro.ordered_sum(x), s)
    dst = torch.zeros(1001, dtype=torch.long)
    assert torch.equal(ro.segment_sum(x, 1, torch.arange(1001), dst, True)[0], s)
    assert (ro.segment_sum(x, 1, torch.arange(1001), dst, False)[0] - x.double().sum(0)).abs().max() < 1e-4


def test_segment_terms_short_matches_general():
    ptr = torch.tensor([0, 2, 2, 3, 5], dtype=torch.int32)
    a, b = ro.segment_terms(1, 1, 5, ptr, None), ro.segment_terms_short(5, ptr)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# preconditions on the float inputs
# ---------------------------------------------------------------------------------------------------------------------
def _no_tiny(h64, what, planted=None):
    small = (h64.abs() < 1e-5) & (h64 != 0 if planted is None else ~planted)
    assert not small.any(), (what, "min |h| %.3e" % h64.abs()[small].min().item())


def test_precondition_relu_masks():
    for c in ro.LINEAR + [ro.LINEAR_TWIN, ro.LINEAR_LDO]:
        if c.relu:
            x, w, b = ro.linear_inputs(c, False)
            _no_tiny(ro.linear(*_to(F64, x, w, b), True)[0], c, planted=torch.zeros(c.rows, c.n, dtype=torch.bool))
    for c in ro.GATHER_LINEAR:
        if c.relu:
            x, w, b, tabs = ro.gather_linear_inputs(c, False)
            h = ro.linear(*_to(F64, x, w, b), True, _gathered(c, tabs, F64))[0]
            _no_tiny(h, c, planted=torch.zeros_like(h, dtype=torch.bool))
    zeros = 0
    for c in ro.RELU_BACKWARD:
        _, h, _ = ro.relu_backward_inputs(c, False)
        if h is not None:
            _no_tiny(h.double(), c)  # exact zeros (of either sign) are the planted ones
            zeros += int((h == 0).sum())
            if c.rows * c.width > 20:
                assert (h == 0).any() and (torch.signbit(h) & (h == 0)).any(), c
    assert zeros > 0


def test_precondition_layernorm_variance():
    planted = 0
    for c in ro.LN_FORWARD:
        y = ro.ln_forward_inputs(c)[0].double()
        var = ro.row_variance(y)
        const = ro.planted_constant_rows(c.rows, c.width, c.special)
        for r in range(c.rows):
            if r in const:
                assert var[r].item() == 0.0, c
                planted += 1
            else:
                assert var[r].item() >= 1e-3, (c, r, var[r].item())
        if c.special == "mean1e3":
            assert (y.mean(-1) - 1e3).abs().max() < 1.0 and 0.5 < y.std(-1).min()
    assert planted > 0
    for c in ro.LN_BACKWARD:
        var = ro.row_variance(ro.ln_backward_inputs(c)[1].double())
        if c.width == 1:
            assert (var == 0).all()
        else:
            assert var.min().item() >= 1e-3, (c, var.min().item())


def test_adamw_reference_matches_torch():
    """The float64 restatement against torch.optim.AdamW in float64, both with the float32-rounded hyper-parameters."""
    hp = {k: ro.f32(v) for k, v in ro.ADAMW_HYPER.items()}
    wd = ro.f32(0.01)
    p0, grads = ro.adamw_inputs(257, 1.0, 5)
    ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([ref], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(257, dtype=F64), torch.zeros(257, dtype=F64)
    for step, g in enumerate(grads, 1):
        ref.grad = g.double()
        opt.step()
        ro.adamw_step64(p, g.double(), m, v, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, step)
        assert (p - ref.detach()).abs().max().item() < 1e-14
        # (torch forms exp_avg with lerp_: the same value, rounded in another place)
        assert torch.allclose(m, opt.state[ref]["exp_avg"], rtol=1e-12, atol=0) and torch.allclose(v, opt.state[ref]["exp_avg_sq"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("tokens", [1, 3, 7, 5000])
def test_token_mean_gradient_is_one_division(tokens):
    """dout / tokens in float32 is what token_mean_backward is compared with bitwise: it is the gradient of the reference."""
    x = torch.randn(2 * tokens, 3, generator=ro.gen(10, tokens), dtype=F64, requires_grad=True)
    dout = torch.randn(2, 3, generator=ro.gen(11, tokens), dtype=F64)
    ro.token_mean(x, 2, tokens).backward(dout)
    assert torch.allclose(x.grad, (dout / tokens).repeat_interleave(tokens, 0), rtol=1e-15, atol=0)
