"""Torch restatements of the C-ABI calls the backward of graph_weather_amd/autograd.py makes (include/gw_amd.h:
gw_mlp_ln_chain_backward, gw_gemm_f32 TN, gw_layernorm_backward, gw_gather_rows, gw_relu_backward, gw_segment_sum_rows), each
computing in float64 what that entry point computes, so that the host logic around them runs on the CPU.  ``install`` puts them in
place of autograd.py's thin wrappers and returns the record of what was called."""
import torch

from graph_weather_amd import autograd as ag


def _ln_bwd64(dn, y, gamma, width=0):
    """LayerNorm backward over the first ``width`` columns (0: all of gamma's); dy / dgamma / dbeta are zero past them."""
    cols = int(gamma.numel())
    width = cols if width <= 0 else width
    yd = y.detach()[:, :width].double().requires_grad_(True)
    gd = gamma.detach()[:width].double().requires_grad_(True)
    bd = torch.zeros_like(gd).requires_grad_(True)
    with torch.enable_grad():  # (grad mode is off inside a Function's backward)
        out = torch.nn.functional.layer_norm(yd, (width,), gd, bd, 1e-5)
    out.backward(dn.detach()[:, :width].double())
    pad = lambda t: torch.nn.functional.pad(t, (0, cols - width))  # noqa: E731
    return pad(yd.grad), pad(gd.grad), pad(bd.grad)


class _Calls:
    def __init__(self):
        self.names = []


def install(monkeypatch) -> _Calls:
    calls = _Calls()

    def packed_t(mlp, layer, W, lo, hi):
        if getattr(mlp, "no_packs", False) or W.shape[0] != 256 or hi - lo != 256:  # (only 256 x 256 blocks have a packed stream)
            return None
        return W[:, lo:hi].detach().clone()  # "stream" of the block: d @ pt

    def chain_backward(d, chain, fan, ln=None, colsum=None, fan_add=None, gather=None):
        calls.names.append("chain" + ("+ln" if ln is not None else "") + ("+gather" if gather is not None else "")
                           + ("+colsum" if colsum is not None else ""))
        rows = d
        if gather is not None:
            idx, tab_rows, add = gather
            n = int(idx.numel())
            b = torch.arange(int(chain[0][2].shape[0]) // n).repeat_interleave(n)
            rows = d[b * tab_rows + idx.long().repeat(len(b) // n)]
            if add is not None:
                rows = rows + add
        cur = rows.double()
        if ln is not None:
            y, gamma, dgamma, dbeta, dy = ln
            gy, gg, gb = _ln_bwd64(rows, y, gamma)
            dgamma += gg.float()
            dbeta += gb.float()
            dy.copy_(gy.float())
            cur = gy
        for pt, mask, out in chain:
            cur = (cur @ pt.double()) * (mask > 0)
            out.copy_(cur.float())
        if colsum is not None:
            colsum += cur.sum(0).float()
        for i, (pt, out) in enumerate(fan):
            v = cur @ pt.double()
            extra = fan_add[i] if fan_add else None
            if extra is ag.FAN_ADD_INPUT:
                v = v + rows.double()
            elif extra is not None:
                v = v + extra.double()
            out.copy_(v.float())

    def gemm_tn_acc(a, b, c, c_col0=0, colsum=None, x3=False):
        calls.names.append("gemm" + ("+colsum" if colsum is not None else ""))
        c[:, c_col0:c_col0 + b.shape[1]] += (a.double().t() @ b.double()).float()
        if colsum is not None:
            colsum += a.double().sum(0).float()

    def layernorm_backward(dn, y, gamma, dgamma, dbeta, width=0):
        calls.names.append("ln_bwd")
        gy, gg, gb = _ln_bwd64(dn, y, gamma, width)
        dgamma += gg.float()
        dbeta += gb.float()
        return gy.float()

    def relu_backward(dh, h, db):
        calls.names.append("relu_bwd")
        if h is not None:
            dh.mul_((h > 0).float())
        if db is not None:
            db += dh.double().sum(0).float()
        return dh

    def input_grad(mlp, layer, d, W, lo, hi, relu_of=None):
        calls.names.append("single")
        out = (d.double() @ W[:, lo:hi].double()).float()
        return out * (relu_of > 0) if relu_of is not None else out

    def gather_rows(table, rows_pb, idx, batch, n_idx, add=None):
        calls.names.append("gather")
        assert table.shape[1] == 256 and table.stride(0) == 256  # (the kernel reads packed 256-float rows)
        b = torch.arange(batch).repeat_interleave(n_idx)
        k = torch.arange(n_idx).repeat(batch) if idx is None else idx.long().repeat(batch)
        out = table[b * rows_pb + k]
        return out + add if add is not None else out.clone()

    def segment_sum_rows(rows, rows_pb_in, batch, batch_out, n_seg, ptr, perm):
        """out[bo, s] = sum over the samples b that map to bo and k in [ptr[s], ptr[s + 1]) of rows[b * rows_pb_in + perm[k]]
        (perm None: k itself); batch_out is ``batch`` (one result per sample) or 1 (summed over the batch)."""
        calls.names.append("segsum")
        assert batch_out in (1, batch)
        n_in = int(ptr[-1])
        order = torch.arange(n_in) if perm is None else perm.long()
        seg = torch.repeat_interleave(torch.arange(n_seg), (ptr[1:] - ptr[:-1]).long())
        out = torch.zeros(batch, n_seg, rows.shape[1], dtype=torch.float64)
        picked = torch.stack([rows[b * rows_pb_in + order] for b in range(batch)]).double()
        out.index_add_(1, seg, picked)
        out = out.sum(0, keepdim=True) if batch_out == 1 else out
        return out.reshape(batch_out * n_seg, rows.shape[1]).float()

    for name, fn in (("_packed_transposed", packed_t), ("chain_backward", chain_backward), ("gemm_tn_acc", gemm_tn_acc),
                     ("layernorm_backward", layernorm_backward), ("relu_backward", relu_backward), ("input_grad", input_grad),
                     ("gather_rows", gather_rows), ("segment_sum_rows", segment_sum_rows)):
        monkeypatch.setattr(ag, name, fn)
    return calls
