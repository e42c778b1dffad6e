"""The training step bench.py times (``--mode train``, ``run_train_extra``) at its own size - 1 degree, batch 2, fp32 and bf16x3 -
against the oracle's fp64 autograd on the device.  As in the bench: FlatGradients, graph_weather_amd.AdamW(flat=...),
NormalizedMSELoss(normalize=False).  Unlike the bench, lr = 1e-2 (with 1e-4 the weights barely move, and a stale packed-weight
cache would go unnoticed).  Step 1 at the initial weights; the AdamW update against an fp64 restatement applied to the product's
own gradients; step 2 at the updated, re-packed weights (the state the bench times) against the oracle at those weights.

Bars are the 10 degree tests' (tests/test_gpu_round2.py, tests/test_gpu_split.py), for every tensor: none needed a wider one.
The oracle's own fp32 autograd is the conditioning yardstick: its error against fp64 is printed for every tensor where it
reaches a third of the bar (at 1 degree only encoder.h3_nodes, 1.2e-2 max-rel / 5.8e-4 l2, inside the bar), and reported
beside every miss."""
import gc
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import sharding as sh  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

from . import oracle_gpu  # noqa: E402

DEV = "cuda:0"
LR = 1e-2
BARS = {"fp32": (2e-2, 3e-3), "bf16x3": (2e-2, 6e-3)}  # (max-rel, l2-rel) per tensor
OWN_BARS = {"bf16x3": {"encoder.h3_nodes": (1.5e-1, 1.5e-2)}}  # tests/test_gpu_split.py
LOSS_REL = {"fp32": 1e-5, "bf16x3": 1e-4}
ADAMW_REL = 1e-6


def _rel(a, ref):
    a, ref = a.detach().double(), ref.detach().double().to(a.device)
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _l2(a, ref):
    a, ref = a.detach().double(), ref.detach().double().to(a.device)
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


_CACHE = {}


def _setup():
    lat_lons = regular_lat_lons(1.0)
    model = gw.GraphWeatherForecaster(lat_lons, resolution=2)  # bench.py run_train_extra: build_model(CONFIGS["c2"])
    deterministic_fill_(model, seed=0)
    G = len(lat_lons)
    feats = seeded_features(2, G, 102, seed=42)
    target = torch.randn(2, G, 78, generator=torch.Generator().manual_seed(1234))
    return model, lat_lons, feats, target


def _oracle_grads(params, g, feats, target, lat_lons, dtype):
    """Loss and gradients of the oracle at ``params`` in ``dtype`` (fp64 / fp32 autograd on the device); the autograd graph is
    freed before returning.  Returns (loss, {name: grad on the host, fp64}, peak GiB)."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    p = oracle_gpu.params_on(params, DEV, dtype, requires_grad=True)
    loss = oracle_gpu.loss(p, g, feats, target, lat_lons, DEV)
    loss.backward()
    grads = {k: v.grad.detach().double().cpu() for k, v in p.items()}
    value = loss.item()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2**30
    del p, loss
    gc.collect()
    torch.cuda.empty_cache()
    return value, grads, peak


def _oracle_step1():
    """Step 1 of the oracle (fp64, and fp32 as the conditioning yardstick) at the initial weights: shared by both precisions."""
    if "step1" not in _CACHE:
        model, lat_lons, feats, target = _setup()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        g = model.encoder.graphs.as_oracle_dict()
        t0 = time.perf_counter()
        l64, g64, peak64 = _oracle_grads(sd, g, feats, target, lat_lons, torch.float64)
        t1 = time.perf_counter()
        l32, g32, peak32 = _oracle_grads(sd, g, feats, target, lat_lons, torch.float32)
        t2 = time.perf_counter()
        print(f"[bench training] oracle step 1: fp64 loss {l64:.9e}, peak {peak64:.1f} GiB, {t1 - t0:.0f} s; fp32 loss {l32:.9e}, "
              f"peak {peak32:.1f} GiB, {t2 - t1:.0f} s")
        cond = {k: (_rel(g32[k], g64[k]), _l2(g32[k], g64[k])) for k in g64}
        _CACHE["step1"] = (l64, g64, cond, peak64)
    return _CACHE["step1"]


def _compare(step, precision, grads, ref, cond):
    """Every gradient against fp64 autograd at its bar; returns the failures and prints the worst case."""
    bad, worst = [], (0.0, 0.0, "")
    for k, gk in grads.items():
        mbar, lbar = OWN_BARS.get(precision, {}).get(k, BARS[precision])
        m, l = _rel(gk, ref[k]), _l2(gk, ref[k])
        om_, ol_ = cond[k]
        if m > mbar or l > lbar:
            bad.append((k, f"max-rel {m:.2e} (bar {mbar:.1e})", f"l2 {l:.2e} (bar {lbar:.1e})",
                        f"oracle fp32 {om_:.2e} / {ol_:.2e}"))
        if m / mbar > worst[0] / BARS[precision][0] and k not in OWN_BARS.get(precision, {}):
            worst = (m, l, k)
    print(f"[bench training {precision}] step {step}: worst max-rel {worst[0]:.2e} (l2 {worst[1]:.2e}, {worst[2]}) of bars "
          f"{BARS[precision][0]:.0e} / {BARS[precision][1]:.0e}; worst l2 {max(_l2(grads[k], ref[k]) for k in grads):.2e}")
    for k, (mb, lb) in OWN_BARS.get(precision, {}).items():
        print(f"    {k} (own bar {mb:.1e} / {lb:.1e}): {_rel(grads[k], ref[k]):.2e} / {_l2(grads[k], ref[k]):.2e}")
    return bad


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_bench_training_step_against_fp64_autograd(precision):
    assert torch.backends.cuda.matmul.allow_tf32 is False
    t_start = time.perf_counter()
    l64, ref1, cond, peak64 = _oracle_step1()
    cand = [(k, m, l) for k, (m, l) in cond.items()
            if m >= OWN_BARS.get(precision, {}).get(k, BARS[precision])[0] / 3 or l >= OWN_BARS.get(precision, {}).get(k, BARS[precision])[1] / 3]
    print(f"[bench training {precision}] oracle fp32 vs fp64 at a third of the bar or more: "
          + (", ".join(f"{k} ({m:.2e} / {l:.2e})" for k, m, l in cand) or "none"))

    model, lat_lons, feats, target = _setup()
    g = model.encoder.graphs.as_oracle_dict()
    model = model.to(DEV).train()
    if precision != "fp32":
        model.set_compute_dtype(gw.BF16X3)
    crit = gw.NormalizedMSELoss([1.0] * 78, lat_lons, normalize=False)
    flat = sh.FlatGradients(model.parameters())
    opt = gw.AdamW(model.parameters(), lr=LR, flat=flat)
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    assert len(names) == len(flat.params) == len(ref1) == 215
    fd, td = feats.to(DEV), target.to(DEV)

    def grads_through_flat():
        return {k: flat.grad[o:o + p.numel()].view_as(p).detach().clone() for k, p, o in zip(names, flat.params, flat.offsets)}

    def step():
        flat.zero_()
        loss = crit(model(fd), td)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item()

    # ---- step 1: initial weights
    torch.cuda.reset_peak_memory_stats()
    loss1 = step()
    grads1 = grads_through_flat()
    peak_product = torch.cuda.max_memory_allocated() / 2**30
    e_loss1 = abs(loss1 - l64) / abs(l64)
    print(f"[bench training {precision}] step 1: loss {loss1:.9e} vs fp64 {l64:.9e}: rel {e_loss1:.2e} (bar {LOSS_REL[precision]:.0e}); "
          f"product peak {peak_product:.1f} GiB, oracle fp64 peak {peak64:.1f} GiB")
    assert e_loss1 <= LOSS_REL[precision]
    bad1 = _compare(1, precision, grads1, ref1, cond)

    # ---- AdamW: against an fp64 restatement of torch.optim.AdamW's first step on the product's own gradients
    before = {k: p.detach().double().clone() for k, p in zip(names, flat.params)}
    opt.step()
    torch.cuda.synchronize()
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 1e-2
    e_adam = 0.0
    for k, p in zip(names, flat.params):
        gk = grads1[k].double()
        m_, v_ = (1 - b1) * gk, (1 - b2) * gk * gk
        ref_p = before[k] * (1 - LR * wd) - (LR / (1 - b1)) * m_ / (v_.sqrt() / np.sqrt(1 - b2) + eps)
        e_adam = max(e_adam, _rel(p, ref_p))
    moved = max(_rel(p, before[k]) for k, p in zip(names, flat.params))
    print(f"[bench training {precision}] AdamW step (lr {LR:g}): max-rel vs fp64 restatement {e_adam:.2e} (bar {ADAMW_REL:.0e}); "
          f"largest relative weight change {moved:.2e}")
    assert e_adam <= ADAMW_REL

    # ---- step 2: the updated weights, re-packed by the kernels' caches - the state the bench times
    loss2 = step()
    grads2 = grads_through_flat()
    params2 = {k: p.detach().clone() for k, p in zip(names, flat.params)}
    sd2 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd2.update(params2)  # (the product's fp32 weights after the step)
    del model, flat, opt, crit, fd, td
    gc.collect()
    torch.cuda.empty_cache()
    l64_2, ref2, peak64_2 = _oracle_grads(sd2, g, feats, target, lat_lons, torch.float64)
    e_loss2 = abs(loss2 - l64_2) / abs(l64_2)
    print(f"[bench training {precision}] step 2: loss {loss2:.9e} vs fp64 {l64_2:.9e}: rel {e_loss2:.2e}; loss moved by "
          f"{abs(l64_2 - l64) / abs(l64):.2e}")
    assert e_loss2 <= LOSS_REL[precision]
    # the test can tell the steps apart: the oracle's step-2 gradients differ from its step-1 gradients by far more than the bar
    apart = sum(_l2(ref2[k], ref1[k]) >= 10 * BARS[precision][1] for k in ref1)
    print(f"[bench training {precision}] oracle gradients, step 2 vs step 1: {apart} of {len(ref1)} tensors differ by >= 10x the "
          f"l2 bar")
    assert apart >= 0.8 * len(ref1)
    bad2 = _compare(2, precision, grads2, ref2, cond)
    print(f"[bench training {precision}] wall time {time.perf_counter() - t_start:.0f} s")
    assert not bad1, bad1[:8]
    assert not bad2, bad2[:8]
