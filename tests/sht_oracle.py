"""fp64 restatement of the reference's ``AMSENormalizedLoss`` (graph_weather/models/losses.py:98-195) in torch, with the
spherical-harmonic transform ``torch_harmonics.RealSHT(nlat, nlon, grid="equiangular")`` written out: a forward-normalised
real FFT along longitude times 2 pi, then the quadrature against orthonormal associated Legendre functions at the
Clenshaw-Curtis latitudes.  Everything is differentiable torch, so autograd gives the oracle gradient.

The tables here are derived on their own, not imported from the product: the weights from the integrals of the Chebyshev
polynomials of the interpolant through the nodes, the Legendre functions from the fully normalised recurrences.

``amse_loss(..., dtype=torch.float32)`` is the yardstick of the tests: the same algorithm in the reference's precision
(float64-built tables rounded to float32, ``torch.fft.rfft`` and ``einsum`` in float32), which is what torch_harmonics runs.
"""
from __future__ import annotations

import math
from functools import lru_cache

import torch


def mmax_of(nlat: int, nlon: int) -> int:
    return min(nlat, nlon // 2 + 1)


def nodes(nlat: int) -> torch.Tensor:
    return math.pi * torch.arange(nlat, dtype=torch.float64) / (nlat - 1)


def quadrature_weights(nlat: int) -> torch.Tensor:
    """Clenshaw-Curtis weights from the integrals of the Chebyshev polynomials: the interpolant through the nodes is
    sum_j c_j T_j(x) with c = the type-I cosine transform of the samples, and int_{-1}^{1} T_j = 2 / (1 - j^2) for even j,
    0 for odd j.  Transposing that map gives the weight of each sample."""
    n = nlat - 1
    k = torch.arange(nlat, dtype=torch.float64)
    j = torch.arange(0, n + 1, 2, dtype=torch.float64)  # even Chebyshev degrees
    integ = 2.0 / (1.0 - j * j)
    # c_j = (2 / n) * sum''_k f_k cos(pi j k / n), halved again at j = 0 and j = n
    cj_scale = torch.full_like(j, 2.0 / n)
    cj_scale[0] *= 0.5
    if n % 2 == 0:
        cj_scale[-1] *= 0.5
    cosmat = torch.cos(math.pi * j[:, None] * k[None, :] / n)
    w = (integ * cj_scale) @ cosmat
    w[0] *= 0.5
    w[-1] *= 0.5
    return w


@lru_cache(maxsize=16)
def legendre(nlat: int, nlon: int) -> torch.Tensor:
    """[mmax, lmax, nlat] orthonormal Pbar_l^m(cos theta_k), zero for l < m, with the Condon-Shortley sign (-1)^m that
    torch_harmonics applies by default (it cancels in the loss, not in the coefficients).  Built in the fully
    normalised form by the standard recurrences
        Pbar_m^m     = -sqrt((2m + 1) / (2m)) * sin(theta) * Pbar_{m-1}^{m-1}
        Pbar_{m+1}^m = sqrt(2m + 3) * cos(theta) * Pbar_m^m
        Pbar_l^m     = sqrt((2l+1)/((l-m)(l+m))) * (sqrt(2l-1) x Pbar_{l-1}^m - sqrt((l+m-1)(l-m-1)/(2l-3)) Pbar_{l-2}^m)"""
    lmax, mmax = nlat, mmax_of(nlat, nlon)
    th = nodes(nlat)
    x, s = torch.cos(th), torch.sin(th)
    s[0] = 0.0
    s[-1] = 0.0
    out = torch.zeros(mmax, lmax, nlat, dtype=torch.float64)
    diag = torch.full((nlat,), math.sqrt(1.0 / (4.0 * math.pi)), dtype=torch.float64)
    for m in range(mmax):
        if m:
            diag = -math.sqrt((2 * m + 1) / (2 * m)) * s * diag
        out[m, m] = diag
        if m + 1 < lmax:
            out[m, m + 1] = math.sqrt(2 * m + 3) * x * diag
        for l in range(m + 2, lmax):
            f = math.sqrt((2 * l + 1) / ((l - m) * (l + m)))
            g = math.sqrt((l + m - 1) * (l - m - 1) / (2 * l - 3))
            out[m, l] = f * (math.sqrt(2 * l - 1) * x * out[m, l - 1] - g * out[m, l - 2])
    return out


@lru_cache(maxsize=16)
def weights_table(nlat: int, nlon: int) -> torch.Tensor:
    return legendre(nlat, nlon) * quadrature_weights(nlat)[None, None, :]


def sht(x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[..., nlat, nlon] real -> [..., lmax, mmax] complex, computed in ``dtype`` (tables always built in float64)."""
    nlat, nlon = x.shape[-2:]
    mmax = mmax_of(nlat, nlon)
    t = weights_table(nlat, nlon).to(device=x.device, dtype=dtype)
    f = 2.0 * math.pi * torch.fft.rfft(x.to(dtype), dim=-1, norm="forward")[..., :mmax]
    fr = torch.view_as_real(f)
    out = torch.einsum("...kmr,mlk->...lmr", fr, t).contiguous()
    return torch.view_as_complex(out)


def amse_terms(pc: torch.Tensor, tc: torch.Tensor, eps: float) -> torch.Tensor:
    """losses.py:169-188 on coefficients [..., l, m] -> per-field spectral loss [...]."""
    pp = (pc.abs() ** 2).sum(-1)
    tt = (tc.abs() ** 2).sum(-1)
    num = (pc * tc.conj()).real.sum(-1)
    den = torch.sqrt(pp * tt)
    coh = num / (den + eps)
    amp = (torch.sqrt(pp + eps) - torch.sqrt(tt + eps)) ** 2
    dec = 2.0 * den * (1.0 - coh)
    return (amp + dec).sum(-1)


def amse_loss(pred: torch.Tensor, target: torch.Tensor, variance: torch.Tensor, eps: float = 1e-9, dtype=torch.float64) -> torch.Tensor:
    b, c, h, w = pred.shape
    pc = sht(pred.reshape(b * c, h, w), dtype)
    tc = sht(target.reshape(b * c, h, w), dtype)
    per = amse_terms(pc, tc, eps).reshape(b, c)
    return (per / (variance.to(device=pred.device, dtype=dtype) + eps)).mean()


def amse_loss_chunked(pred, target, variance, eps: float = 1e-9, dtype=torch.float64, chunk: int = 6, grad: bool = False):
    """The same loss with the fields transformed ``chunk`` at a time (the 1 degree shape in float64).  With ``grad`` also the
    gradient with respect to ``pred``, accumulated chunk by chunk."""
    b, c, h, w = pred.shape
    n = b * c
    p = pred.reshape(n, h, w)
    t = target.reshape(n, h, w)
    inv = 1.0 / (variance.to(device=pred.device, dtype=dtype).reshape(-1) + eps)
    total = torch.zeros((), dtype=dtype, device=pred.device)
    g = torch.zeros(n, h, w, dtype=dtype, device=pred.device) if grad else None
    for i in range(0, n, chunk):
        pi = p[i:i + chunk].detach().to(dtype).requires_grad_(grad)
        per = amse_terms(sht(pi, dtype), sht(t[i:i + chunk], dtype), eps)
        idx = torch.arange(i, min(i + chunk, n), device=pred.device) % c
        part = (per * inv[idx]).sum() / n
        if grad:
            g[i:i + chunk] = torch.autograd.grad(part, pi)[0]
        total = total + part.detach()
    return (total, g.reshape(b, c, h, w)) if grad else total
