"""Plain-torch restatements, parameterised by dtype, of what GenCast's Sampler and loss need: the inverse spherical-harmonic transform
``torch_harmonics.InverseRealSHT(nlat, nlon, lmax, mmax, grid="equiangular")``, ``generate_isotropic_noise`` from given coefficients
(utils/noise.py), ``Sampler.sample`` (sampler.py) over ``gencast_model_oracle.denoiser_forward`` with a supplied list of coefficient
draws, and ``WeightedMSELoss`` (weighted_mse_loss.py).  Touches no product code.

The Legendre functions come from ``sht_oracle.legendre`` (the fully normalised recurrences, derived apart from the product's
``sht_tables``), always built in float64 and rounded to ``dtype`` once; the longitude synthesis is ``torch.fft.irfft``.  With
``dtype=torch.float32`` a function is the yardstick of the GPU tests: the same algorithm in the reference's precision.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import gencast_model_oracle as mo
from . import sht_oracle


# ---- the inverse transform ---------------------------------------------------------------------------------------------------
def lmax_of(num_lat: int, num_lon: int) -> int:
    """utils/noise.py: lmax = num_lat on a 2N x N grid, num_lat - 1 on a 2N x (N + 1) grid; anything else raises there."""
    if 2 * num_lat == num_lon:
        return num_lat
    if 2 * (num_lat - 1) == num_lon:
        return num_lat - 1
    raise ValueError("grid %d x %d" % (num_lon, num_lat))


def inverse_legendre(nlat: int, nlon: int) -> torch.Tensor:
    """[mmax = lmax + 1, lmax, nlat] float64 ``Pbar_l^m(cos theta_k)``, zero for m > l: no quadrature weights in the inverse."""
    lmax = lmax_of(nlat, nlon)
    p = sht_oracle.legendre(nlat, nlon)  # [min(nlat, nlon // 2 + 1), nlat, nlat]
    out = torch.zeros(lmax + 1, lmax, nlat, dtype=torch.float64)
    m = min(p.shape[0], lmax + 1)
    out[:m] = p[:m, :lmax]
    return out


def isht(coeffs: torch.Tensor, nlat: int, nlon: int, dtype=torch.float64) -> torch.Tensor:
    """complex [..., lmax, mmax] -> real [..., nlat, nlon] in ``dtype``: the Legendre sum for the real and the imaginary parts apart,
    then ``irfft(n=nlon, norm="forward")``, as torch_harmonics' InverseRealSHT.forward."""
    pct = inverse_legendre(nlat, nlon).to(dtype)
    x = torch.view_as_real(coeffs.to(torch.complex64 if dtype == torch.float32 else torch.complex128))
    rl = torch.einsum("...lm,mlk->...km", x[..., 0], pct)
    im = torch.einsum("...lm,mlk->...km", x[..., 1], pct)
    g = torch.view_as_complex(torch.stack((rl, im), -1).contiguous())
    return torch.fft.irfft(g, n=nlon, dim=-1, norm="forward")


def isotropic_noise(coeffs: torch.Tensor, num_lon: int, num_lat: int, dtype=torch.float64) -> torch.Tensor:
    """utils/noise.py from the unscaled complex draws [samples, lmax, mmax] -> [lon, lat, samples]."""
    c = coeffs.to(torch.complex64 if dtype == torch.float32 else torch.complex128) / np.sqrt((num_lat ** 2) // 2)
    noise = isht(c, num_lat, num_lon, dtype) * np.sqrt(2 * np.pi)
    return noise.permute(2, 1, 0).contiguous()  # "b lat lon -> lon lat b"


def noise_variance(num_lon: int, num_lat: int) -> torch.Tensor:
    """[lon, lat] float64: the exact variance of isotropic noise at every grid point.  The noise is linear in the real and the
    imaginary parts of the coefficients, each an independent normal of variance 1/2 (a complex64 standard normal), so the variance
    is the sum over those degrees of freedom of the squared response to a unit coefficient, halved."""
    lmax = lmax_of(num_lat, num_lon)
    mmax = lmax + 1
    n = lmax * mmax
    basis = torch.zeros(2 * n, lmax, mmax, dtype=torch.complex128)
    flat = basis.view(2 * n, n)
    flat[torch.arange(n), torch.arange(n)] = 1.0
    flat[n + torch.arange(n), torch.arange(n)] = 1.0j
    cols = isotropic_noise(basis, num_lon, num_lat, torch.float64)  # [lon, lat, 2 n]
    return 0.5 * (cols ** 2).sum(-1)


# ---- the sampler -------------------------------------------------------------------------------------------------------------
SAMPLER_DEFAULTS = dict(S_noise=1.05, S_tmin=0.75, S_tmax=80.0, S_churn=2.5, r=0.5, sigma_max=80.0, sigma_min=0.03, rho=7, num_steps=20)


def schedule(**kw):
    """(sigmas float32 tensor, gammas list) as sampler.py forms them with float32 tensors on the CPU."""
    k = dict(SAMPLER_DEFAULTS, **kw)
    u = torch.arange(0, k["num_steps"]) / (k["num_steps"] - 1)
    sigmas = (k["sigma_max"] ** (1 / k["rho"]) + u * (k["sigma_min"] ** (1 / k["rho"]) - k["sigma_max"] ** (1 / k["rho"]))) ** k["rho"]
    gammas = [min(k["S_churn"] / k["num_steps"], math.sqrt(2) - 1) if k["S_tmin"] <= sigmas[i] <= k["S_tmax"] else 0.0
              for i in range(len(sigmas) - 1)]
    return sigmas, gammas


def sampler_sample(denoise, prev_inputs: torch.Tensor, draws, num_lon: int, num_lat: int, dtype=torch.float64, **kw) -> torch.Tensor:
    """Sampler.sample for one sample: ``denoise(x, prev_inputs, noise_levels)`` the Denoiser in ``dtype``, ``draws`` the unscaled
    coefficient draws [out, lmax, mmax] in the order the reference makes them.  The schedule (the float32 sigmas and the churn
    decisions taken on them) is the reference's CPU one in every dtype; the rest of the arithmetic runs in ``dtype``."""
    k = dict(SAMPLER_DEFAULTS, **kw)
    sig32, gammas = schedule(**kw)
    sigmas = sig32.to(dtype)
    draws = iter(draws)
    ones = torch.ones(1, 1, dtype=dtype)
    prev_inputs = prev_inputs.to(dtype)
    x = sigmas[0] * isotropic_noise(next(draws), num_lon, num_lat, dtype).unsqueeze(0)
    for i in range(len(sigmas) - 1):
        gamma = gammas[i]
        noise = (k["S_noise"] * isotropic_noise(next(draws), num_lon, num_lat, dtype)).unsqueeze(0)
        sigma_hat = sigmas[i] * (gamma + 1)
        if gamma > 0:
            x = x + (sigma_hat ** 2 - sigmas[i] ** 2) ** 0.5 * noise
        denoised = denoise(x, prev_inputs, sigma_hat * ones)
        if i == len(sigmas) - 2:
            d = (x - denoised) / sigma_hat
            x = x + d * (sigmas[i + 1] - sigma_hat)
        else:
            lambda_hat = -torch.log(sigma_hat)
            lambda_next = -torch.log(sigmas[i + 1])
            h = lambda_next - lambda_hat
            lambda_mid = lambda_hat + k["r"] * h
            sigma_mid = torch.exp(-lambda_mid)
            u = sigma_mid / sigma_hat * x - (torch.exp(-k["r"] * h) - 1) * denoised
            denoised_2 = denoise(u, prev_inputs, sigma_mid * ones)
            D = (1 - 1 / (2 * k["r"])) * denoised + 1 / (2 * k["r"]) * denoised_2
            x = sigmas[i + 1] / sigma_hat * x - (torch.exp(-h) - 1) * D
    return x


def denoiser_fn(p, kw, graphs):
    """``denoise`` of ``sampler_sample`` over ``gencast_model_oracle.denoiser_forward`` (parameters and float tables of one dtype)."""
    return lambda x, prev, sigma: mo.denoiser_forward(p, kw, graphs, x, prev, sigma)


SAMPLER_CASE = "gencast_model_b"  # the Denoiser of the sampler fixture: 16 x 9 grid, 5 output features, weights by seed
SAMPLER_SEED = 71  # torch.manual_seed before the reference's Sampler.sample
SAMPLER_KW = dict(num_steps=5)


def sampler_prev_inputs() -> torch.Tensor:
    return mo.case_inputs(SAMPLER_CASE, batch=1)[1]


# ---- the loss ----------------------------------------------------------------------------------------------------------------
def loss_weights(grid_lat=None, pressure_levels=None, num_atmospheric_features=None, single_features_weights=None, dtype=torch.float64):
    """(area_weights, features_weights) as WeightedMSELoss.__init__ forms them, in ``dtype``."""
    aw = fw = None
    if grid_lat is not None:
        aw = torch.abs(torch.cos(grid_lat.to(dtype) * np.pi / 180.0))
        aw = aw / torch.mean(aw)
    if pressure_levels is not None:
        pw = pressure_levels.to(dtype) / torch.sum(pressure_levels.to(dtype))
        fw = torch.cat((pw.repeat(num_atmospheric_features), single_features_weights.to(dtype)), dim=-1)
    return aw, fw


def weighted_mse_loss(pred, noise_level, target, aw=None, fw=None, dtype=torch.float64, sigma_data=1):
    """WeightedMSELoss.forward in ``dtype`` (differentiable)."""
    loss = (pred.to(dtype) - target.to(dtype)) ** 2
    if aw is not None:
        loss = loss * aw.to(dtype)[None, None, :, None]
    if fw is not None:
        loss = loss * fw.to(dtype)[None, None, None, :]
    loss = loss.flatten(1).mean(-1)
    s = noise_level.to(dtype)
    loss = loss * ((s ** 2 + sigma_data ** 2) / (s * sigma_data) ** 2).flatten()
    return loss.mean()


# name -> ((B, lon, lat, var), area weights, (pressure levels, atmospheric features, single weights) or None, seed)
LOSS_CASES = {
    "all_weights": ((2, 12, 7, 5), True, ([50.0, 500.0], 2, [1.0]), 81),
    "area_only": ((3, 16, 9, 83), True, None, 82),
    "features_only": ((2, 64, 33, 7), False, ([100.0, 500.0, 850.0], 2, [0.1]), 83),
    "no_weights": ((1, 8, 4, 1), False, None, 84),
}


def loss_case(name: str):
    """(constructor keywords of WeightedMSELoss, pred, noise_level, target) float32 from the case's seed."""
    shape, area, feats, seed = LOSS_CASES[name]
    rs = np.random.RandomState(seed)
    pred = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    target = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    sigma = torch.from_numpy(np.exp(rs.uniform(np.log(0.02), np.log(88.0), (shape[0], 1))).astype(np.float32))
    kw = {}
    if area:
        kw["grid_lat"] = torch.linspace(-80.0, 80.0, shape[2]) + 1.5
    if feats is not None:
        kw.update(pressure_levels=torch.tensor(feats[0]), num_atmospheric_features=feats[1], single_features_weights=torch.tensor(feats[2]))
    return kw, pred, sigma, target
