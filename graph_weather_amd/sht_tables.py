"""Host tables of the real spherical-harmonic transform behind ``AMSENormalizedLoss`` (numpy, float64).

The transform is ``torch_harmonics.RealSHT(nlat, nlon, grid="equiangular")`` with its defaults: ``lmax = nlat``,
``mmax = min(lmax, nlon // 2 + 1)``, orthonormal harmonics, Clenshaw-Curtis latitudes ``theta_k = pi k / (nlat - 1)`` with
both poles.  Everything here is computed in float64 and rounded to float32 only by ``device_tables``.

What a shape costs on the device: the cos / -sin matrix is ``2 * ceil(mmax / 64) * 64 * nlon`` floats and the Legendre
table, packed triangularly (degrees ``l < m`` are not stored), ``sum_m (lmax - m) * nlat`` floats - 0.55 MB + 11.7 MB at
1 degree (180 x 360), 8.8 MB + 747 MB at 0.25 degree (720 x 1440; 1.5 GB dense).
"""
from __future__ import annotations

import numpy as np

TILE = 64  # row padding of the cos and sin halves of the device matrix (csrc/gw_sht.hip: a tile is all cos or all sin)


def mmax_of(nlat: int, nlon: int) -> int:
    return min(nlat, nlon // 2 + 1)


def colatitudes(nlat: int) -> np.ndarray:
    return np.pi * np.arange(nlat, dtype=np.float64) / (nlat - 1)


def clenshaw_curtis_weights(nlat: int) -> np.ndarray:
    """Weights of the Clenshaw-Curtis rule on [-1, 1] at ``x_k = cos(pi k / (nlat - 1))`` (exact up to degree nlat - 1)."""
    if nlat < 2:
        raise ValueError("nlat must be at least 2")
    n = nlat - 1
    k = np.arange(nlat, dtype=np.float64)
    w = np.ones(nlat, dtype=np.float64)
    for j in range(1, n // 2 + 1):
        b = 1.0 if 2 * j == n else 2.0
        w -= b / (4.0 * j * j - 1.0) * np.cos(2.0 * j * k * np.pi / n)
    c = np.full(nlat, 2.0)
    c[0] = c[-1] = 1.0
    return c * w / n


def legendre_orders(nlat: int, nlon: int):
    """Yields ``(m, P_m)`` with ``P_m[l - m, k] = Pbar_l^m(cos theta_k)`` for ``l = m .. lmax - 1``: normalised so that
    ``Pbar_l^m(cos theta) e^{i m phi}`` has unit L2 norm on the sphere, with the Condon-Shortley sign.  The usual three-term
    recurrence in l, started from the closed form of ``Pbar_m^m``."""
    lmax, mmax = nlat, mmax_of(nlat, nlon)
    theta = colatitudes(nlat)
    x, s = np.cos(theta), np.sin(theta)
    s[0] = s[-1] = 0.0  # sin(pi) is 1.2e-16 in floating point; the poles carry only m = 0
    pmm = np.full(nlat, 1.0 / np.sqrt(4.0 * np.pi))
    for m in range(mmax):
        if m > 0:
            pmm = -np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * pmm
        p = np.zeros((lmax - m, nlat), dtype=np.float64)
        p[0] = pmm
        if m + 1 < lmax:
            p[1] = np.sqrt(2.0 * m + 3.0) * x * pmm
        for l in range(m + 2, lmax):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            p[l - m] = a * (x * p[l - m - 1] - b * p[l - m - 2])
        yield m, p


def legendre_table(nlat: int, nlon: int) -> np.ndarray:
    """Dense ``P[m, l, k] = Pbar_l^m(cos theta_k)`` ([mmax, lmax, nlat], zero for l < m)."""
    p = np.zeros((mmax_of(nlat, nlon), nlat, nlat), dtype=np.float64)
    for m, pm in legendre_orders(nlat, nlon):
        p[m, m:] = pm
    return p


def latitude_table(nlat: int, nlon: int) -> np.ndarray:
    """Dense ``T[m, l, k] = Pbar_l^m(cos theta_k) * w_k``."""
    return legendre_table(nlat, nlon) * clenshaw_curtis_weights(nlat)[None, None, :]


def packed_latitude_table(nlat: int, nlon: int, dtype=np.float32) -> np.ndarray:
    """``latitude_table`` packed triangularly, built order by order (the dense table is never formed)."""
    w = clenshaw_curtis_weights(nlat)
    out = np.empty(triangular_offset(mmax_of(nlat, nlon), nlat, nlat), dtype=dtype)
    for m, pm in legendre_orders(nlat, nlon):
        o = triangular_offset(m, nlat, nlat)
        out[o:o + pm.size] = (pm * w[None, :]).reshape(-1)
    return out


def triangular_offset(m: int, lmax: int, nlat: int) -> int:
    return (m * lmax - m * (m - 1) // 2) * nlat


def pack_triangular(t: np.ndarray) -> np.ndarray:
    """Rows ``l >= m`` of every order of a dense [mmax, lmax, nlat] table, one after the other."""
    mmax, lmax, nlat = t.shape
    out = np.empty(triangular_offset(mmax, lmax, nlat), dtype=t.dtype)
    for m in range(mmax):
        o = triangular_offset(m, lmax, nlat)
        out[o:o + (lmax - m) * nlat] = t[m, m:].reshape(-1)
    return out


def unpack_triangular(packed: np.ndarray, mmax: int, lmax: int, nlat: int) -> np.ndarray:
    t = np.zeros((mmax, lmax, nlat), dtype=packed.dtype)
    for m in range(mmax):
        o = triangular_offset(m, lmax, nlat)
        t[m, m:] = packed[o:o + (lmax - m) * nlat].reshape(lmax - m, nlat)
    return t


def dft_matrix(nlon: int, mmax: int) -> np.ndarray:
    """``D`` [nlon, 2 * mmax]: ``x @ D`` = (real parts, imaginary parts) of ``2 pi * rfft(x, norm="forward")[:mmax]``."""
    # the phase is reduced in integers first: 2 pi (m j mod nlon) / nlon keeps the argument below 2 pi
    ang = 2.0 * np.pi * np.mod(np.arange(nlon)[:, None] * np.arange(mmax)[None, :], nlon).astype(np.float64) / nlon
    f = 2.0 * np.pi / nlon
    return np.concatenate([f * np.cos(ang), -f * np.sin(ang)], axis=1)


def table_bytes(nlat: int, nlon: int) -> int:
    mmax = mmax_of(nlat, nlon)
    rows = 2 * ((mmax + TILE - 1) // TILE) * TILE
    return 4 * (rows * nlon + triangular_offset(mmax, nlat, nlat))


def device_tables(nlat: int, nlon: int):
    """(dft [2 * Mp, nlon], legendre [packed]) as float32 numpy arrays in the layout ``gw_amse_forward`` reads."""
    mmax = mmax_of(nlat, nlon)
    mp = ((mmax + TILE - 1) // TILE) * TILE
    d = dft_matrix(nlon, mmax)
    dft = np.zeros((2 * mp, nlon), dtype=np.float32)
    dft[:mmax] = d[:, :mmax].T
    dft[mp:mp + mmax] = d[:, mmax:].T
    return dft, packed_latitude_table(nlat, nlon)


# ---------------------------------------------------------------------------------------------------------------------
# The inverse transform behind GenCast's generate_isotropic_noise: torch_harmonics.InverseRealSHT(nlat, nlon, lmax, mmax = lmax + 1,
# grid="equiangular").  Unweighted Legendre functions for l < lmax and the irfft(norm="forward") matrix.
# ---------------------------------------------------------------------------------------------------------------------
def isht_lmax(nlat: int, nlon: int) -> int:
    """lmax of the two grids the reference's ``generate_isotropic_noise`` accepts; 0 for any other shape."""
    if nlat < 2 or nlon < 2:
        return 0
    if nlon == 2 * nlat:
        return nlat
    if nlon == 2 * (nlat - 1):
        return nlat - 1
    return 0


def isht_packed_legendre_table(nlat: int, nlon: int, dtype=np.float32) -> np.ndarray:
    """``Pbar_l^m(cos theta_k)`` for ``m <= l < lmax``, packed triangularly order by order (``triangular_offset(m, lmax, nlat)``).
    The last order ``m = lmax`` of ``mmax = lmax + 1`` has no degree below lmax and takes no room."""
    lmax = isht_lmax(nlat, nlon)
    if not lmax:
        raise ValueError("the inverse transform needs nlon = 2 nlat or nlon = 2 (nlat - 1), got %d x %d" % (nlon, nlat))
    out = np.empty(triangular_offset(lmax + 1, lmax, nlat), dtype=dtype)
    # legendre_orders yields l < nlat for m < min(nlat, nlon // 2 + 1): every order below lmax, with at least lmax - m rows
    for m, pm in legendre_orders(nlat, nlon):
        if m >= lmax:
            break
        o = triangular_offset(m, lmax, nlat)
        out[o:o + (lmax - m) * nlat] = pm[:lmax - m].reshape(-1)
    return out


def synthesis_matrix(nlon: int, mmax: int) -> np.ndarray:
    """``S`` [2 * mmax, nlon]: ``irfft(G, n=nlon, norm="forward") = G.real @ S[:mmax] + G.imag @ S[mmax:]`` for ``G`` of
    ``mmax <= nlon // 2 + 1`` orders - ``w_m cos(2 pi m j / nlon)`` and ``-w_m sin(...)``, ``w_0 = w_{nlon/2} = 1``, else 2.  The
    sine rows of m = 0 and m = nlon / 2 are exactly zero: irfft ignores those imaginary parts."""
    m = np.arange(mmax)
    # the phase is reduced in integers first, as in dft_matrix
    ang = 2.0 * np.pi * np.mod(m[:, None] * np.arange(nlon)[None, :], nlon).astype(np.float64) / nlon
    w = np.where((m == 0) | (2 * m == nlon), 1.0, 2.0)[:, None]
    sin = -w * np.sin(ang)
    sin[(m == 0) | (2 * m == nlon)] = 0.0
    return np.concatenate([w * np.cos(ang), sin], axis=0)


def isht_table_bytes(nlat: int, nlon: int) -> int:
    lmax = isht_lmax(nlat, nlon)
    rows = 2 * ((lmax + 1 + TILE - 1) // TILE) * TILE
    return 4 * (rows * nlon + triangular_offset(lmax + 1, lmax, nlat))


def isht_device_tables(nlat: int, nlon: int):
    """(synthesis [2 * Mp, nlon], legendre [packed]) as float32 numpy arrays in the layout ``gw_isht_forward`` reads."""
    mmax = isht_lmax(nlat, nlon) + 1
    mp = ((mmax + TILE - 1) // TILE) * TILE
    s = synthesis_matrix(nlon, mmax)
    syn = np.zeros((2 * mp, nlon), dtype=np.float32)
    syn[:mmax] = s[:mmax]
    syn[mp:mp + mmax] = s[mmax:]
    return syn, isht_packed_legendre_table(nlat, nlon)
