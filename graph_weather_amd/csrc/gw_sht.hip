// gw_sht.hip - AMSENormalizedLoss (graph_weather/models/losses.py:98-195): the real spherical-harmonic transform of
// torch_harmonics.RealSHT(nlat, nlon, grid="equiangular") as two dense products on v_mfma_f32_16x16x4_f32 (exact fp32), the
// loss epilogue fused into the second one, and the adjoint pair for the gradient of the prediction.
//
//   lon_fwd_kernel    F[c, m, q] = sum_j D[c, m, j] * x[q, j]: rows q = (field, latitude) of prediction and target against the
//                     cos / -sin matrix (2 pi / nlon folded in).  cos is even and sin odd about j = nlon / 2, so the product
//                     runs on x[j] +- x[nlon - j] with K = nlon / 2 + 1.  F is written m-major, the layout lat_fwd reads.
//   lat_fwd_kernel    per order m: a[l, n] = sum_k T[m, l, k] * F[c, m, n, k] for the four operands (re / im of prediction and
//                     target) of 16 fields x 64 degrees, then pp += |a|^2, tt += |b|^2, num += Re(a conj b) in registers.
//                     Tiles with l < m are skipped; the coefficients reach memory only when a gradient is wanted.  The orders
//                     are dealt round-robin over gridDim.z workgroups whose partial sums go to the workspace.
//   terms_kernel      per (l, n): the partials summed in split order and the loss term and its two derivatives in fp64
//   field_kernel      per field: the terms summed over l in one fixed order, divided by the variance (fp64)
//   final_kernel      one workgroup: fixed-shape tree over the fields
//   lat_bwd_kernel    dF[c, m, n, k] = sum_{l >= m} da_c[l, n] * T[m, l, k], da = dloss * (2 g_pp a + g_num b) formed on load
//   lon_bwd_kernel    dx[q, j] = sum_{c, m} dF[c, m, q] * D[c, m, j], folded: the cos and sin halves accumulate apart and
//                     j and nlon - j are written as their sum and difference
// No float atomics; every sum has one fixed order, so equal inputs give bitwise equal results.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_internal.hpp"

using namespace gw;

namespace {

typedef float sh_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;  // workgroup tile (64 x 64, four waves)
constexpr int kStep = 16;  // K per LDS stage
constexpr int kLd = kStep + 1;

int fail(const char* msg) { return set_error(GW_E_BADARG, msg); }

struct Geom {
  int N, C, H, W;  // fields per tensor, channels, nlat, nlon
  int L, M, Mp, Kf;  // lmax, mmax, mmax rounded up to the tile, folded longitude count nlon / 2 + 1
};

__host__ __device__ inline int64_t tri_off(int m, int L, int H) {  // first float of order m in the packed Legendre table
  return ((int64_t)m * L - (int64_t)m * (m - 1) / 2) * H;
}

// One 64 x 64 x [k0, k1) product step of the workgroup.  la(row, k) / lb(col, k) return the operand values (0 outside the
// problem).  *_KFAST: consecutive threads walk k (the operand is contiguous along k), else they walk the row / column.  The
// next stage's global loads are issued before the current stage's MFMAs.  Wave w owns 16 * WR rows x 16 * WC columns.
template <int WR, int WC, bool A_KFAST, bool B_KFAST, class LA, class LB>
__device__ inline void tile_product(sh_f32x4 (&acc)[WR][WC], int k0, int k1, LA la, LB lb, float* As, float* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWavesM = 4 / WR;
  const int wm = (wave % kWavesM) * 16 * WR, wn = (wave / kWavesM) * 16 * WC;
  const int ar = A_KFAST ? (tid >> 4) : (tid & 63), ak = A_KFAST ? (tid & 15) : (tid >> 6);
  const int br = B_KFAST ? (tid >> 4) : (tid & 63), bk = B_KFAST ? (tid & 15) : (tid >> 6);
  float ra[4], rb[4];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = A_KFAST ? la(ar + 16 * i, kb + ak) : la(ar, kb + ak + 4 * i);
      rb[i] = B_KFAST ? lb(br + 16 * i, kb + bk) : lb(br, kb + bk + 4 * i);
    }
  };
  if (k0 < k1) fetch(k0);
  for (int kb = k0; kb < k1; kb += kStep) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (A_KFAST) As[(ar + 16 * i) * kLd + ak] = ra[i];
      else As[ar * kLd + ak + 4 * i] = ra[i];
      if (B_KFAST) Bs[(br + 16 * i) * kLd + bk] = rb[i];
      else Bs[br * kLd + bk + 4 * i] = rb[i];
    }
    __syncthreads();
    if (kb + kStep < k1) fetch(kb + kStep);
#pragma unroll
    for (int kk = 0; kk < kStep; kk += 4) {
      const int k = kk + (lane >> 4);
      float af[WR], bf[WC];
#pragma unroll
      for (int i = 0; i < WR; ++i) af[i] = As[(wm + i * 16 + (lane & 15)) * kLd + k];
#pragma unroll
      for (int j = 0; j < WC; ++j) bf[j] = Bs[(wn + j * 16 + (lane & 15)) * kLd + k];
#pragma unroll
      for (int i = 0; i < WR; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
}

template <int WR, int WC>
__device__ inline void zero_acc(sh_f32x4 (&acc)[WR][WC]) {
#pragma unroll
  for (int i = 0; i < WR; ++i)
#pragma unroll
    for (int j = 0; j < WC; ++j) acc[i][j] = sh_f32x4{0.f, 0.f, 0.f, 0.f};
}

// grid (row tiles of q over 2 N H, tiles of the padded (c, m) rows), block 256.  C[i, q]: i = c * Mp + m.
__global__ __launch_bounds__(256) void lon_fwd_kernel(Geom g, const float* __restrict__ pred, const float* __restrict__ target,
                                                      const float* __restrict__ dft, float* __restrict__ F) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t NH = (int64_t)g.N * g.H, Q = 2 * NH;
  const int64_t q0 = (int64_t)blockIdx.x * kTile;
  const int i0 = blockIdx.y * kTile;
  const int c = i0 >= g.Mp ? 1 : 0;  // Mp is a multiple of the tile: a tile is all cos or all sin
  const float sgn = c ? -1.f : 1.f;
  sh_f32x4 acc[2][2];
  zero_acc(acc);
  auto la = [&](int r, int k) -> float { return k < g.Kf ? dft[(int64_t)(i0 + r) * g.W + k] : 0.f; };
  auto lb = [&](int col, int k) -> float {
    const int64_t q = q0 + col;
    if (q >= Q || k >= g.Kf) return 0.f;
    const float* x = q < NH ? pred + q * g.W : target + (q - NH) * g.W;
    float v = x[k];
    if (k > 0 && 2 * k != g.W) v += sgn * x[g.W - k];
    return v;
  };
  tile_product<2, 2, true, true>(acc, 0, g.Kf, la, lb, As, Bs);
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t q = q0 + wn + j * 16 + (lane & 15);
    if (q >= Q) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = i0 + wm + i * 16 + 4 * (lane >> 4) + r - c * g.Mp;
        if (m < g.M) F[((int64_t)c * g.M + m) * Q + q] = acc[i][j][r];
      }
  }
}

// grid (tiles of 16 fields, tiles of 64 degrees, m splits), block 256.  Wave w owns degrees l0 + 16 w + [0, 16) and the four
// 16-column blocks (pred re, pred im, target re, target im) of the same 16 fields, so a lane holds all four coefficients of
// its (l, n).  part[((z * 3 + s) * L + l) * N + n], s = pp, tt, num.  coef[((kind * M + m) * L + l) * N + n] when not NULL.
__global__ __launch_bounds__(256) void lat_fwd_kernel(Geom g, const float* __restrict__ F, const float* __restrict__ leg,
                                                      float* __restrict__ part, float* __restrict__ coef) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16, l0 = blockIdx.y * kTile;
  const int64_t fld_stride = g.H, Q = 2 * (int64_t)g.N * g.H;
  float pp[4] = {0.f, 0.f, 0.f, 0.f}, tt[4] = {0.f, 0.f, 0.f, 0.f}, num[4] = {0.f, 0.f, 0.f, 0.f};
  const int m_end = min(g.M, min(g.L, l0 + kTile));
  const int n = n0 + (lane & 15);
  for (int m = blockIdx.z; m < m_end; m += gridDim.z) {
    sh_f32x4 acc[1][4];
    zero_acc(acc);
    const float* Tm = leg + tri_off(m, g.L, g.H);
    auto la = [&](int r, int k) -> float {
      const int l = l0 + r;
      return (l >= m && l < g.L && k < g.H) ? Tm[(int64_t)(l - m) * g.H + k] : 0.f;
    };
    auto lb = [&](int col, int k) -> float {
      const int kind = col >> 4, nn = n0 + (col & 15);
      if (nn >= g.N || k >= g.H) return 0.f;
      const int64_t fld = (int64_t)(kind >> 1) * g.N + nn;
      return F[((int64_t)(kind & 1) * g.M + m) * Q + fld * fld_stride + k];
    };
    tile_product<1, 4, true, true>(acc, 0, g.H, la, lb, As, Bs);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = acc[0][0][r], ai = acc[0][1][r], br = acc[0][2][r], bi = acc[0][3][r];
      pp[r] = fmaf(ar, ar, fmaf(ai, ai, pp[r]));
      tt[r] = fmaf(br, br, fmaf(bi, bi, tt[r]));
      num[r] = fmaf(ar, br, fmaf(ai, bi, num[r]));
      const int l = l0 + wave * 16 + 4 * (lane >> 4) + r;
      if (coef && l >= m && l < g.L && n < g.N) {
        const int64_t plane = (int64_t)g.M * g.L * g.N, o = ((int64_t)m * g.L + l) * g.N + n;
        coef[o] = ar;
        coef[plane + o] = ai;
        coef[2 * plane + o] = br;
        coef[3 * plane + o] = bi;
      }
    }
  }
  if (n >= g.N) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int l = l0 + wave * 16 + 4 * (lane >> 4) + r;
    if (l >= g.L) continue;
    float* p = part + ((int64_t)blockIdx.z * 3 * g.L + l) * g.N + n;
    p[0] = pp[r];
    p[(int64_t)g.L * g.N] = tt[r];
    p[2 * (int64_t)g.L * g.N] = num[r];
  }
}

// one thread per e = l * N + n.  term[e] (fp64) is the loss term before the variance division; gfac[e] / gfac[L N + e] are
// d term / d pp and d term / d num times 1 / (N_fields * (var + eps)).
__global__ __launch_bounds__(256) void terms_kernel(Geom g, int splits, const float* __restrict__ part, const float* __restrict__ var,
                                                    double eps, double* __restrict__ term, float* __restrict__ gfac) {
  const int64_t LN = (int64_t)g.L * g.N;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  double pp = 0.0, tt = 0.0, num = 0.0;
  for (int z = 0; z < splits; ++z) {
    const float* p = part + (int64_t)z * 3 * LN + e;
    pp += (double)p[0];
    tt += (double)p[LN];
    num += (double)p[2 * LN];
  }
  const double den = sqrt(pp * tt), de = den + eps;
  const double sa = sqrt(pp + eps), sb = sqrt(tt + eps);
  const double coh = num / de;
  term[e] = (sa - sb) * (sa - sb) + 2.0 * den * (1.0 - coh);
  if (gfac) {
    const int n = (int)(e % g.N);
    const double scale = 1.0 / (((double)var[n % g.C] + eps) * (double)g.N);
    // d den / d pp = tt / (2 den): not finite where the field has no power at this degree, as the reference's autograd
    const double g_den = 2.0 - 2.0 * num * eps / (de * de);
    gfac[e] = (float)(((sa - sb) / sa + g_den * tt / (2.0 * den)) * scale);
    gfac[LN + e] = (float)(-2.0 * den / de * scale);
  }
}

// grid (tiles of 16 fields), block 256: thread (s, i) = (tid >> 4, tid & 15) sums the terms of field n0 + i over the degrees
// l = s, s + 16, ...; the 16 strided sums are added in order and scaled -> per[n] = sum_l term / (var + eps)
__global__ __launch_bounds__(256) void field_kernel(Geom g, const double* __restrict__ term, const float* __restrict__ var, double eps,
                                                    double* __restrict__ per) {
  __shared__ double red[16][16];
  const int i = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + i;
  double f = 0.0;
  if (n < g.N)
    for (int l = s; l < g.L; l += 16) f += term[(int64_t)l * g.N + n];
  red[s][i] = f;
  __syncthreads();
  if (s == 0 && n < g.N) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += red[k][i];
    per[n] = t / ((double)var[n % g.C] + eps);
  }
}

// one workgroup: the mean over the fields as a fixed-shape tree
__global__ __launch_bounds__(256) void final_kernel(Geom g, const double* __restrict__ per, float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int n = threadIdx.x; n < g.N; n += 256) s += per[n];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] / (double)g.N);
}

// grid (field tiles * latitude tiles, 2 (re / im), M), block 256.  C[n, k] over l in [m, L).
__global__ __launch_bounds__(256) void lat_bwd_kernel(Geom g, const float* __restrict__ coef, const float* __restrict__ gfac,
                                                      const float* __restrict__ dloss, const float* __restrict__ leg,
                                                      float* __restrict__ dF) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kt = (g.H + kTile - 1) / kTile;
  const int n0 = (blockIdx.x / kt) * kTile, h0 = (blockIdx.x % kt) * kTile;
  const int c = blockIdx.y, m = blockIdx.z;
  const int64_t LN = (int64_t)g.L * g.N, plane = (int64_t)g.M * LN;
  const float dl = *dloss;
  const float* ca = coef + (int64_t)c * plane + (int64_t)m * LN;
  const float* cb = ca + 2 * plane;
  const float* Tm = leg + tri_off(m, g.L, g.H);
  sh_f32x4 acc[2][2];
  zero_acc(acc);
  auto la = [&](int r, int k) -> float {
    const int n = n0 + r, l = m + k;
    if (n >= g.N || l >= g.L) return 0.f;
    const int64_t o = (int64_t)l * g.N + n;
    return dl * (2.f * gfac[o] * ca[o] + gfac[LN + o] * cb[o]);
  };
  auto lb = [&](int col, int k) -> float {
    const int h = h0 + col;
    return (h < g.H && m + k < g.L) ? Tm[(int64_t)k * g.H + h] : 0.f;
  };
  tile_product<2, 2, false, false>(acc, 0, g.L - m, la, lb, As, Bs);
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int h = h0 + wn + j * 16 + (lane & 15);
    if (h >= g.H) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (n < g.N) dF[(((int64_t)c * g.M + m) * g.N + n) * g.H + h] = acc[i][j][r];
      }
  }
}

// grid (row tiles of q over N H, tiles of the folded longitudes), block 256
__global__ __launch_bounds__(256) void lon_bwd_kernel(Geom g, const float* __restrict__ dF, const float* __restrict__ dft,
                                                      float* __restrict__ dx) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t Q = (int64_t)g.N * g.H;
  const int64_t q0 = (int64_t)blockIdx.x * kTile;
  const int j0 = blockIdx.y * kTile;
  sh_f32x4 even[2][2], odd[2][2];
  zero_acc(even);
  zero_acc(odd);
  auto half = [&](int c, sh_f32x4(&acc)[2][2]) {
    auto la = [&](int r, int k) -> float {
      const int64_t q = q0 + r;
      return (q < Q && k < g.M) ? dF[((int64_t)c * g.M + k) * Q + q] : 0.f;
    };
    auto lb = [&](int col, int k) -> float {
      const int j = j0 + col;
      return (j < g.Kf && k < g.M) ? dft[((int64_t)c * g.Mp + k) * g.W + j] : 0.f;
    };
    tile_product<2, 2, false, false>(acc, 0, g.M, la, lb, As, Bs);
  };
  half(0, even);
  half(1, odd);
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const int j = j0 + wn + jb * 16 + (lane & 15);
    if (j >= g.Kf) continue;
    const bool paired = j > 0 && 2 * j != g.W;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t q = q0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (q >= Q) continue;
        const float e = even[i][jb][r], o = odd[i][jb][r];
        dx[q * g.W + j] = e + o;
        if (paired) dx[q * g.W + (g.W - j)] = e - o;
      }
  }
}

bool make_geom(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, Geom* g) {
  if (fields < 1 || channels < 1 || fields % channels || nlat < 2 || nlon < 2) return false;
  g->N = fields;
  g->C = channels;
  g->H = nlat;
  g->W = nlon;
  g->L = nlat;
  g->M = nlat < nlon / 2 + 1 ? nlat : nlon / 2 + 1;
  g->Mp = (g->M + kTile - 1) / kTile * kTile;
  g->Kf = nlon / 2 + 1;
  return true;
}

int splits_of(const Geom& g) {
  const int tiles = ((g.N + 15) / 16) * ((g.L + kTile - 1) / kTile);
  int s = (768 + tiles - 1) / tiles;
  s = s > 32 ? 32 : s;
  s = s > g.M ? g.M : s;
  return s < 1 ? 1 : s;
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

struct Layout {
  size_t f_bytes, part_bytes, term_bytes;
  size_t total(bool backward) const { return backward ? f_bytes / 2 : f_bytes + part_bytes + term_bytes; }
};

Layout layout_of(const Geom& g) {
  Layout l;
  l.f_bytes = align256((size_t)2 * g.M * 2 * g.N * g.H * sizeof(float));  // the backward's dF is half of it (N fields)
  l.part_bytes = align256((size_t)splits_of(g) * 3 * g.L * g.N * sizeof(float));
  l.term_bytes = align256(((size_t)g.L + 1) * g.N * sizeof(double));  // the terms, then the per-field sums
  return l;
}

bool too_large(const Geom& g) {
  return (int64_t)2 * g.N * g.H > INT32_MAX / 4 || (int64_t)2 * g.N * g.H * g.W > ((int64_t)1 << 40) ||
         (int64_t)g.L * g.N > INT32_MAX / 4;
}

}  // namespace

extern "C" {

int32_t gw_amse_mmax(int32_t nlat, int32_t nlon) {
  if (nlat < 2 || nlon < 2) return 0;
  return nlat < nlon / 2 + 1 ? nlat : nlon / 2 + 1;
}

int32_t gw_amse_dft_rows(int32_t nlat, int32_t nlon) {
  const int m = gw_amse_mmax(nlat, nlon);
  return m ? 2 * ((m + kTile - 1) / kTile * kTile) : 0;
}

size_t gw_amse_legendre_floats(int32_t nlat, int32_t nlon) {
  const int m = gw_amse_mmax(nlat, nlon);
  return m ? (size_t)tri_off(m, nlat, nlat) : 0;
}

size_t gw_amse_coeff_floats(int32_t fields, int32_t nlat, int32_t nlon) {
  const int m = gw_amse_mmax(nlat, nlon);
  return (m && fields > 0) ? (size_t)4 * m * nlat * fields : 0;
}

size_t gw_amse_workspace_bytes(int32_t fields, int32_t nlat, int32_t nlon, int32_t backward) {
  Geom g;
  if (!make_geom(fields, 1, nlat, nlon, &g)) {
    set_error(GW_E_BADARG, "gw_amse_workspace_bytes: fields >= 1, nlat >= 2 and nlon >= 2 are required");
    return 0;
  }
  return layout_of(g).total(backward != 0);
}

int gw_amse_forward(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, const float* pred, const float* target,
                    const float* dft, const float* legendre, const float* variance, double epsilon, void* workspace,
                    size_t workspace_bytes, float* coeff, float* gfac, float* loss, void* stream) {
  Geom g;
  if (!make_geom(fields, channels, nlat, nlon, &g))
    return fail("gw_amse_forward: fields a positive multiple of channels, nlat >= 2 and nlon >= 2 are required");
  if (!pred || !target || !dft || !legendre || !variance || !loss) return fail("gw_amse_forward: null operand");
  if ((coeff == nullptr) != (gfac == nullptr)) return fail("gw_amse_forward: coeff and gfac are saved together or not at all");
  if (too_large(g)) return set_error(GW_E_UNSUPPORTED, "gw_amse_forward: shape too large");
  const Layout lay = layout_of(g);
  if (!workspace || workspace_bytes < lay.total(false)) return fail("gw_amse_forward: workspace smaller than gw_amse_workspace_bytes");
  float* F = (float*)workspace;
  float* part = (float*)((char*)workspace + lay.f_bytes);
  double* term = (double*)((char*)workspace + lay.f_bytes + lay.part_bytes);
  hipStream_t s = (hipStream_t)stream;
  const int64_t Q = 2 * (int64_t)g.N * g.H;
  hipLaunchKernelGGL(lon_fwd_kernel, dim3((unsigned)((Q + kTile - 1) / kTile), (unsigned)(2 * g.Mp / kTile)), dim3(256), 0, s, g, pred,
                     target, dft, F);
  int rc = check_launch("lon_fwd_kernel launch");
  if (rc != GW_OK) return rc;
  const int splits = splits_of(g);
  hipLaunchKernelGGL(lat_fwd_kernel, dim3((g.N + 15) / 16, (g.L + kTile - 1) / kTile, splits), dim3(256), 0, s, g, (const float*)F,
                     legendre, part, coeff);
  if ((rc = check_launch("lat_fwd_kernel launch")) != GW_OK) return rc;
  const int64_t LN = (int64_t)g.L * g.N;
  hipLaunchKernelGGL(terms_kernel, dim3((unsigned)((LN + 255) / 256)), dim3(256), 0, s, g, splits, (const float*)part, variance, epsilon,
                     term, gfac);
  if ((rc = check_launch("terms_kernel launch")) != GW_OK) return rc;
  double* per = term + LN;
  hipLaunchKernelGGL(field_kernel, dim3((g.N + 15) / 16), dim3(256), 0, s, g, (const double*)term, variance, epsilon, per);
  if ((rc = check_launch("field_kernel launch")) != GW_OK) return rc;
  hipLaunchKernelGGL(final_kernel, dim3(1), dim3(256), 0, s, g, (const double*)per, loss);
  return check_launch("final_kernel launch");
}

int gw_amse_backward(int32_t fields, int32_t nlat, int32_t nlon, const float* coeff, const float* gfac, const float* dloss,
                     const float* dft, const float* legendre, void* workspace, size_t workspace_bytes, float* dpred, void* stream) {
  Geom g;
  if (!make_geom(fields, 1, nlat, nlon, &g)) return fail("gw_amse_backward: fields >= 1, nlat >= 2 and nlon >= 2 are required");
  if (!coeff || !gfac || !dloss || !dft || !legendre || !dpred) return fail("gw_amse_backward: null operand");
  if (too_large(g)) return set_error(GW_E_UNSUPPORTED, "gw_amse_backward: shape too large");
  const Layout lay = layout_of(g);
  if (!workspace || workspace_bytes < lay.total(true)) return fail("gw_amse_backward: workspace smaller than gw_amse_workspace_bytes");
  float* dF = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int nt = (g.N + kTile - 1) / kTile, kt = (g.H + kTile - 1) / kTile;
  hipLaunchKernelGGL(lat_bwd_kernel, dim3(nt * kt, 2, g.M), dim3(256), 0, s, g, coeff, gfac, dloss, legendre, dF);
  int rc = check_launch("lat_bwd_kernel launch");
  if (rc != GW_OK) return rc;
  const int64_t Q = (int64_t)g.N * g.H;
  hipLaunchKernelGGL(lon_bwd_kernel, dim3((unsigned)((Q + kTile - 1) / kTile), (unsigned)((g.Kf + kTile - 1) / kTile)), dim3(256), 0, s, g,
                     (const float*)dF, dft, dpred);
  return check_launch("lon_bwd_kernel launch");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The inverse transform: torch_harmonics.InverseRealSHT(nlat, nlon, lmax, mmax = lmax + 1, grid="equiangular"), which GenCast's
// generate_isotropic_noise (utils/noise.py) applies to white coefficients.  Two products with the structure of the adjoint pair
// above, on unweighted Legendre functions and the irfft matrix (no quadrature weights, no loss terms):
//   isht_lat_kernel   per order m: G_c[m, k, q] = sum_{l >= m} c_c[q, l, m] * P[m, l, k], c = re / im, straight from the
//                     interleaved complex64 coefficients [fields, lmax, mmax].  The K range starts at l = m.  The imaginary
//                     part of m = 0 is read as zero (irfft ignores it); the order m = lmax = nlon / 2 has no degree l < lmax
//                     at all, so it is never visited and its imaginary part is ignored too.
//   isht_lon_kernel   out[b, j, k, ch] = scale * sum_{c, m < lmax} D[c, m, j] * G_c[m, k, q], q = b * C + ch, folded about
//                     j = nlon / 2 as lon_bwd_kernel folds.  The rows of G are (k, q) with q fastest, so the 16 lanes of an
//                     accumulator column write consecutive channels of the final [B, lon, lat, C] layout: no permute pass.
// One fixed summation order per output element, independent of the number of fields; no atomics; no host synchronisation.
namespace {

// lmax of the two grids generate_isotropic_noise accepts, 0 for any other
int isht_lmax(int nlat, int nlon) {
  if (nlat < 2 || nlon < 2) return 0;
  if (nlon == 2 * nlat) return nlat;
  if (nlon == 2 * (nlat - 1)) return nlat - 1;
  return 0;
}

bool make_isht_geom(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, Geom* g) {
  const int L = isht_lmax(nlat, nlon);
  if (fields < 1 || channels < 1 || fields % channels || L < 1) return false;
  g->N = fields;
  g->C = channels;
  g->H = nlat;
  g->W = nlon;
  g->L = L;
  g->M = L + 1;
  g->Mp = (g->M + kTile - 1) / kTile * kTile;
  g->Kf = nlon / 2 + 1;
  return true;
}

size_t isht_bytes(const Geom& g) { return align256((size_t)2 * g.L * g.N * g.H * sizeof(float)); }

// grid (lmax orders, latitude tiles, tiles of 32 fields), block 256.  Tile rows are latitudes, tile columns (c, field): columns
// [0, 32) the real parts of 32 fields, [32, 64) their imaginary parts.  G[((c * L + m) * H + k) * N + q].
__global__ __launch_bounds__(256) void isht_lat_kernel(Geom g, const float* __restrict__ coef, const float* __restrict__ leg,
                                                       float* __restrict__ G) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x, h0 = blockIdx.y * kTile, n0 = blockIdx.z * 32;
  const float* Pm = leg + tri_off(m, g.L, g.H);
  sh_f32x4 acc[2][2];
  zero_acc(acc);
  auto la = [&](int r, int k) -> float {
    const int h = h0 + r;
    return (h < g.H && m + k < g.L) ? Pm[(int64_t)k * g.H + h] : 0.f;
  };
  auto lb = [&](int col, int k) -> float {
    const int c = col >> 5, n = n0 + (col & 31), l = m + k;
    if (n >= g.N || l >= g.L || (c && m == 0)) return 0.f;
    return coef[(((int64_t)n * g.L + l) * g.M + m) * 2 + c];
  };
  tile_product<2, 2, false, true>(acc, 0, g.L - m, la, lb, As, Bs);
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int c = wn >> 5;  // a wave's 32 columns are all real or all imaginary
  float* Gm = G + ((int64_t)c * g.L + m) * g.H * g.N;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + j * 16 + (lane & 15);
    if (n >= g.N) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = h0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (h < g.H) Gm[(int64_t)h * g.N + n] = acc[i][j][r];
      }
  }
}

// grid (tiles of the (k, q) rows of G over H N, tiles of the folded longitudes), block 256.  Tile rows are longitudes, tile
// columns the rows of G.
__global__ __launch_bounds__(256) void isht_lon_kernel(Geom g, const float* __restrict__ G, const float* __restrict__ syn, float scale,
                                                       float* __restrict__ out) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t R = (int64_t)g.H * g.N;
  const int64_t q0 = (int64_t)blockIdx.x * kTile;
  const int j0 = blockIdx.y * kTile;
  sh_f32x4 even[2][2], odd[2][2];
  zero_acc(even);
  zero_acc(odd);
  auto half = [&](int c, sh_f32x4(&acc)[2][2]) {
    auto la = [&](int r, int k) -> float {
      const int j = j0 + r;
      return (j < g.Kf && k < g.L) ? syn[((int64_t)c * g.Mp + k) * g.W + j] : 0.f;
    };
    auto lb = [&](int col, int k) -> float {
      const int64_t q = q0 + col;
      return (q < R && k < g.L) ? G[((int64_t)c * g.L + k) * R + q] : 0.f;
    };
    tile_product<2, 2, false, false>(acc, 0, g.L, la, lb, As, Bs);
  };
  half(0, even);
  half(1, odd);
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const int64_t row = q0 + wn + jb * 16 + (lane & 15);
    if (row >= R) continue;
    const int k = (int)(row / g.N), q = (int)(row % g.N);
    const int b = q / g.C, ch = q % g.C;
    float* o = out + ((int64_t)b * g.W * g.H + k) * g.C + ch;  // + j * H * C
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (j >= g.Kf) continue;
        const float e = even[i][jb][r], d = odd[i][jb][r];
        o[(int64_t)j * g.H * g.C] = scale * (e + d);
        if (j > 0 && 2 * j != g.W) o[(int64_t)(g.W - j) * g.H * g.C] = scale * (e - d);
      }
  }
}

}  // namespace

extern "C" {

int32_t gw_isht_lmax(int32_t nlat, int32_t nlon) { return isht_lmax(nlat, nlon); }

size_t gw_isht_legendre_floats(int32_t nlat, int32_t nlon) {
  const int L = isht_lmax(nlat, nlon);
  return L ? (size_t)tri_off(L + 1, L, nlat) : 0;
}

size_t gw_isht_workspace_bytes(int32_t fields, int32_t nlat, int32_t nlon) {
  Geom g;
  if (!make_isht_geom(fields, 1, nlat, nlon, &g)) {
    set_error(GW_E_BADARG, "gw_isht_workspace_bytes: fields >= 1 and nlon = 2 nlat or 2 (nlat - 1) are required");
    return 0;
  }
  return isht_bytes(g);
}

int gw_isht_forward(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, const float* coeffs, const float* synthesis,
                    const float* legendre, float scale, void* workspace, size_t workspace_bytes, float* out, void* stream) {
  Geom g;
  if (!make_isht_geom(fields, channels, nlat, nlon, &g))
    return fail("gw_isht_forward: fields a positive multiple of channels and nlon = 2 nlat or 2 (nlat - 1) are required");
  if (!coeffs || !synthesis || !legendre || !out) return fail("gw_isht_forward: null operand");
  const int64_t R = (int64_t)g.N * g.H;
  if (R > INT32_MAX / 4 || R * g.W > ((int64_t)1 << 40) || (g.N + 31) / 32 > 65535)
    return set_error(GW_E_UNSUPPORTED, "gw_isht_forward: shape too large");
  if (!workspace || workspace_bytes < isht_bytes(g)) return fail("gw_isht_forward: workspace smaller than gw_isht_workspace_bytes");
  float* G = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(isht_lat_kernel, dim3(g.L, (g.H + kTile - 1) / kTile, (g.N + 31) / 32), dim3(256), 0, s, g, coeffs, legendre, G);
  int rc = check_launch("isht_lat_kernel launch");
  if (rc != GW_OK) return rc;
  hipLaunchKernelGGL(isht_lon_kernel, dim3((unsigned)((R + kTile - 1) / kTile), (unsigned)((g.Kf + kTile - 1) / kTile)), dim3(256), 0, s, g,
                     (const float*)G, synthesis, scale, out);
  return check_launch("isht_lon_kernel launch");
}

}  // extern "C"
