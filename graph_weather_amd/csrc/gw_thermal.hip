// gw_thermal.hip - ThermalizerLayer (graph_weather/models/layers/thermalizer.py): the AdaptiveUNet score model and the
// diffusion step around it, on NHWC pixel rows (row (b * H + y) * W + x, one channel per column).  Everything is fp32.
//
//   conv_nt_kernel       implicit GEMM (pixels x cout, K = taps x cin) on v_mfma_f32_16x16x4_f32: Conv2d, its input
//                        gradient, the output-parity sub-convolutions of ConvTranspose2d and that transpose's input gradient.
//                        The operand load applies GroupNorm + ReLU of the producer, or forms the noisy input and the two
//                        position channels; the epilogue adds the bias, or writes (noisy - s1 * eps_hat) / sa.
//   conv_tn_kernel       weight gradient: per-tap TN products over fixed pixel slabs -> partials; wgrad_reduce_kernel sums
//                        the slabs in one fixed order into the weight layout
//   colsum_*             bias gradients (column sums), slab partials summed in one fixed order
//   gn_*                 GroupNorm statistics as (count, mean, M2) partials merged with Chan's formula in one fixed order;
//                        backward sums of dy and dy * xhat per (sample, channel) in one fixed order
//   maxpool_*            MaxPool2d(3, 2, 1) with the argmax kept; backward as a gather over the windows holding a pixel
//   resize_*             bilinear resize (align_corners=False); backward as a gather over the output pixels reading a pixel
//   rows_kernel          row-wise ends of the diffusion step
// No float atomics anywhere: every result is bitwise reproducible.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_internal.hpp"

using namespace gw;

namespace {

typedef float th_f32x4 __attribute__((ext_vector_type(4)));

int fail(const char* msg) { return set_error(GW_E_BADARG, msg); }

constexpr int kTile = 64;     // GEMM tile (64 x 64, four waves of 32 x 32)
constexpr int kStep = 16;     // K per LDS stage
constexpr int kLdA = kStep + 1;

__device__ inline float diffuse(float sa, float s1, float x, float e) { return sa * x + s1 * e; }

__device__ inline float pos_coord(int i, int n) { return n > 1 ? (float)i / (float)(n - 1) : 0.f; }

// ReLU as torch computes it: NaN stays NaN (fmaxf would turn it into 0).  The backward masks use z > 0, which is false for
// NaN, as torch's threshold backward.
__device__ inline float relu_nan(float z) { return z > 0.f ? z : (z != z ? z : 0.f); }

// A operand of pixel row `row` (image b, coordinates iy, ix), channel ci < cin.
template <int AMODE>
__device__ inline float load_a(const gw_thermal_conv_args& g, int64_t row, int b, int iy, int ix, int ci) {
  if (AMODE == GW_THERMAL_A_DIFFUSE) {
    const int F = g.features;
    if (ci < F) return diffuse(g.sa, g.s1, g.a[row * g.ld_a + ci], g.eps[row * F + ci]);
    return ci == F ? pos_coord(ix, g.in_w) : pos_coord(iy, g.in_h);
  }
  const float v = g.a[row * g.ld_a + ci];
  if (AMODE == GW_THERMAL_A_GN_RELU) {
    const int k = b * g.cin + ci;
    return relu_nan(fmaf(v, g.a_scale[k], g.a_shift[k]));
  }
  return v;
}

// grid (M tiles, N tiles), block 256.  Wave w computes rows (w & 1) * 32 + [0, 32) x columns (w >> 1) * 32 + [0, 32) of the
// 64 x 64 tile as 2 x 2 MFMA blocks.  Loader: thread -> K column tid & 15 of pixels (tid >> 4) + 16 i (A), weight row
// (tid >> 6) * 4 + i of column tid & 63 (B).
template <int AMODE, int EMODE>
__global__ __launch_bounds__(256) void conv_nt_kernel(gw_thermal_conv_args g) {
  __shared__ float As[kTile * kLdA];
  __shared__ float Bs[kStep * kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int Q = g.q_h * g.q_w;
  const int M = g.batch * Q;
  const int m0 = blockIdx.x * kTile, n0 = blockIdx.y * kTile;
  const int lk = tid & 15, lr = tid >> 4;
  int pb[4], pqy[4], pqx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + lr + 16 * i;
    if (m < M) {
      pb[i] = m / Q;
      const int r = m - pb[i] * Q;
      pqy[i] = r / g.q_w;
      pqx[i] = r - pqy[i] * g.q_w;
    } else {
      pb[i] = -1;
      pqy[i] = pqx[i] = 0;
    }
  }
  th_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = th_f32x4{0.f, 0.f, 0.f, 0.f};
  const int bn = n0 + lane;
  const int bk = (tid >> 6) * 4;
  for (int ty = 0; ty < g.ty.n; ++ty) {
    for (int tx = 0; tx < g.tx.n; ++tx) {
      int64_t prow[4];
      int piy[4], pix[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        piy[i] = g.in_scale_h * pqy[i] + g.ty.in_off[ty];
        pix[i] = g.in_scale_w * pqx[i] + g.tx.in_off[tx];
        const bool ok = pb[i] >= 0 && piy[i] >= 0 && piy[i] < g.in_h && pix[i] >= 0 && pix[i] < g.in_w;
        prow[i] = ok ? ((int64_t)pb[i] * g.in_h + piy[i]) * g.in_w + pix[i] : -1;
      }
      const int64_t woff = (int64_t)g.ty.w_idx[ty] * g.w_stride_y + (int64_t)g.tx.w_idx[tx] * g.w_stride_x;
      for (int c0 = 0; c0 < g.cin; c0 += kStep) {
        const int ci = c0 + lk;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          As[(lr + 16 * i) * kLdA + lk] = (prow[i] >= 0 && ci < g.cin) ? load_a<AMODE>(g, prow[i], pb[i], piy[i], pix[i], ci) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int wc = c0 + bk + i;
          Bs[(bk + i) * kTile + lane] =
              (wc < g.cin && bn < g.cout) ? g.w[woff + (int64_t)wc * g.w_stride_ci + (int64_t)bn * g.w_stride_co] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kStep; kk += 4) {
          const int k = kk + (lane >> 4);
          float af[2], bf[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) af[i] = As[(wm + i * 16 + (lane & 15)) * kLdA + k];
#pragma unroll
          for (int j = 0; j < 2; ++j) bf[j] = Bs[k * kTile + wn + j * 16 + (lane & 15)];
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
      }
    }
  }
  // C/D map: column lane & 15, row 4 * (lane >> 4) + r
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = n0 + wn + j * 16 + (lane & 15);
    if (co >= g.cout) continue;
    const float bias = g.bias ? g.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (m >= M) continue;
        const int b = m / Q;
        const int rq = m - b * Q;
        const int qy = rq / g.q_w, qx = rq - (rq / g.q_w) * g.q_w;
        const int oy = g.out_scale_h * qy + g.out_off_h, ox = g.out_scale_w * qx + g.out_off_w;
        if (oy >= g.out_h || ox >= g.out_w) continue;
        const int64_t orow = ((int64_t)b * g.out_h + oy) * g.out_w + ox;
        const float v = acc[i][j][r] + bias;
        if (EMODE == GW_THERMAL_E_DIFFUSE) {
          const float noisy = diffuse(g.sa, g.s1, g.x[orow * g.ld_x + co], g.eps[orow * g.features + co]);
          g.out[orow * g.ld_out + co] = (noisy - g.s1 * v) / g.sa;
        } else {
          g.out[orow * g.ld_out + co] = v;
        }
      }
    }
  }
}

// Weight gradient.  grid (cin tiles * cout tiles, slabs, live taps), block 256: the 64 x 64 (ci, co) tile of one tap over
// the GEMM pixels [slab * slab_px, +slab_px) -> part[((slab * taps + tap) * cin + ci) * cout + co].
template <int AMODE>
__global__ __launch_bounds__(256) void conv_tn_kernel(gw_thermal_conv_args g, int slab_px, float* __restrict__ part) {
  __shared__ float As[kStep * kTile];
  __shared__ float Gs[kStep * kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int ntn = (g.cout + kTile - 1) / kTile;
  const int ci0 = (blockIdx.x / ntn) * kTile, co0 = (blockIdx.x % ntn) * kTile;
  const int tap = blockIdx.z, ty = tap / g.tx.n, tx = tap - ty * g.tx.n;
  const int Q = g.q_h * g.q_w;
  const int M = g.batch * Q;
  const int p0 = blockIdx.y * slab_px, p1 = min(M, p0 + slab_px);
  th_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = th_f32x4{0.f, 0.f, 0.f, 0.f};
  const int ci = ci0 + lane, co = co0 + lane;
  for (int pk = p0; pk < p1; pk += kStep) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = wave * 4 + i;
      const int m = pk + k;
      float av = 0.f, gv = 0.f;
      if (m < p1) {
        const int b = m / Q;
        const int rq = m - b * Q;
        const int qy = rq / g.q_w, qx = rq - (rq / g.q_w) * g.q_w;
        const int iy = g.in_scale_h * qy + g.ty.in_off[ty], ix = g.in_scale_w * qx + g.tx.in_off[tx];
        if (ci < g.cin && iy >= 0 && iy < g.in_h && ix >= 0 && ix < g.in_w)
          av = load_a<AMODE>(g, ((int64_t)b * g.in_h + iy) * g.in_w + ix, b, iy, ix, ci);
        const int oy = g.out_scale_h * qy + g.out_off_h, ox = g.out_scale_w * qx + g.out_off_w;
        if (co < g.cout && oy < g.out_h && ox < g.out_w) gv = g.out[(((int64_t)b * g.out_h + oy) * g.out_w + ox) * g.ld_out + co];
      }
      As[k * kTile + lane] = av;
      Gs[k * kTile + lane] = gv;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kStep; kk += 4) {
      const int k = kk + (lane >> 4);
      float af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = As[k * kTile + wm + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = Gs[k * kTile + wn + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  const int ntaps = g.ty.n * g.tx.n;
  float* dst = part + ((int64_t)blockIdx.y * ntaps + tap) * g.cin * g.cout;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = co0 + wn + j * 16 + (lane & 15);
    if (c >= g.cout) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cc = ci0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (cc < g.cin) dst[(int64_t)cc * g.cout + c] = acc[i][j][r];
      }
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(gw_thermal_conv_args g, int slabs, const float* __restrict__ part,
                                                           float* __restrict__ dw) {
  const int ntaps = g.ty.n * g.tx.n;
  const int64_t per_tap = (int64_t)g.cin * g.cout;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per_tap * ntaps) return;
  const int tap = (int)(e / per_tap);
  const int64_t r = e - tap * per_tap;
  const int ci = (int)(r / g.cout), co = (int)(r - (int64_t)ci * g.cout);
  float s = 0.f;
  for (int k = 0; k < slabs; ++k) s += part[(int64_t)k * ntaps * per_tap + e];
  const int ty = tap / g.tx.n, tx = tap - ty * g.tx.n;
  dw[(int64_t)g.ty.w_idx[ty] * g.w_stride_y + (int64_t)g.tx.w_idx[tx] * g.w_stride_x + (int64_t)ci * g.w_stride_ci +
     (int64_t)co * g.w_stride_co] = s;
}

constexpr int kColSlab = 256;  // rows per column-sum partial

// grid (column tiles, slabs), block 256: lane -> column, wave -> every 4th row of the slab
__global__ __launch_bounds__(256) void colsum_partial_kernel(int64_t rows, int cols, const float* __restrict__ g, int ld,
                                                             float* __restrict__ part) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * kColSlab, r1 = min(rows, r0 + kColSlab);
  float s = 0.f;
  if (c < cols)
    for (int64_t r = r0 + wave; r < r1; r += 4) s += g[r * ld + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < cols) part[(int64_t)blockIdx.y * cols + c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

__global__ __launch_bounds__(256) void colsum_final_kernel(int cols, int slabs, const float* __restrict__ part, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int k = 0; k < slabs; ++k) s += part[(int64_t)k * cols + c];
  out[c] = s;
}

constexpr int kGnSlab = 256;  // pixels per GroupNorm statistics partial

struct Moments {
  float n, mean, m2;
};

__device__ inline Moments chan_merge(Moments a, Moments b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  return Moments{n, a.mean + d * fb, a.m2 + b.m2 + d * d * a.n * fb};
}

// grid (batch * groups, slabs), block 256: Welford over the slab's elements, then a fixed-order tree of Chan merges
__global__ __launch_bounds__(256) void gn_stats_partial_kernel(int hw, int C, int groups, const float* __restrict__ x, int ld,
                                                               float* __restrict__ part) {
  __shared__ float red[3][256];
  const int bg = blockIdx.x, b = bg / groups, gi = bg - b * groups;
  const int cpg = C / groups;
  const int p0 = blockIdx.y * kGnSlab, p1 = min(hw, p0 + kGnSlab);
  const int n_el = (p1 - p0) * cpg;
  Moments m{0.f, 0.f, 0.f};
  for (int e = threadIdx.x; e < n_el; e += 256) {
    const int p = p0 + e / cpg, c = gi * cpg + e % cpg;
    const float v = x[((int64_t)b * hw + p) * ld + c];
    m.n += 1.f;
    const float d = v - m.mean;
    m.mean += d / m.n;
    m.m2 += d * (v - m.mean);
  }
  red[0][threadIdx.x] = m.n;
  red[1][threadIdx.x] = m.mean;
  red[2][threadIdx.x] = m.m2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const Moments o = chan_merge(Moments{red[0][threadIdx.x], red[1][threadIdx.x], red[2][threadIdx.x]},
                                   Moments{red[0][threadIdx.x + s], red[1][threadIdx.x + s], red[2][threadIdx.x + s]});
      red[0][threadIdx.x] = o.n;
      red[1][threadIdx.x] = o.mean;
      red[2][threadIdx.x] = o.m2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float* p = part + ((int64_t)bg * gridDim.y + blockIdx.y) * 3;
    p[0] = red[0][0];
    p[1] = red[1][0];
    p[2] = red[2][0];
  }
}

// one thread per (b, g): slab partials merged in slab order (fp64), then the per-channel affine of the consumer's load
__global__ __launch_bounds__(64) void gn_stats_final_kernel(int batch, int C, int groups, int slabs, const float* __restrict__ part,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            float* __restrict__ stats, float* __restrict__ scale,
                                                            float* __restrict__ shift) {
  const int bg = blockIdx.x * 64 + threadIdx.x;
  if (bg >= batch * groups) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int k = 0; k < slabs; ++k) {
    const float* p = part + ((int64_t)bg * slabs + k) * 3;
    const double nb = p[0];
    if (nb == 0.0) continue;
    const double tot = n + nb, d = (double)p[1] - mean;
    mean += d * nb / tot;
    m2 += (double)p[2] + d * d * n * nb / tot;
    n = tot;
  }
  const float mu = (float)mean;
  const float rstd = (float)(1.0 / sqrt(m2 / n + (double)eps));
  stats[bg * 2] = mu;
  stats[bg * 2 + 1] = rstd;
  const int b = bg / groups, gi = bg - b * groups, cpg = C / groups;
  for (int c = gi * cpg; c < (gi + 1) * cpg; ++c) {
    const float sc = gamma[c] * rstd;
    scale[b * C + c] = sc;
    shift[b * C + c] = beta[c] - mu * sc;
  }
}

// grid (batch * channel tiles, slabs), block 256: per (b, c) sums of dz and dz * xhat over the slab's pixels,
// dz = dy * [x * scale + shift > 0] -> part[(slab * batch + b) * C + c] (two planes)
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(int batch, int hw, int C, int groups, const float* __restrict__ x, int ld,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ stats, const float* __restrict__ dy,
                                                             int ld_dy, float* __restrict__ part) {
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ct = (C + 63) / 64;
  const int b = blockIdx.x / ct, c = (blockIdx.x - b * ct) * 64 + lane;
  const int p0 = blockIdx.y * kGnSlab, p1 = min(hw, p0 + kGnSlab);
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const int bg = b * groups + c / (C / groups);
    const float mu = stats[bg * 2], rstd = stats[bg * 2 + 1];
    const float sc = scale[b * C + c], sh = shift[b * C + c];
    for (int p = p0 + wave; p < p1; p += 4) {
      const int64_t row = (int64_t)b * hw + p;
      const float v = x[row * ld + c];
      const float dz = fmaf(v, sc, sh) > 0.f ? dy[row * ld_dy + c] : 0.f;
      s1 += dz;
      s2 += dz * ((v - mu) * rstd);
    }
  }
  red[0][wave][lane] = s1;
  red[1][wave][lane] = s2;
  __syncthreads();
  if (wave == 0 && c < C) {
    const int64_t o = ((int64_t)blockIdx.y * batch + b) * C + c;
    const int64_t plane = (int64_t)gridDim.y * batch * C;
    part[o] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    part[plane + o] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
  }
}

// one block: S1, S2 per (b, c) over the slabs in order; dgamma / dbeta over the batch in order; per (b, g) the two sums of
// the input gradient's mean terms, coef[b, g] = (sum gamma * S1, sum gamma * S2)
__global__ __launch_bounds__(256) void gn_bwd_final_kernel(int batch, int C, int groups, int slabs, const float* __restrict__ part,
                                                           const float* __restrict__ gamma, float* __restrict__ sums,
                                                           float* __restrict__ coef, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  const int64_t plane = (int64_t)slabs * batch * C;
  for (int e = threadIdx.x; e < batch * C; e += 256) {
    float a = 0.f, q = 0.f;
    for (int k = 0; k < slabs; ++k) {
      a += part[(int64_t)k * batch * C + e];
      q += part[plane + (int64_t)k * batch * C + e];
    }
    sums[e] = a;
    sums[batch * C + e] = q;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, q = 0.f;
    for (int b = 0; b < batch; ++b) {
      a += sums[b * C + c];
      q += sums[batch * C + b * C + c];
    }
    if (dbeta) dbeta[c] = a;
    if (dgamma) dgamma[c] = q;
  }
  const int cpg = C / groups;
  for (int bg = threadIdx.x; bg < batch * groups; bg += 256) {
    const int b = bg / groups, gi = bg - b * groups;
    float a = 0.f, q = 0.f;
    for (int c = gi * cpg; c < (gi + 1) * cpg; ++c) {
      a += gamma[c] * sums[b * C + c];
      q += gamma[c] * sums[batch * C + b * C + c];
    }
    coef[bg * 2] = a;
    coef[bg * 2 + 1] = q;
  }
}

// dx = rstd * (gamma * dz - (A + xhat * B) / n)
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(int64_t total, int hw, int C, int groups, const float* __restrict__ x, int ld,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ dy, int ld_dy, const float* __restrict__ coef,
                                                           float* __restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / C;
  const int c = (int)(e - row * C);
  const int b = (int)(row / hw);
  const int cpg = C / groups;
  const int bg = b * groups + c / cpg;
  const float mu = stats[bg * 2], rstd = stats[bg * 2 + 1];
  const float v = x[row * ld + c];
  const float dz = fmaf(v, scale[b * C + c], shift[b * C + c]) > 0.f ? dy[row * ld_dy + c] : 0.f;
  const float inv_n = 1.f / ((float)hw * (float)cpg);
  const float xh = (v - mu) * rstd;
  dx[e] = rstd * (gamma[c] * dz - (coef[bg * 2] + xh * coef[bg * 2 + 1]) * inv_n);
}

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(int64_t total, int h, int w, int ho, int wo, int C, const float* __restrict__ x,
                                                          int ld, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          float* __restrict__ out, int ld_out, int32_t* __restrict__ idx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t orow = e / C;
  const int c = (int)(e - orow * C);
  const int b = (int)(orow / ((int64_t)ho * wo));
  const int r = (int)(orow - (int64_t)b * ho * wo);
  const int oy = r / wo, ox = r - (r / wo) * wo;
  const float sc = scale[b * C + c], sh = shift[b * C + c];
  float best = -INFINITY;
  int arg = -1;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= h) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= w) continue;
      const float v = relu_nan(fmaf(x[(((int64_t)b * h + iy) * w + ix) * ld + c], sc, sh));
      if (v > best || arg < 0 || v != v) {
        best = v;
        arg = iy * w + ix;
      }
    }
  }
  out[orow * ld_out + c] = best;
  idx[e] = arg;
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(int64_t total, int h, int w, int ho, int wo, int C, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ g1, int ld1, const float* __restrict__ g2, int ld2,
                                                          float* __restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / C;
  const int c = (int)(e - row * C);
  const int b = (int)(row / ((int64_t)h * w));
  const int r = (int)(row - (int64_t)b * h * w);
  const int iy = r / w, ix = r - (r / w) * w;
  float s = 0.f;
  for (int oy = iy / 2; oy <= min((iy + 1) / 2, ho - 1); ++oy)
    for (int ox = ix / 2; ox <= min((ix + 1) / 2, wo - 1); ++ox) {
      const int64_t orow = ((int64_t)b * ho + oy) * wo + ox;
      if (idx[orow * C + c] == r) s += g2 ? g1[orow * ld1 + c] + g2[orow * ld2 + c] : g1[orow * ld1 + c];
    }
  dx[e] = s;
}

struct Lerp {
  int i0, i1;
  float l0, l1;
};

// interpolate(mode="bilinear", align_corners=False) source index of output index o (size n_in -> n_out)
__device__ inline Lerp lerp_of(int o, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  const int i0 = (int)src;
  const int step = i0 < n_in - 1 ? 1 : 0;
  const float l1 = src - (float)i0;
  return Lerp{i0, i0 + step, 1.f - l1, l1};
}

__global__ __launch_bounds__(256) void resize_fwd_kernel(int64_t total, int hi, int wi, int ho, int wo, int C, const float* __restrict__ x,
                                                         int ld, float* __restrict__ out, int ld_out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t orow = e / C;
  const int c = (int)(e - orow * C);
  const int b = (int)(orow / ((int64_t)ho * wo));
  const int r = (int)(orow - (int64_t)b * ho * wo);
  const int oy = r / wo, ox = r - (r / wo) * wo;
  const Lerp ly = lerp_of(oy, hi, ho), lx = lerp_of(ox, wi, wo);
  const float* base = x + (int64_t)b * hi * wi * ld + c;
  const float v00 = base[((int64_t)ly.i0 * wi + lx.i0) * ld], v01 = base[((int64_t)ly.i0 * wi + lx.i1) * ld];
  const float v10 = base[((int64_t)ly.i1 * wi + lx.i0) * ld], v11 = base[((int64_t)ly.i1 * wi + lx.i1) * ld];
  out[orow * ld_out + c] = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

__device__ inline float lerp_weight(const Lerp& l, int i) { return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f); }

// output indices whose source pair can hold input index i (a superset; lerp_weight picks the exact ones)
__device__ inline void lerp_range(int i, int n_in, int n_out, int& lo, int& hi) {
  const float inv = (float)n_out / (float)n_in;
  lo = max(0, (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1);
  hi = min(n_out - 1, (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1);
}

__global__ __launch_bounds__(256) void resize_bwd_kernel(int64_t total, int hi, int wi, int ho, int wo, int C, const float* __restrict__ g,
                                                         int ld_g, float* __restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / C;
  const int c = (int)(e - row * C);
  const int b = (int)(row / ((int64_t)hi * wi));
  const int r = (int)(row - (int64_t)b * hi * wi);
  const int iy = r / wi, ix = r - (r / wi) * wi;
  int ylo, yhi, xlo, xhi;
  lerp_range(iy, hi, ho, ylo, yhi);
  lerp_range(ix, wi, wo, xlo, xhi);
  float s = 0.f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float wy = lerp_weight(lerp_of(oy, hi, ho), iy);
    if (wy == 0.f) continue;
    for (int ox = xlo; ox <= xhi; ++ox) {
      const float wx = lerp_weight(lerp_of(ox, wi, wo), ix);
      if (wx == 0.f) continue;
      s += wy * wx * g[(((int64_t)b * ho + oy) * wo + ox) * ld_g + c];
    }
  }
  dx[e] = s;
}

__global__ __launch_bounds__(256) void rows_kernel(int mode, int64_t total, int F, float sa, float s1, const float* __restrict__ p, int ld_p,
                                                   const float* __restrict__ q, int ld_q, const float* __restrict__ r, int ld_r,
                                                   float* __restrict__ out, int ld_out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / F;
  const int c = (int)(e - row * F);
  float v;
  if (mode == GW_THERMAL_ROWS_FINALIZE) {
    const float noisy = diffuse(sa, s1, p[row * ld_p + c], q[row * ld_q + c]);
    v = (noisy - s1 * r[row * ld_r + c]) / sa;
  } else if (mode == GW_THERMAL_ROWS_SCALE) {
    v = sa * p[row * ld_p + c];
  } else {
    v = p[row * ld_p + c] + sa * q[row * ld_q + c];
  }
  out[row * ld_out + c] = v;
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + 255) / 256); }

bool fits32(int64_t rows, int64_t ld) { return rows * ld <= INT32_MAX; }

int validate_conv(const gw_thermal_conv_args* a, const char* what) {
  if (!a) return fail(what);
  if (a->batch < 1 || a->in_h < 1 || a->in_w < 1 || a->out_h < 1 || a->out_w < 1 || a->q_h < 1 || a->q_w < 1 || a->cin < 1 ||
      a->cout < 1)
    return set_error(GW_E_BADARG, "gw_thermal_conv: empty geometry");
  if (a->in_scale_h < 1 || a->in_scale_w < 1 || a->out_scale_h < 1 || a->out_scale_w < 1 || a->out_off_h < 0 || a->out_off_w < 0)
    return set_error(GW_E_BADARG, "gw_thermal_conv: bad pixel mapping");
  if (a->out_scale_h * (a->q_h - 1) + a->out_off_h >= a->out_h || a->out_scale_w * (a->q_w - 1) + a->out_off_w >= a->out_w)
    return set_error(GW_E_BADARG, "gw_thermal_conv: the GEMM pixels map outside the output image");
  if (a->ty.n < 1 || a->ty.n > GW_THERMAL_MAX_TAPS || a->tx.n < 1 || a->tx.n > GW_THERMAL_MAX_TAPS)
    return set_error(GW_E_BADARG, "gw_thermal_conv: 1..7 taps per axis");
  if (!a->a || !a->w || !a->out) return set_error(GW_E_BADARG, "gw_thermal_conv: null operand");
  if (a->a_mode < GW_THERMAL_A_PLAIN || a->a_mode > GW_THERMAL_A_DIFFUSE || a->e_mode < GW_THERMAL_E_STORE ||
      a->e_mode > GW_THERMAL_E_DIFFUSE)
    return set_error(GW_E_BADARG, "gw_thermal_conv: unknown operand or epilogue mode");
  if (a->a_mode == GW_THERMAL_A_GN_RELU && (!a->a_scale || !a->a_shift))
    return set_error(GW_E_BADARG, "gw_thermal_conv: GroupNorm load without scale / shift");
  if (a->a_mode == GW_THERMAL_A_DIFFUSE && (!a->eps || a->features < 1 || a->cin > a->features + 2 || a->ld_a < a->features))
    return set_error(GW_E_BADARG, "gw_thermal_conv: diffusion load needs eps, features >= 1 and cin <= features + 2");
  if (a->a_mode != GW_THERMAL_A_DIFFUSE && a->ld_a < a->cin) return set_error(GW_E_BADARG, "gw_thermal_conv: ld_a < cin");
  if (a->e_mode == GW_THERMAL_E_DIFFUSE &&
      (!a->x || !a->eps || a->features != a->cout || a->ld_x < a->cout || !(a->sa > 0.f)))
    return set_error(GW_E_BADARG, "gw_thermal_conv: diffusion epilogue needs x, eps, features == cout and sa > 0");
  if (a->ld_out < a->cout) return set_error(GW_E_BADARG, "gw_thermal_conv: ld_out < cout");
  const int64_t in_rows = (int64_t)a->batch * a->in_h * a->in_w, out_rows = (int64_t)a->batch * a->out_h * a->out_w;
  if (!fits32(in_rows, a->ld_a) || !fits32(out_rows, a->ld_out) || !fits32(out_rows, a->ld_x) ||
      (int64_t)a->batch * a->q_h * a->q_w > INT32_MAX / 2)
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_conv: more than 2^31-1 elements");
  return GW_OK;
}

struct Split {
  int slab_px, slabs;
};

Split split_of(const gw_thermal_conv_args* a) {
  const int64_t M = (int64_t)a->batch * a->q_h * a->q_w;
  const int tiles = ((a->cin + kTile - 1) / kTile) * ((a->cout + kTile - 1) / kTile) * a->ty.n * a->tx.n;
  int want = (2048 + tiles - 1) / tiles;
  want = want < 1 ? 1 : (want > 64 ? 64 : want);
  int64_t px = (M + want - 1) / want;
  px = (px + kStep - 1) / kStep * kStep;
  if (px < 64) px = 64;
  return Split{(int)px, (int)((M + px - 1) / px)};
}

size_t wgrad_bytes(const gw_thermal_conv_args* a) {
  const Split s = split_of(a);
  return (size_t)s.slabs * a->ty.n * a->tx.n * a->cin * a->cout * sizeof(float);
}

int gn_slabs(int hw) { return (hw + kGnSlab - 1) / kGnSlab; }

int validate_gn(int batch, int hw, int C, int groups, const float* x, int ld, const char* what) {
  if (batch < 1 || hw < 1 || C < 1 || groups < 1 || C % groups || !x || ld < C) return set_error(GW_E_BADARG, what);
  if (!fits32((int64_t)batch * hw, ld)) return set_error(GW_E_UNSUPPORTED, what);
  return GW_OK;
}

}  // namespace

extern "C" {

int gw_thermal_conv_forward(const gw_thermal_conv_args* a, void* stream) {
  int rc = validate_conv(a, "gw_thermal_conv_forward: null arguments");
  if (rc != GW_OK) return rc;
  const int64_t M = (int64_t)a->batch * a->q_h * a->q_w;
  const dim3 grid((unsigned)((M + kTile - 1) / kTile), (unsigned)((a->cout + kTile - 1) / kTile));
  hipStream_t s = (hipStream_t)stream;
  const bool ed = a->e_mode == GW_THERMAL_E_DIFFUSE;
  switch (a->a_mode) {
    case GW_THERMAL_A_PLAIN:
      if (ed) hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_PLAIN, GW_THERMAL_E_DIFFUSE>), grid, dim3(256), 0, s, *a);
      else hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_PLAIN, GW_THERMAL_E_STORE>), grid, dim3(256), 0, s, *a);
      break;
    case GW_THERMAL_A_GN_RELU:
      if (ed) hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_GN_RELU, GW_THERMAL_E_DIFFUSE>), grid, dim3(256), 0, s, *a);
      else hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_GN_RELU, GW_THERMAL_E_STORE>), grid, dim3(256), 0, s, *a);
      break;
    default:
      if (ed) hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_DIFFUSE, GW_THERMAL_E_DIFFUSE>), grid, dim3(256), 0, s, *a);
      else hipLaunchKernelGGL((conv_nt_kernel<GW_THERMAL_A_DIFFUSE, GW_THERMAL_E_STORE>), grid, dim3(256), 0, s, *a);
  }
  return check_launch("conv_nt_kernel launch");
}

size_t gw_thermal_conv_wgrad_workspace_bytes(const gw_thermal_conv_args* a) {
  if (validate_conv(a, "gw_thermal_conv_wgrad_workspace_bytes: null arguments") != GW_OK) return 0;
  return wgrad_bytes(a);
}

int gw_thermal_conv_wgrad(const gw_thermal_conv_args* a, void* workspace, size_t workspace_bytes, float* dw, void* stream) {
  int rc = validate_conv(a, "gw_thermal_conv_wgrad: null arguments");
  if (rc != GW_OK) return rc;
  if (!dw) return fail("gw_thermal_conv_wgrad: null dw");
  if (!workspace || workspace_bytes < wgrad_bytes(a))
    return fail("gw_thermal_conv_wgrad: workspace smaller than gw_thermal_conv_wgrad_workspace_bytes");
  const Split sp = split_of(a);
  const int tiles = ((a->cin + kTile - 1) / kTile) * ((a->cout + kTile - 1) / kTile);
  const dim3 grid((unsigned)tiles, (unsigned)sp.slabs, (unsigned)(a->ty.n * a->tx.n));
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  switch (a->a_mode) {
    case GW_THERMAL_A_PLAIN:
      hipLaunchKernelGGL(conv_tn_kernel<GW_THERMAL_A_PLAIN>, grid, dim3(256), 0, s, *a, sp.slab_px, part);
      break;
    case GW_THERMAL_A_GN_RELU:
      hipLaunchKernelGGL(conv_tn_kernel<GW_THERMAL_A_GN_RELU>, grid, dim3(256), 0, s, *a, sp.slab_px, part);
      break;
    default:
      hipLaunchKernelGGL(conv_tn_kernel<GW_THERMAL_A_DIFFUSE>, grid, dim3(256), 0, s, *a, sp.slab_px, part);
  }
  if ((rc = check_launch("conv_tn_kernel launch")) != GW_OK) return rc;
  const int64_t total = (int64_t)a->ty.n * a->tx.n * a->cin * a->cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks_for(total)), dim3(256), 0, s, *a, sp.slabs, (const float*)part, dw);
  return check_launch("wgrad_reduce_kernel launch");
}

size_t gw_thermal_colsum_workspace_bytes(int64_t rows, int32_t cols) {
  if (rows < 1 || cols < 1) return 0;
  return (size_t)((rows + kColSlab - 1) / kColSlab) * cols * sizeof(float);
}

int gw_thermal_colsum(int64_t rows, int32_t cols, const float* g, int32_t ld, void* workspace, size_t workspace_bytes, float* out,
                      void* stream) {
  if (rows < 1 || cols < 1 || !g || ld < cols || !out) return fail("gw_thermal_colsum: bad arguments");
  if (!fits32(rows, ld)) return set_error(GW_E_UNSUPPORTED, "gw_thermal_colsum: more than 2^31-1 elements");
  if (!workspace || workspace_bytes < gw_thermal_colsum_workspace_bytes(rows, cols))
    return fail("gw_thermal_colsum: workspace smaller than gw_thermal_colsum_workspace_bytes");
  const int slabs = (int)((rows + kColSlab - 1) / kColSlab);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((cols + 63) / 64, slabs), dim3(256), 0, s, rows, cols, g, ld, (float*)workspace);
  int rc = check_launch("colsum_partial_kernel launch");
  if (rc != GW_OK) return rc;
  hipLaunchKernelGGL(colsum_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, cols, slabs, (const float*)workspace, out);
  return check_launch("colsum_final_kernel launch");
}

size_t gw_thermal_groupnorm_workspace_bytes(int32_t batch, int32_t hw, int32_t channels, int32_t groups) {
  if (batch < 1 || hw < 1 || channels < 1 || groups < 1) return 0;
  const size_t slabs = (size_t)gn_slabs(hw);
  const size_t fwd = slabs * batch * groups * 3;
  const size_t bwd = 2 * slabs * batch * channels + 2 * (size_t)batch * channels + 2 * (size_t)batch * groups;
  return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

int gw_thermal_groupnorm_forward(int32_t batch, int32_t hw, int32_t channels, int32_t groups, const float* x, int32_t ld_x,
                                 const float* gamma, const float* beta, float eps, void* workspace, size_t workspace_bytes,
                                 float* stats, float* scale, float* shift, void* stream) {
  int rc = validate_gn(batch, hw, channels, groups, x, ld_x, "gw_thermal_groupnorm_forward: bad arguments");
  if (rc != GW_OK) return rc;
  if (!gamma || !beta || !stats || !scale || !shift || !(eps > 0.f)) return fail("gw_thermal_groupnorm_forward: null operand");
  if (!workspace || workspace_bytes < gw_thermal_groupnorm_workspace_bytes(batch, hw, channels, groups))
    return fail("gw_thermal_groupnorm_forward: workspace smaller than gw_thermal_groupnorm_workspace_bytes");
  const int slabs = gn_slabs(hw);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(gn_stats_partial_kernel, dim3(batch * groups, slabs), dim3(256), 0, s, hw, channels, groups, x, ld_x, part);
  if ((rc = check_launch("gn_stats_partial_kernel launch")) != GW_OK) return rc;
  hipLaunchKernelGGL(gn_stats_final_kernel, dim3((batch * groups + 63) / 64), dim3(64), 0, s, batch, channels, groups, slabs,
                     (const float*)part, gamma, beta, eps, stats, scale, shift);
  return check_launch("gn_stats_final_kernel launch");
}

int gw_thermal_groupnorm_backward(int32_t batch, int32_t hw, int32_t channels, int32_t groups, const float* x, int32_t ld_x,
                                  const float* scale, const float* shift, const float* stats, const float* gamma, const float* dy,
                                  int32_t ld_dy, void* workspace, size_t workspace_bytes, float* dx, float* dgamma, float* dbeta,
                                  void* stream) {
  int rc = validate_gn(batch, hw, channels, groups, x, ld_x, "gw_thermal_groupnorm_backward: bad arguments");
  if (rc != GW_OK) return rc;
  if (!scale || !shift || !stats || !gamma || !dy || ld_dy < channels || !dx) return fail("gw_thermal_groupnorm_backward: null operand");
  if (!fits32((int64_t)batch * hw, ld_dy)) return set_error(GW_E_UNSUPPORTED, "gw_thermal_groupnorm_backward: too large");
  if (!workspace || workspace_bytes < gw_thermal_groupnorm_workspace_bytes(batch, hw, channels, groups))
    return fail("gw_thermal_groupnorm_backward: workspace smaller than gw_thermal_groupnorm_workspace_bytes");
  const int slabs = gn_slabs(hw);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  float* sums = part + 2 * (size_t)slabs * batch * channels;
  float* coef = sums + 2 * (size_t)batch * channels;
  const int ct = (channels + 63) / 64;
  hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(batch * ct, slabs), dim3(256), 0, s, batch, hw, channels, groups, x, ld_x, scale, shift,
                     stats, dy, ld_dy, part);
  if ((rc = check_launch("gn_bwd_partial_kernel launch")) != GW_OK) return rc;
  hipLaunchKernelGGL(gn_bwd_final_kernel, dim3(1), dim3(256), 0, s, batch, channels, groups, slabs, (const float*)part, gamma, sums, coef,
                     dgamma, dbeta);
  if ((rc = check_launch("gn_bwd_final_kernel launch")) != GW_OK) return rc;
  const int64_t total = (int64_t)batch * hw * channels;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(blocks_for(total)), dim3(256), 0, s, total, hw, channels, groups, x, ld_x, scale, shift,
                     stats, gamma, dy, ld_dy, (const float*)coef, dx);
  return check_launch("gn_bwd_apply_kernel launch");
}

int gw_thermal_maxpool_forward(int32_t batch, int32_t h, int32_t w, int32_t channels, const float* x, int32_t ld_x,
                               const float* scale, const float* shift, float* out, int32_t ld_out, int32_t* idx, void* stream) {
  if (batch < 1 || h < 1 || w < 1 || channels < 1 || !x || ld_x < channels || !scale || !shift || !out || ld_out < channels || !idx)
    return fail("gw_thermal_maxpool_forward: bad arguments");
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  if (!fits32((int64_t)batch * h * w, ld_x) || !fits32((int64_t)batch * ho * wo, ld_out))
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_maxpool_forward: more than 2^31-1 elements");
  const int64_t total = (int64_t)batch * ho * wo * channels;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, total, h, w, ho, wo, channels, x,
                     ld_x, scale, shift, out, ld_out, idx);
  return check_launch("maxpool_fwd_kernel launch");
}

int gw_thermal_maxpool_backward(int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* idx, const float* g1,
                                int32_t ld_g1, const float* g2, int32_t ld_g2, float* dx, void* stream) {
  if (batch < 1 || h < 1 || w < 1 || channels < 1 || !idx || !g1 || ld_g1 < channels || (g2 && ld_g2 < channels) || !dx)
    return fail("gw_thermal_maxpool_backward: bad arguments");
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  if (!fits32((int64_t)batch * h * w, channels) || !fits32((int64_t)batch * ho * wo, ld_g1) ||
      (g2 && !fits32((int64_t)batch * ho * wo, ld_g2)))
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_maxpool_backward: more than 2^31-1 elements");
  const int64_t total = (int64_t)batch * h * w * channels;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, total, h, w, ho, wo, channels, idx,
                     g1, ld_g1, g2, ld_g2, dx);
  return check_launch("maxpool_bwd_kernel launch");
}

int gw_thermal_resize_forward(int32_t batch, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out, int32_t channels,
                              const float* x, int32_t ld_x, float* out, int32_t ld_out, void* stream) {
  if (batch < 1 || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1 || channels < 1 || !x || ld_x < channels || !out ||
      ld_out < channels)
    return fail("gw_thermal_resize_forward: bad arguments");
  if (!fits32((int64_t)batch * h_in * w_in, ld_x) || !fits32((int64_t)batch * h_out * w_out, ld_out))
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_resize_forward: more than 2^31-1 elements");
  const int64_t total = (int64_t)batch * h_out * w_out * channels;
  hipLaunchKernelGGL(resize_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, total, h_in, w_in, h_out, w_out,
                     channels, x, ld_x, out, ld_out);
  return check_launch("resize_fwd_kernel launch");
}

int gw_thermal_resize_backward(int32_t batch, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out, int32_t channels,
                               const float* g, int32_t ld_g, float* dx, void* stream) {
  if (batch < 1 || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1 || channels < 1 || !g || ld_g < channels || !dx)
    return fail("gw_thermal_resize_backward: bad arguments");
  if (!fits32((int64_t)batch * h_in * w_in, channels) || !fits32((int64_t)batch * h_out * w_out, ld_g))
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_resize_backward: more than 2^31-1 elements");
  const int64_t total = (int64_t)batch * h_in * w_in * channels;
  hipLaunchKernelGGL(resize_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, total, h_in, w_in, h_out, w_out,
                     channels, g, ld_g, dx);
  return check_launch("resize_bwd_kernel launch");
}

int gw_thermal_rows(int32_t mode, int64_t rows, int32_t features, float sa, float s1, const float* p, int32_t ld_p, const float* q,
                    int32_t ld_q, const float* r, int32_t ld_r, float* out, int32_t ld_out, void* stream) {
  if (mode < GW_THERMAL_ROWS_FINALIZE || mode > GW_THERMAL_ROWS_AXPY || rows < 1 || features < 1 || !p || ld_p < features || !out ||
      ld_out < features)
    return fail("gw_thermal_rows: bad arguments");
  if (mode != GW_THERMAL_ROWS_SCALE && (!q || ld_q < features)) return fail("gw_thermal_rows: null q");
  if (mode == GW_THERMAL_ROWS_FINALIZE && (!r || ld_r < features || !(sa > 0.f))) return fail("gw_thermal_rows: null r or sa <= 0");
  if (!fits32(rows, ld_p) || !fits32(rows, ld_out) || !fits32(rows, ld_q > 0 ? ld_q : 1) || !fits32(rows, ld_r > 0 ? ld_r : 1))
    return set_error(GW_E_UNSUPPORTED, "gw_thermal_rows: more than 2^31-1 elements");
  const int64_t total = rows * features;
  hipLaunchKernelGGL(rows_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, mode, total, features, sa, s1, p, ld_p,
                     q, ld_q, r, ld_r, out, ld_out);
  return check_launch("rows_kernel launch");
}

}  // extern "C"
