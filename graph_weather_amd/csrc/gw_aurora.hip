// gw_aurora.hip - EarthSystemLoss of the Aurora models (graph_weather/models/aurora/model.py): the three terms, their
// weighted total and the gradient, without an N x N object.
//
//   spatial term   mean over [N, N, C] of m_ij (e_ic - e_jc)^2, e = pred - target, m_ij = 1 where the raw points i, j lie
//                  closer than 5 degrees.  pair_kernel: one workgroup per 32 rows i walks the 64-row tiles of j in order.  A
//                  tile without a pair inside the radius costs the distance test only; otherwise its e rows are staged in
//                  LDS and every thread (row i, 8 of the 64 j) sums its direct differences channel by channel (no Gram form:
//                  |e_i|^2 + |e_j|^2 - 2 e_i.e_j cancels).  The same pass accumulates G_i = sum_j m_ij (e_i - e_j) in fp64 in
//                  LDS; the gradient is 4 G / (N^2 C) (m is symmetric), so the backward is a scaling.
//   mse, physical  stream_kernel: sums of pred, (pred - target)^2, relu(-pred), relu(pred - 500) per workgroup in fp64;
//                  lat_kernel, which needs the global mean of pred: sum_r relu(pred[r, 0] - w_r mean), w_r = 1 - |lat_r| / 90,
//                  and sum_r [active] w_r for the derivative through the mean.
//   final_kernel   one thread adds every partial in workgroup order in fp64 and forms the four scalars.
//   grad_kernel    d total' / d pred and d target for an upstream gradient on each of the four scalars.
//
//   relu_kernel, row_scale_kernel                a ReLU that follows a LayerNorm; AuroraModel's per-point mask
//   token_mean_kernel / token_mean_grad_kernel   the mean over the tokens of PerceiverProcessor (processor.py) and its gradient
//
//   ordered weight gradients   the training kernels of gw_train.hip / gw_wide.hip add their row slabs with float atomics, whose order
//                  is not fixed; Aurora's backward uses tn_kernel (dW[i, j] = sum_r A[r, i] B[r, j] on fp32 MFMA, the bias gradient as
//                  a column of ones) and ln_dy_kernel / ln_cols_kernel (LayerNorm backward) instead: per-slab partials in the
//                  caller's workspace, added in slab order by slab_sum_kernel.  Gradients are then bitwise reproducible, which
//                  is what lets use_checkpointing reproduce the plain backward bit for bit.
//
// The key-padding mask of PerceiverProcessor's attention is the MASKED form of the attention kernels in gw_fengwu.hip
// (gw_attention_masked_forward / _backward).
//
// fp32 data, no atomics, every sum in one fixed order: equal inputs give bitwise equal results.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kPairRows = 32;    // rows i per workgroup of pair_kernel
constexpr int kPairCols = 64;    // rows j per tile
constexpr int kPairMaxC = 128;   // channels (LDS: 32 x C doubles + 64 x (C + 1) floats)
constexpr int kStreamBlocks = 1024;  // upper bound of the streaming grids
constexpr float kRadius2 = 25.0f;    // (5 degrees)^2
constexpr float kMaxValue = 500.0f;

struct Layout {  // the workspace, in doubles
  int64_t total, rows;  // batch * n * channels, batch * n
  int stream_blocks, lat_blocks, pair_blocks;
  int64_t off_stream, off_lat, off_pair, doubles;  // stream: [blocks][4], lat: [blocks][2], pair: [blocks]
};

Layout layout(int32_t batch, int32_t n, int32_t channels) {
  Layout l;
  l.rows = (int64_t)batch * n;
  l.total = l.rows * channels;
  const int64_t sb = (l.total + 1023) / 1024, lb = (l.rows + 255) / 256;
  l.stream_blocks = (int)(sb < kStreamBlocks ? sb : kStreamBlocks);
  l.lat_blocks = (int)(lb < kStreamBlocks ? lb : kStreamBlocks);
  l.pair_blocks = (n + kPairRows - 1) / kPairRows;
  l.off_stream = 0;
  l.off_lat = l.off_stream + 4 * (int64_t)l.stream_blocks;
  l.off_pair = l.off_lat + 2 * (int64_t)l.lat_blocks;
  l.doubles = l.off_pair + l.pair_blocks;
  return l;
}

size_t pair_lds_bytes(int C) { return (size_t)kPairRows * C * sizeof(double) + (size_t)kPairCols * (C + 1) * sizeof(float); }

// the 256 values of a workgroup added as a fixed tree; the result is valid in thread 0
__device__ inline double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// grid ceil(N / 32), block 256: thread = (row r = tid / 8, column phase jj = tid % 8).
__global__ __launch_bounds__(256) void pair_kernel(int N, int C, const float* __restrict__ pred, const float* __restrict__ target,
                                                   const float* __restrict__ pts, float* __restrict__ G, double* __restrict__ part) {
  extern __shared__ double pair_lds[];
  __shared__ double red[256];
  double* Gacc = pair_lds;                                            // [32][C]
  float* es = reinterpret_cast<float*>(pair_lds + kPairRows * C);     // [64][C + 1]
  const int tid = threadIdx.x, r = tid >> 3, jj = tid & 7, lde = C + 1;
  const int i = blockIdx.x * kPairRows + r;
  const bool row = i < N;
  const float xi = row ? pts[2 * (int64_t)i] : 0.f, yi = row ? pts[2 * (int64_t)i + 1] : 0.f;
  const float* pi = pred + (int64_t)(row ? i : 0) * C;
  const float* ti = target + (int64_t)(row ? i : 0) * C;
  for (int idx = tid; idx < kPairRows * C; idx += 256) Gacc[idx] = 0.0;
  double lsum = 0.0;
  for (int j0 = 0; j0 < N; j0 += kPairCols) {
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int j = j0 + jj + 8 * s;
      if (row && j < N) {
        const float dx = xi - pts[2 * (int64_t)j], dy = yi - pts[2 * (int64_t)j + 1];
        if (dx * dx + dy * dy < kRadius2) m |= 1u << s;
      }
    }
    // also the barrier between the previous tile's readers of es and this tile's writers (and after the zeroing of Gacc)
    if (!__syncthreads_or(m != 0)) continue;
    const int nj = min(kPairCols, N - j0);
    const float* pj = pred + (int64_t)j0 * C;
    const float* tj = target + (int64_t)j0 * C;
    for (int idx = tid; idx < nj * C; idx += 256) {
      const int jr = idx / C;
      es[jr * lde + (idx - jr * C)] = pj[idx] - tj[idx];
    }
    __syncthreads();
    if (__ballot(m != 0) == 0) continue;  // this wave's 8 rows have nothing in the tile (the barriers above are block-uniform)
    for (int c = 0; c < C; ++c) {
      const float ei = row ? pi[c] - ti[c] : 0.f;
      float g = 0.f, l = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if ((m >> s) & 1u) {
          const float d = ei - es[(jj + 8 * s) * lde + c];
          g += d;
          l = fmaf(d, d, l);
        }
      g += __shfl_xor(g, 1);
      g += __shfl_xor(g, 2);
      g += __shfl_xor(g, 4);
      lsum += (double)l;
      if (jj == 0) Gacc[r * C + c] += (double)g;
    }
  }
  const double s = block_sum(lsum, red);  // its first barrier also orders the last additions to Gacc
  if (tid == 0) part[blockIdx.x] = s;
  for (int idx = tid; idx < kPairRows * C; idx += 256) {
    const int rr = idx / C, ii = blockIdx.x * kPairRows + rr;
    if (ii < N) G[(int64_t)ii * C + (idx - rr * C)] = (float)Gacc[idx];
  }
}

// part[block][4] = sums of pred, (pred - target)^2, relu(-pred), relu(pred - 500) over the workgroup's elements
__global__ __launch_bounds__(256) void stream_kernel(int64_t total, const float* __restrict__ pred, const float* __restrict__ target,
                                                     double* __restrict__ part) {
  __shared__ double red[256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const float p = pred[e], d = target ? p - target[e] : 0.f;
    s0 += (double)p;
    s1 += (double)d * (double)d;
    s2 += (double)fmaxf(-p, 0.f);
    s3 += (double)fmaxf(p - kMaxValue, 0.f);
  }
  const double r0 = block_sum(s0, red), r1 = block_sum(s1, red), r2 = block_sum(s2, red), r3 = block_sum(s3, red);
  if (threadIdx.x == 0) {
    double* o = part + 4 * (int64_t)blockIdx.x;
    o[0] = r0, o[1] = r1, o[2] = r2, o[3] = r3;
  }
}

__device__ inline float mean_of(const double* stream_part, int stream_blocks, int64_t total) {
  double s = 0.0;
  for (int b = 0; b < stream_blocks; ++b) s += stream_part[4 * (int64_t)b];
  return (float)(s / (double)total);
}

// part[block][2] = sum_r relu(pred[r, 0] - w_r mean), sum_r [pred[r, 0] - w_r mean > 0] w_r
__global__ __launch_bounds__(256) void lat_kernel(int64_t rows, int C, int64_t total, const float* __restrict__ pred,
                                                  const float* __restrict__ pts, const double* __restrict__ stream_part, int stream_blocks,
                                                  double* __restrict__ part) {
  __shared__ double red[256];
  __shared__ float mean_s;
  if (threadIdx.x == 0) mean_s = mean_of(stream_part, stream_blocks, total);
  __syncthreads();
  const float mean = mean_s;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows; q += (int64_t)gridDim.x * 256) {
    const float w = 1.0f - fabsf(pts[2 * q + 1]) / 90.0f;
    const float v = pred[q * C] - w * mean;
    if (v > 0.f) s0 += (double)v, s1 += (double)w;
  }
  const double r0 = block_sum(s0, red), r1 = block_sum(s1, red);
  if (threadIdx.x == 0) part[2 * (int64_t)blockIdx.x] = r0, part[2 * (int64_t)blockIdx.x + 1] = r1;
}

// out = (total, mse, spatial, physical); stats = (mean of pred, sum_r [active] w_r)
__global__ void final_kernel(Layout l, int N, int C, int spatial, float alpha, float beta, float gamma, const double* __restrict__ ws,
                             float* __restrict__ out, float* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, lat[2] = {0.0, 0.0}, pair = 0.0;
  for (int b = 0; b < l.stream_blocks; ++b)
    for (int k = 0; k < 4; ++k) s[k] += ws[l.off_stream + 4 * (int64_t)b + k];
  for (int b = 0; b < l.lat_blocks; ++b)
    for (int k = 0; k < 2; ++k) lat[k] += ws[l.off_lat + 2 * (int64_t)b + k];
  if (spatial)
    for (int b = 0; b < l.pair_blocks; ++b) pair += ws[l.off_pair + b];
  const double T = (double)l.total;
  // the three scalars are rounded to fp32 where the reference holds fp32 scalars, the total is formed from them
  const float mse = (float)(s[1] / T);
  const float sp = spatial ? (float)(pair / ((double)N * (double)N * (double)C)) : 0.f;
  const float phys = (float)(s[2] / T + s[3] / T + 0.1 * (lat[0] / (double)l.rows));
  out[0] = alpha * mse + beta * sp + gamma * phys;
  out[1] = mse;
  out[2] = sp;
  out[3] = phys;
  stats[0] = mean_of(ws + l.off_stream, l.stream_blocks, l.total);
  stats[1] = (float)lat[1];
}

// gout = the upstream gradients of (total, mse, spatial, physical)
__global__ __launch_bounds__(256) void grad_kernel(int64_t total, int64_t rows, int N, int C, int spatial, float alpha, float beta,
                                                   float gamma, const float* __restrict__ pred, const float* __restrict__ target,
                                                   const float* __restrict__ pts, const float* __restrict__ G,
                                                   const float* __restrict__ stats, const float* __restrict__ gout,
                                                   float* __restrict__ dpred, float* __restrict__ dtarget) {
  const float g_total = gout[0];
  const float a_mse = gout[1] + alpha * g_total, a_sp = gout[2] + beta * g_total, a_ph = gout[3] + gamma * g_total;
  const float mean = stats[0];
  const double T = (double)total;
  const float c_mse = (float)(2.0 * (double)a_mse / T);
  const float c_sp = spatial ? (float)(4.0 * (double)a_sp / ((double)N * (double)N * (double)C)) : 0.f;
  const float c_el = (float)((double)a_ph / T);
  const float c_lat = (float)(0.1 * (double)a_ph / (double)rows);
  const float c_mean = (float)(-0.1 * (double)a_ph * (double)stats[1] / ((double)rows * T));  // through pred.mean()
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / C;
    const int c = (int)(e - q * C);
    const float p = pred[e];
    const float pair = spatial ? c_sp * G[e] : 0.f;
    const float dm = target ? c_mse * (p - target[e]) + pair : pair;
    float ph = c_mean;
    if (p < 0.f) ph -= c_el;
    if (p > kMaxValue) ph += c_el;
    if (c == 0) {
      const float w = 1.0f - fabsf(pts[2 * q + 1]) / 90.0f;
      if (p - w * mean > 0.f) ph += c_lat;
    }
    if (dpred) dpred[e] = dm + ph;
    if (dtarget) dtarget[e] = -dm;
  }
}

// out[b, d] = mean over the tokens s of x[(b, s), d]: one thread per (b, d) walks the tokens in order
__global__ __launch_bounds__(256) void token_mean_kernel(int tokens, int width, const float* __restrict__ x, int64_t ldx,
                                                         float* __restrict__ out, int64_t ldo) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= width) return;
  const float* xb = x + (int64_t)blockIdx.y * tokens * ldx + d;
  double acc = 0.0;  // fp64: thousands of tokens in one chain
  for (int s = 0; s < tokens; ++s) acc += (double)xb[(int64_t)s * ldx];
  out[(int64_t)blockIdx.y * ldo + d] = (float)(acc / (double)tokens);
}

// dx[(b, s), d] = dout[b, d] / tokens
__global__ __launch_bounds__(256) void token_mean_grad_kernel(int64_t rows, int tokens, int width, const float* __restrict__ dout,
                                                              int64_t ldg, float* __restrict__ dx, int64_t ldx) {
  const int64_t total = rows * width;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / width;
    const int d = (int)(e - q * width);
    dx[q * ldx + d] = dout[(q / tokens) * ldg + d] / (float)tokens;
  }
}

// y = max(x, 0) (the ReLU behind a LayerNorm in PointEncoder; a ReLU behind a Linear is that kernel's epilogue)
__global__ __launch_bounds__(256) void relu_kernel(int64_t n, const float* __restrict__ x, float* __restrict__ y) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) y[e] = fmaxf(x[e], 0.f);
}

// out[r, :] = x[r, :] * m[r] (AuroraModel's point mask)
__global__ __launch_bounds__(256) void row_scale_kernel(int64_t rows, int width, const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ m, float* __restrict__ out, int64_t ldo) {
  const int64_t total = rows * width;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / width;
    const int d = (int)(e - q * width);
    out[q * ldo + d] = x[q * ldx + d] * m[q];
  }
}

unsigned grid_for(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// ---- ordered weight gradients ---------------------------------------------------------------------------------------------
constexpr int kSlabRows = 1024;  // rows per partial of tn_kernel
constexpr int kLnSlab = 256;     // rows per partial of ln_cols_kernel
constexpr int kTile = 64, kStep = 16, kLd = kStep + 1;

// part[slab][i][j] = sum over the slab's rows r of A[r, i] B[r, j]; j = n is a column of ones (the column sums of A).
// grid (tiles of i x tiles of j, slabs), block 256: four waves of 16 rows of the 64 x 64 tile, 16 reduction rows per LDS stage;
// the accumulator is folded into a second one every 8 stages so that the fp32 sum grows in blocks, not as one long chain.
__global__ __launch_bounds__(256) void tn_kernel(int m, int n, int64_t rows, const float* __restrict__ A, int64_t lda,
                                                 const float* __restrict__ B, int64_t ldb, float* __restrict__ part) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int J = n + 1, tj = (J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const int64_t r_begin = (int64_t)blockIdx.y * kSlabRows, r_end = r_begin + kSlabRows < rows ? r_begin + kSlabRows : rows;
  f32x4 acc[4], tot[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = tot[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int stage = 0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kStep, ++stage) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int rr = (tid >> 6) + 4 * s, x = tid & 63;
      const int64_t r = r0 + rr;
      float av = 0.f, bv = 0.f;
      if (r < r_end) {
        if (i0 + x < m) av = ldg1(A + r * lda + i0 + x);
        if (j0 + x < n) bv = ldg1(B + r * ldb + j0 + x);
        else if (j0 + x == n) bv = 1.f;
      }
      As[x * kLd + rr] = av;
      Bs[x * kLd + rr] = bv;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kStep / 4; ++ks) {
      const float av = As[(16 * wave + l16) * kLd + 4 * ks + kq];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[(16 * jt + l16) * kLd + 4 * ks + kq], acc[jt], 0, 0, 0);
    }
    if ((stage & 7) == 7) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) tot[jt] += acc[jt], acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    tot[jt] += acc[jt];
    const int j = j0 + 16 * jt + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * wave + 4 * kq + r;
      if (i < m && j < J) stg1(part + ((int64_t)blockIdx.y * m + i) * J + j, tot[jt][r]);
    }
  }
}

// c[i, j] = sum_s part[s][i][j] (s ascending) for j < n; colsum[i] = the same of column n
__global__ __launch_bounds__(256) void tn_sum_kernel(int S, int m, int n, const float* __restrict__ part, float* __restrict__ c,
                                                     int64_t ldc, float* __restrict__ colsum) {
  const int J = n + 1;
  const int64_t total = (int64_t)m * J;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / J), j = (int)(e - (int64_t)i * J);
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += (double)ldg1(part + (int64_t)sl * total + e);
    if (j < n) stg1(c + i * ldc + j, (float)s);
    else if (colsum != nullptr) stg1(colsum + i, (float)s);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One wave per row: dy = rstd (g - mean(g) - xhat mean(g xhat)), g = dn gamma, xhat = (y - mean) rstd; (mean, rstd) kept per row.
__global__ __launch_bounds__(256) void ln_dy_kernel(int64_t rows, int width, const float* __restrict__ dn, int64_t ld_dn,
                                                    const float* __restrict__ y, int64_t ld_y, const float* __restrict__ gamma,
                                                    float* __restrict__ dy, int64_t ld_dy, float* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* yr = y + r * ld_y;
  const float* gr = dn + r * ld_dn;
  float s = 0.f;
  for (int c = lane; c < width; c += 64) s += ldg1(yr + c);
  const float mean = wave_sum(s) / (float)width;
  float v = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float d = ldg1(yr + c) - mean;
    v = fmaf(d, d, v);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)width + 1e-5f);
  float a = 0.f, b = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float g = ldg1(gr + c) * ldg1(gamma + c), xh = (ldg1(yr + c) - mean) * rstd;
    a += g;
    b = fmaf(g, xh, b);
  }
  a = wave_sum(a) / (float)width;
  b = wave_sum(b) / (float)width;
  for (int c = lane; c < width; c += 64) {
    const float g = ldg1(gr + c) * ldg1(gamma + c), xh = (ldg1(yr + c) - mean) * rstd;
    stg1(dy + r * ld_dy + c, rstd * (g - a - xh * b));
  }
  if (lane == 0) stat[2 * r] = mean, stat[2 * r + 1] = rstd;
}

// part[slab][0][c] = sum over the slab's rows of dn xhat, part[slab][1][c] = of dn; one thread per column walks the rows in order
__global__ __launch_bounds__(256) void ln_cols_kernel(int64_t rows, int width, const float* __restrict__ dn, int64_t ld_dn,
                                                      const float* __restrict__ y, int64_t ld_y, const float* __restrict__ stat,
                                                      float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const int64_t r_begin = (int64_t)blockIdx.y * kLnSlab, r_end = r_begin + kLnSlab < rows ? r_begin + kLnSlab : rows;
  double dg = 0.0, db = 0.0;  // fp64: a chain of 256 fp32 additions would cost more than the float32 reference's pairwise sums
  for (int64_t r = r_begin; r < r_end; ++r) {
    const float g = ldg1(dn + r * ld_dn + c);
    dg += (double)(g * ((ldg1(y + r * ld_y + c) - stat[2 * r]) * stat[2 * r + 1]));
    db += (double)g;
  }
  part[((int64_t)blockIdx.y * 2) * width + c] = (float)dg;
  part[((int64_t)blockIdx.y * 2 + 1) * width + c] = (float)db;
}

__global__ __launch_bounds__(256) void ln_sum_kernel(int S, int width, const float* __restrict__ part, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * width) return;
  double s = 0.0;
  for (int sl = 0; sl < S; ++sl) s += (double)ldg1(part + (int64_t)sl * 2 * width + e);
  if (e < width) dgamma[e] = (float)s;
  else dbeta[e - width] = (float)s;
}

size_t tn_bytes(int m, int n, int64_t rows) { return (size_t)((rows + kSlabRows - 1) / kSlabRows) * (size_t)m * (size_t)(n + 1) * sizeof(float); }
size_t ln_bytes(int64_t rows, int width) {
  return ((size_t)2 * (size_t)rows + (size_t)((rows + kLnSlab - 1) / kLnSlab) * 2 * (size_t)width) * sizeof(float);
}
bool tn_ok(int m, int n, int64_t rows) {
  return m >= 1 && n >= 1 && rows >= 1 && (rows + kSlabRows - 1) / kSlabRows <= 65535 && m < (1 << 24) && n < (1 << 24);
}
bool ln_ok(int64_t rows, int width) {
  return rows >= 1 && width >= 1 && width <= 4096 && (rows + kLnSlab - 1) / kLnSlab <= 65535 && rows < ((int64_t)1 << 31);
}

int check_dims(const char* msg, int32_t batch, int32_t n, int32_t channels, int32_t spatial) {
  if (batch < 1 || n < 1 || channels < 1 || (int64_t)batch * n * channels >= ((int64_t)1 << 40)) return failf(GW_E_BADARG, msg);
  if (spatial && batch != 1) return failf(GW_E_BADARG, msg);
  return GW_OK;
}

}  // namespace

extern "C" {

size_t gw_earth_loss_workspace_bytes(int32_t batch, int32_t n, int32_t channels) {
  if (check_dims("gw_earth_loss_workspace_bytes: bad arguments", batch, n, channels, 0) != GW_OK) return 0;
  return (size_t)layout(batch, n, channels).doubles * sizeof(double);
}

int gw_earth_loss_forward(int32_t batch, int32_t n, int32_t channels, const float* pred, const float* target, const float* points,
                          int32_t spatial, float alpha, float beta, float gamma, void* workspace, size_t workspace_bytes, float* out,
                          float* pair_rows, float* stats, void* stream) {
  const char* bad = "gw_earth_loss_forward: bad arguments";
  if (!pred || !points || !workspace || !out || !stats || (spatial && (!target || !pair_rows))) return failf(GW_E_BADARG, bad);
  if (int rc = check_dims(bad, batch, n, channels, spatial)) return rc;
  if (((uintptr_t)workspace & 7) != 0) return failf(GW_E_BADARG, bad);
  const Layout l = layout(batch, n, channels);
  if (workspace_bytes < (size_t)l.doubles * sizeof(double)) return failf(GW_E_BADARG, "gw_earth_loss_forward: bad arguments (workspace)");
  if (spatial && channels > kPairMaxC)
    return failf(GW_E_UNSUPPORTED, "gw_earth_loss_forward: the spatial term takes at most 128 channels");
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stream_kernel, dim3((unsigned)l.stream_blocks), dim3(256), 0, st, l.total, pred, target, ws + l.off_stream);
  if (int rc = check_launch("stream_kernel launch")) return rc;
  hipLaunchKernelGGL(lat_kernel, dim3((unsigned)l.lat_blocks), dim3(256), 0, st, l.rows, (int)channels, l.total, pred, points,
                     ws + l.off_stream, l.stream_blocks, ws + l.off_lat);
  if (int rc = check_launch("lat_kernel launch")) return rc;
  if (spatial) {
    const size_t lds = pair_lds_bytes(channels);
    static DeviceOnce once;
    if (once.first())
      (void)hipFuncSetAttribute((const void*)pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pair_lds_bytes(kPairMaxC));
    hipLaunchKernelGGL(pair_kernel, dim3((unsigned)l.pair_blocks), dim3(256), lds, st, (int)n, (int)channels, pred, target, points,
                       pair_rows, ws + l.off_pair);
    if (int rc = check_launch("pair_kernel launch")) return rc;
  }
  hipLaunchKernelGGL(final_kernel, dim3(1), dim3(64), 0, st, l, (int)n, (int)channels, (int)spatial, alpha, beta, gamma,
                     (const double*)ws, out, stats);
  return check_launch("final_kernel launch");
}

int gw_earth_loss_backward(int32_t batch, int32_t n, int32_t channels, const float* pred, const float* target, const float* points,
                           int32_t spatial, float alpha, float beta, float gamma, const float* pair_rows, const float* stats,
                           const float* gout, float* dpred, float* dtarget, void* stream) {
  const char* bad = "gw_earth_loss_backward: bad arguments";
  if (!pred || !points || !stats || !gout || (!dpred && !dtarget) || (dtarget && !target) || (spatial && (!target || !pair_rows)))
    return failf(GW_E_BADARG, bad);
  if (int rc = check_dims(bad, batch, n, channels, spatial)) return rc;
  const Layout l = layout(batch, n, channels);
  hipLaunchKernelGGL(grad_kernel, dim3((unsigned)l.stream_blocks), dim3(256), 0, (hipStream_t)stream, l.total, l.rows, (int)n,
                     (int)channels, (int)spatial, alpha, beta, gamma, pred, target, points, pair_rows, stats, gout, dpred, dtarget);
  return check_launch("grad_kernel launch");
}

int gw_token_mean_forward(int32_t batch, int32_t tokens, int32_t width, const float* x, int32_t ld_x, float* out, int32_t ld_out,
                          void* stream) {
  if (!x || !out || batch < 1 || batch > 65535 || tokens < 1 || width < 1 || ld_x < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_token_mean_forward: bad arguments");
  hipLaunchKernelGGL(token_mean_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     (int)tokens, (int)width, x, (int64_t)ld_x, out, (int64_t)ld_out);
  return check_launch("token_mean_kernel launch");
}

int gw_token_mean_backward(int32_t batch, int32_t tokens, int32_t width, const float* dout, int32_t ld_dout, float* dx, int32_t ld_dx,
                           void* stream) {
  if (!dout || !dx || batch < 1 || batch > 65535 || tokens < 1 || width < 1 || ld_dout < width || ld_dx < width)
    return failf(GW_E_BADARG, "gw_token_mean_backward: bad arguments");
  const int64_t rows = (int64_t)batch * tokens, blocks = (rows * width + 255) / 256;
  hipLaunchKernelGGL(token_mean_grad_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, rows,
                     (int)tokens, (int)width, dout, (int64_t)ld_dout, dx, (int64_t)ld_dx);
  return check_launch("token_mean_grad_kernel launch");
}

size_t gw_gemm_tn_ordered_workspace_bytes(int32_t m, int32_t n, int64_t rows) {
  if (!tn_ok(m, n, rows)) {
    failf(GW_E_BADARG, "gw_gemm_tn_ordered_workspace_bytes: bad arguments");
    return 0;
  }
  return tn_bytes(m, n, rows);
}

int gw_gemm_tn_ordered(int32_t m, int32_t n, int64_t rows, const float* a, int32_t lda, const float* b, int32_t ldb, void* workspace,
                       size_t workspace_bytes, float* c, int32_t ldc, float* colsum, void* stream) {
  if (!a || !b || !c || !workspace || !tn_ok(m, n, rows) || lda < m || ldb < n || ldc < n)
    return failf(GW_E_BADARG, "gw_gemm_tn_ordered: bad arguments");
  if (workspace_bytes < tn_bytes(m, n, rows)) return failf(GW_E_BADARG, "gw_gemm_tn_ordered: bad arguments (workspace)");
  const int slabs = (int)((rows + kSlabRows - 1) / kSlabRows);
  const int64_t tiles = (int64_t)((m + kTile - 1) / kTile) * ((n + 1 + kTile - 1) / kTile);
  hipLaunchKernelGGL(tn_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, (int)m, (int)n, rows, a,
                     (int64_t)lda, b, (int64_t)ldb, (float*)workspace);
  if (int rc = check_launch("tn_kernel launch")) return rc;
  hipLaunchKernelGGL(tn_sum_kernel, dim3(grid_for((int64_t)m * (n + 1))), dim3(256), 0, (hipStream_t)stream, slabs, (int)m, (int)n,
                     (const float*)workspace, c, (int64_t)ldc, colsum);
  return check_launch("tn_sum_kernel launch");
}

size_t gw_layernorm_backward_ordered_workspace_bytes(int64_t rows, int32_t width) {
  if (!ln_ok(rows, width)) {
    failf(GW_E_BADARG, "gw_layernorm_backward_ordered_workspace_bytes: bad arguments");
    return 0;
  }
  return ln_bytes(rows, width);
}

int gw_layernorm_backward_ordered(int64_t rows, int32_t width, const float* dn, int32_t ld_dn, const float* y, int32_t ld_y,
                                  const float* gamma, void* workspace, size_t workspace_bytes, float* dy, int32_t ld_dy, float* dgamma,
                                  float* dbeta, void* stream) {
  if (!dn || !y || !gamma || !workspace || !dy || !dgamma || !dbeta || !ln_ok(rows, width) || ld_dn < width || ld_y < width ||
      ld_dy < width)
    return failf(GW_E_BADARG, "gw_layernorm_backward_ordered: bad arguments");
  if (workspace_bytes < ln_bytes(rows, width)) return failf(GW_E_BADARG, "gw_layernorm_backward_ordered: bad arguments (workspace)");
  float* stat = (float*)workspace;
  float* part = stat + 2 * rows;
  const int slabs = (int)((rows + kLnSlab - 1) / kLnSlab);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ln_dy_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, (int)width, dn, (int64_t)ld_dn, y,
                     (int64_t)ld_y, gamma, dy, (int64_t)ld_dy, stat);
  if (int rc = check_launch("ln_dy_kernel launch")) return rc;
  hipLaunchKernelGGL(ln_cols_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)slabs), dim3(256), 0, st, rows, (int)width, dn,
                     (int64_t)ld_dn, y, (int64_t)ld_y, (const float*)stat, part);
  if (int rc = check_launch("ln_cols_kernel launch")) return rc;
  hipLaunchKernelGGL(ln_sum_kernel, dim3((unsigned)((2 * width + 255) / 256)), dim3(256), 0, st, slabs, (int)width, (const float*)part,
                     dgamma, dbeta);
  return check_launch("ln_sum_kernel launch");
}

int gw_relu_forward(int64_t n, const float* x, float* y, void* stream) {
  if (!x || !y || n < 0) return failf(GW_E_BADARG, "gw_relu_forward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(relu_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, x, y);
  return check_launch("relu_kernel launch");
}

int gw_row_scale(int64_t rows, int32_t width, const float* x, int32_t ld_x, const float* row_factor, float* out, int32_t ld_out,
                 void* stream) {
  if (!x || !row_factor || !out || rows < 0 || width < 1 || ld_x < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_row_scale: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(row_scale_kernel, dim3(grid_for(rows * width)), dim3(256), 0, (hipStream_t)stream, rows, (int)width, x,
                     (int64_t)ld_x, row_factor, out, (int64_t)ld_out);
  return check_launch("row_scale_kernel launch");
}

}  // extern "C"
