// gw_convnd.hip - the convolution towers of WeatherMesh (graph_weather/models/weathermesh/layers.py: ConvDownBlock, ConvUpBlock;
// encoder.py: to_latent; decoder.py: split): convolutions with kernel 1 or 3, padding k / 2 and stride 1 or 2 per axis as implicit
// GEMMs on v_mfma_f32_16x16x4_f32, BatchNorm statistics, the residual tail gelu(bn2(y2) + bn_skip(ys)) with its backward, and
// 2 x bilinear upsampling.  All fp32, no atomics, every sum in one fixed order: every launch is bitwise repeatable.
//
// A volume is addressed by three strides as in gw_conv3d.hip - element (b, c, voxel v = (z H + y) W + x) at b sb + c sc + v sv -
// so NCDHW tensors, channels-last rows and depth slices of a larger buffer are read and written where they lie.  A 2-D
// convolution is the depth-1 case with kd = 1.  Per axis an input of length L gives an output of length (L - 1) / s + 1, for the
// padded 3-tap and for the unpadded 1-tap convolution alike.
//
//   conv_kernel<false>  out(b, j, o) = bias[j] + sum_{c, k} w[j, c, k] A(x(b, c, o s + k - p))                    rows o, reduction (c, k)
//       A is the identity (PLAIN) or gelu(x scale[c] + shift[c]) (BN_GELU: the BatchNorm + GELU in front of conv2 is applied on
//       load and its result never stored); the zero padding is a bounds predicate applied after A.
//   conv_kernel<true>   dx(b, c, i) = sum_{j, k} w[j, c, k] dout(b, j, (i + p - k) / s)                           rows i of ONE parity class
//       With stride 2 only the taps k = (i + p) mod 2 (mod 2) reach an output voxel: the input voxels are split by the parity of
//       each strided axis and every class is one launch whose reduction runs over that class's own taps (stride 2, kernel 3:
//       one tap for even i, two for odd i; kernel 1: one tap for even i, none for odd i, which stores zeros) - no MFMA step
//       multiplies a structural zero.
//   wgrad_kernel        dw[j, (c, k)] = sum_o dout(b, j, o) A(x(b, c, o s + k - p)), db[j] = sum_o dout(b, j, o)    reduction o
//       per slab of kSlab output voxels into the caller's workspace; reduce_kernel adds the slabs in order.
//
// Tiles are those of gw_conv3d.hip: 64 x 64 with 16 reduction indices per LDS stage (rows padded to 17 floats), four waves of 16 rows, four independent accumulators per wave (the four column tiles: the 40-cycle dependent latency
// of the 16x16x4 form is covered by the other three), folded into a second set every 8 stages so that a
// reduction of channels x 27 taps is a sum of short fp32 chains.  All volume offsets are 64-bit.
//
// BatchNorm statistics: one workgroup per channel, two passes (mean, then the centred sum of squares), accumulated in double
// per thread and combined in a fixed tree - never E[x^2] - E[x]^2.  The statistics of a BatchNorm are one table [4][C]:
// scale = gamma rstd, shift = beta - mean scale, mean, rstd.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kSlab = 1024;  // output voxels per weight-gradient partial
constexpr int kTile = 64, kStep = 16, kLd = kStep + 1;
constexpr int kRed = 1024;  // threads of a per-channel reduction workgroup

struct Vol {
  float* p;
  int64_t sb, sc, sv;
};

// One axis of a launch.  Row index i of the launch is the result's coordinate i rs + par; tap t is kernel index k = kb + t ks.
//   forward / weight gradient: rs = 1, par = 0, the source coordinate is i s + k - p (source length Ls)
//   data gradient:             rs = s, par = the class's parity, the source coordinate is (i s + par + p - k) / s (exact)
struct Axis {
  int n;       // rows along this axis
  int Ld, Ls;  // lengths of the result and of the source
  int s, p, rs, par;
  int nt, kb, ks;
};

struct ConvArgs {
  Axis ax[3];
  int B, M;  // M = B n0 n1 n2 rows
  int R;     // reduction length: source channels x nt0 nt1 nt2
  int J;     // result channels
  int KH, KW;
  Vol src, dst;
  const float* w;  // w(j, c, k) at w[j wsj + c wsc + (k0 KH + k1) KW + k2]
  int64_t wsj, wsc;
  const float* bias;
  const float* a_scale;  // BN_GELU: [source channels]; NULL: PLAIN
  const float* a_shift;
  int accumulate;  // dst += the result
};

struct WgradArgs {
  Axis ax[3];  // forward axes: n = output length
  int B, M;
  Vol a;  // dout, read at the output voxel
  int I;  // cout
  Vol src;
  int J;  // cin x taps; column J of the result is the bias gradient
  const float* a_scale;
  const float* a_shift;
  float* part;  // [slabs][I][J + 1]
};

struct Row {
  int b, c0, c1, c2;  // batch element and the result's coordinates
  bool ok;
};

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

__device__ __forceinline__ Row row_of(const Axis (&ax)[3], int M, int m) {
  Row q;
  q.ok = m < M;
  int v = q.ok ? m : 0;
  const int n12 = ax[1].n * ax[2].n, nv = ax[0].n * n12;
  q.b = v / nv;
  v -= q.b * nv;
  const int i0 = v / n12;
  v -= i0 * n12;
  const int i1 = v / ax[2].n, i2 = v - i1 * ax[2].n;
  q.c0 = i0 * ax[0].rs + ax[0].par, q.c1 = i1 * ax[1].rs + ax[1].par, q.c2 = i2 * ax[2].rs + ax[2].par;
  return q;
}

struct Tap {
  int c, k0, k1, k2;
};

__device__ __forceinline__ Tap tap_of(const Axis (&ax)[3], int r) {
  const int t12 = ax[1].nt * ax[2].nt, T = ax[0].nt * t12;
  Tap t;
  t.c = r / T;
  int u = r - t.c * T;
  const int t0 = u / t12;
  u -= t0 * t12;
  const int t1 = u / ax[2].nt, t2 = u - t1 * ax[2].nt;
  t.k0 = ax[0].kb + t0 * ax[0].ks, t.k1 = ax[1].kb + t1 * ax[1].ks, t.k2 = ax[2].kb + t2 * ax[2].ks;
  return t;
}

template <bool kGrad>
__device__ __forceinline__ int src_coord(const Axis& x, int c, int k) {
  return kGrad ? (c + x.p - k) / x.s : c * x.s + k - x.p;  // kGrad: the numerator is never negative where s = 2 (see the header)
}

// A(src(b, c, source voxel of (row q, tap t))), zero outside the volume
template <bool kGrad>
__device__ __forceinline__ float operand(const Axis (&ax)[3], const Vol& s, const float* a_scale, const float* a_shift, const Row& q,
                                         const Tap& t) {
  const int z = src_coord<kGrad>(ax[0], q.c0, t.k0), y = src_coord<kGrad>(ax[1], q.c1, t.k1), x = src_coord<kGrad>(ax[2], q.c2, t.k2);
  if (!q.ok || z < 0 || z >= ax[0].Ls || y < 0 || y >= ax[1].Ls || x < 0 || x >= ax[2].Ls) return 0.f;
  float v = ldg1(s.p + q.b * s.sb + t.c * s.sc + ((int64_t)(z * ax[1].Ls + y) * ax[2].Ls + x) * s.sv);
  if (a_scale != nullptr) v = gelu_f(fmaf(v, ldg1(a_scale + t.c), ldg1(a_shift + t.c)));
  return v;
}

__device__ __forceinline__ void mfma_stage(f32x4 (&acc)[4], const float* As, const float* Bs, int wave, int l16, int kq) {
#pragma unroll
  for (int ks = 0; ks < kStep / 4; ++ks) {
    const float av = As[(16 * wave + l16) * kLd + 4 * ks + kq];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
      acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[(16 * jt + l16) * kLd + 4 * ks + kq], acc[jt], 0, 0, 0);
  }
}

__device__ __forceinline__ void fold(f32x4 (&tot)[4], f32x4 (&acc)[4]) {
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) tot[jt] += acc[jt], acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// grid (tiles of m) x (tiles of j), flattened; block 256.  A thread stages the taps of ONE row (tid & 63) for the whole sweep.
template <bool kGrad>
__global__ __launch_bounds__(256) void conv_kernel(const ConvArgs a) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int tj = (a.J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const Row q = row_of(a.ax, a.M, i0 + (tid & 63));
  f32x4 acc[4], tot[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = tot[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int stage = 0;
  for (int r0 = 0; r0 < a.R; r0 += kStep, ++stage) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int rr = (tid >> 6) + 4 * s, r = r0 + rr;
      float val = 0.f;
      if (r < a.R) val = operand<kGrad>(a.ax, a.src, a.a_scale, a.a_shift, q, tap_of(a.ax, r));
      As[(tid & 63) * kLd + rr] = val;
    }
    for (int idx = tid; idx < kTile * kStep; idx += 256) {
      const int j = idx >> 4, rr = idx & 15, r = r0 + rr;
      float val = 0.f;
      if (j0 + j < a.J && r < a.R) {
        const Tap t = tap_of(a.ax, r);
        val = ldg1(a.w + (j0 + j) * a.wsj + t.c * a.wsc + ((t.k0 * a.KH + t.k1) * a.KW + t.k2));
      }
      Bs[j * kLd + rr] = val;
    }
    __syncthreads();
    mfma_stage(acc, As, Bs, wave, l16, kq);
    if ((stage & 7) == 7) fold(tot, acc);
  }
  fold(tot, acc);
  // tot[jt][r] = C[i0 + 16 wave + 4 kq + r][j0 + 16 jt + l16]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const Row o = row_of(a.ax, a.M, i0 + 16 * wave + 4 * kq + r);
    if (!o.ok) continue;
    float* row = a.dst.p + o.b * a.dst.sb + ((int64_t)(o.c0 * a.ax[1].Ld + o.c1) * a.ax[2].Ld + o.c2) * a.dst.sv;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l16;
      if (j >= a.J) continue;
      float v = tot[jt][r] + (a.bias != nullptr ? ldg1(a.bias + j) : 0.f);
      if (a.accumulate) v += ldg1(row + j * a.dst.sc);
      stg1(row + j * a.dst.sc, v);
    }
  }
}

// grid (tiles of i x tiles of j, slabs); block 256
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs a) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int J = a.J + 1;
  const int tj = (J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const int m_begin = (int)blockIdx.y * kSlab, m_end = min(m_begin + kSlab, a.M);
  const int nv = a.ax[0].n * a.ax[1].n * a.ax[2].n;
  f32x4 acc[4], tot[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = tot[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int stage = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += kStep, ++stage) {
    __syncthreads();
    const int rr = tid & 15, m = m0 + rr;  // the output voxel of this thread in both operands
    const bool mok = m < m_end;
    const Row q = row_of(a.ax, a.M, mok ? m : a.M);
    const int v = mok ? m - q.b * nv : 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int x = (tid >> 4) + 16 * s;
      const int i = i0 + x, j = j0 + x;
      float av = 0.f, bv = 0.f;
      if (mok) {
        if (i < a.I) av = ldg1(a.a.p + q.b * a.a.sb + i * a.a.sc + v * a.a.sv);
        if (j < a.J) bv = operand<false>(a.ax, a.src, a.a_scale, a.a_shift, q, tap_of(a.ax, j));
        else if (j < J) bv = 1.f;
      }
      As[x * kLd + rr] = av;
      Bs[x * kLd + rr] = bv;
    }
    __syncthreads();
    mfma_stage(acc, As, Bs, wave, l16, kq);
    if ((stage & 7) == 7) fold(tot, acc);
  }
  fold(tot, acc);
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int j = j0 + 16 * jt + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * wave + 4 * kq + r;
      if (i < a.I && j < J) stg1(a.part + ((int64_t)blockIdx.y * a.I + i) * J + j, tot[jt][r]);
    }
  }
}

// dw[i, j] = sum_s part[s][i][j] (s ascending, j < DJ); db[i] = the same of column DJ (db may be NULL)
__global__ __launch_bounds__(256) void reduce_kernel(int S, int DI, int DJ, const float* __restrict__ part, float* __restrict__ dw,
                                                     float* __restrict__ db) {
  const int J = DJ + 1;
  const int64_t nw = (int64_t)DI * DJ, total = nw + (db != nullptr ? DI : 0);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int i, j;
    if (e < nw) i = (int)(e / DJ), j = (int)(e - (int64_t)i * DJ);
    else i = (int)(e - nw), j = DJ;
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += (double)ldg1(part + ((int64_t)sl * DI + i) * J + j);
    if (e < nw) stg1(dw + e, (float)s);
    else stg1(db + (e - nw), (float)s);
  }
}

// ---- per-channel reductions: workgroup of kRed threads, every thread a double, combined in a fixed tree ----------------------
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();  // red may still be read from the previous call
  red[tid] = v;
  __syncthreads();
  for (int half = kRed / 2; half > 0; half >>= 1) {
    if (tid < half) red[tid] += red[tid + half];
    __syncthreads();
  }
  return red[0];
}

struct BnArgs {
  int B, C;
  int64_t V;
  Vol x;
  const float* gamma;
  const float* beta;
  float eps, momentum;
  int training;
  float* running_mean;
  float* running_var;
  float* stats;  // [4][C]: scale, shift, mean, rstd
};

// grid C; block kRed
__global__ __launch_bounds__(kRed) void bn_stats_kernel(const BnArgs a) {
  __shared__ double red[kRed];
  const int c = blockIdx.x, tid = threadIdx.x;
  float mean, rstd;
  if (a.training) {
    const int64_t n = (int64_t)a.B * a.V;
    const float* base = a.x.p + c * a.x.sc;
    double s = 0.0;
    for (int64_t e = tid; e < n; e += kRed) {
      const int64_t b = e / a.V, v = e - b * a.V;
      s += (double)ldg1(base + b * a.x.sb + v * a.x.sv);
    }
    const double mu = block_sum(s, red) / (double)n;
    s = 0.0;
    for (int64_t e = tid; e < n; e += kRed) {
      const int64_t b = e / a.V, v = e - b * a.V;
      const double d = (double)ldg1(base + b * a.x.sb + v * a.x.sv) - mu;
      s += d * d;
    }
    const double m2 = block_sum(s, red), var = m2 / (double)n;
    mean = (float)mu, rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    if (tid == 0 && a.running_mean != nullptr) {
      const double unbiased = n > 1 ? m2 / (double)(n - 1) : var;
      stg1(a.running_mean + c, (float)((1.0 - a.momentum) * (double)ldg1(a.running_mean + c) + a.momentum * mu));
      stg1(a.running_var + c, (float)((1.0 - a.momentum) * (double)ldg1(a.running_var + c) + a.momentum * unbiased));
    }
  } else {
    mean = ldg1(a.running_mean + c);
    rstd = (float)(1.0 / sqrt((double)ldg1(a.running_var + c) + (double)a.eps));
  }
  if (tid == 0) {
    const float scale = ldg1(a.gamma + c) * rstd;
    stg1(a.stats + c, scale);
    stg1(a.stats + a.C + c, ldg1(a.beta + c) - mean * scale);
    stg1(a.stats + 2 * a.C + c, mean);
    stg1(a.stats + 3 * a.C + c, rstd);
  }
}

struct TailArgs {
  int B, C;
  int64_t V;
  int training;
  Vol y2, ys, g, o2, os;  // ys.p NULL: one BatchNorm only (bn1); g: the incoming gradient (backward) or the output (forward)
  const float* st2;       // [4][C]
  const float* sts;
  float* sums;            // [4][C]: sum dz, sum dz zhat2, sum dz, sum dz zhats
};

__device__ __forceinline__ int64_t at(const Vol& t, int64_t b, int c, int64_t v) { return b * t.sb + c * t.sc + v * t.sv; }

__device__ __forceinline__ float tail_pre(const TailArgs& a, int64_t b, int c, int64_t v, float& y2, float& ys) {
  y2 = ldg1(a.y2.p + at(a.y2, b, c, v));
  float u = fmaf(y2, ldg1(a.st2 + c), ldg1(a.st2 + a.C + c));
  ys = 0.f;
  if (a.ys.p != nullptr) {
    ys = ldg1(a.ys.p + at(a.ys, b, c, v));
    u += fmaf(ys, ldg1(a.sts + c), ldg1(a.sts + a.C + c));
  }
  return u;
}

// out = gelu(y2 s2 + t2 + ys ss + ts); grid-stride over (b, c, v), v fastest
__global__ __launch_bounds__(256) void tail_forward_kernel(const TailArgs a) {
  const int64_t total = (int64_t)a.B * a.C * a.V;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t v = e % a.V, bc = e / a.V;
    const int c = (int)(bc % a.C);
    const int64_t b = bc / a.C;
    float y2, ys;
    const float u = tail_pre(a, b, c, v, y2, ys);
    stg1(a.g.p + at(a.g, b, c, v), gelu_f(u));
  }
}

// grid C; block kRed: sums[0] = sum dz, sums[1] = sum dz zhat2, sums[2] = sum dz, sums[3] = sum dz zhats, dz = g gelu'(u)
__global__ __launch_bounds__(kRed) void tail_reduce_kernel(const TailArgs a) {
  __shared__ double red[kRed];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t n = (int64_t)a.B * a.V;
  const float m2 = ldg1(a.st2 + 2 * a.C + c), r2 = ldg1(a.st2 + 3 * a.C + c);
  const bool two = a.ys.p != nullptr;
  const float ms = two ? ldg1(a.sts + 2 * a.C + c) : 0.f, rs = two ? ldg1(a.sts + 3 * a.C + c) : 0.f;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t e = tid; e < n; e += kRed) {
    const int64_t b = e / a.V, v = e - b * a.V;
    float y2, ys;
    const float u = tail_pre(a, b, c, v, y2, ys);
    const float dz = ldg1(a.g.p + at(a.g, b, c, v)) * gelu_grad_f(u);
    s0 += (double)dz;
    s1 += (double)dz * (double)((y2 - m2) * r2);
    s2 += (double)dz * (double)((ys - ms) * rs);
  }
  s0 = block_sum(s0, red), s1 = block_sum(s1, red);
  if (two) s2 = block_sum(s2, red);
  if (tid == 0) {
    stg1(a.sums + c, (float)s0);
    stg1(a.sums + a.C + c, (float)s1);
    if (two) stg1(a.sums + 2 * a.C + c, (float)s0), stg1(a.sums + 3 * a.C + c, (float)s2);
  }
}

// dy2 = s2 (dz - mean(dz) - zhat2 mean(dz zhat2)) in training, s2 dz in eval; dys likewise
__global__ __launch_bounds__(256) void tail_apply_kernel(const TailArgs a) {
  const int64_t total = (int64_t)a.B * a.C * a.V;
  const float inv_n = 1.f / (float)((int64_t)a.B * a.V);
  const bool two = a.ys.p != nullptr;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t v = e % a.V, bc = e / a.V;
    const int c = (int)(bc % a.C);
    const int64_t b = bc / a.C;
    float y2, ys;
    const float u = tail_pre(a, b, c, v, y2, ys);
    const float dz = ldg1(a.g.p + at(a.g, b, c, v)) * gelu_grad_f(u);
    float d2 = dz, ds = dz;
    if (a.training) {
      const float mdz = ldg1(a.sums + c) * inv_n;
      d2 = dz - mdz - (y2 - ldg1(a.st2 + 2 * a.C + c)) * ldg1(a.st2 + 3 * a.C + c) * (ldg1(a.sums + a.C + c) * inv_n);
      if (two) ds = dz - mdz - (ys - ldg1(a.sts + 2 * a.C + c)) * ldg1(a.sts + 3 * a.C + c) * (ldg1(a.sums + 3 * a.C + c) * inv_n);
    }
    stg1(a.o2.p + at(a.o2, b, c, v), d2 * ldg1(a.st2 + c));
    if (two) stg1(a.os.p + at(a.os, b, c, v), ds * ldg1(a.sts + c));
  }
}

// ---- 2 x bilinear upsampling of the last two axes (align_corners = False) -----------------------------------------------
struct UpArgs {
  int B, C, D, H, W;  // the SOURCE's lengths; the upsampled volume is [D, 2 H, 2 W]
  Vol lo, hi;
};

// out[2 i] = 0.25 x[i - 1] + 0.75 x[i], out[2 i + 1] = 0.75 x[i] + 0.25 x[i + 1], indices clamped
__global__ __launch_bounds__(256) void up_forward_kernel(const UpArgs a) {
  const int H2 = 2 * a.H, W2 = 2 * a.W;
  const int64_t plane = (int64_t)H2 * W2, total = (int64_t)a.B * a.C * a.D * plane;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ox = (int)(e % W2);
    int64_t t = e / W2;
    const int oy = (int)(t % H2);
    t /= H2;
    const int z = (int)(t % a.D);
    t /= a.D;
    const int c = (int)(t % a.C);
    const int64_t b = t / a.C;
    const int iy = oy >> 1, ix = ox >> 1;
    const int ya = (oy & 1) ? iy : max(iy - 1, 0), yb = (oy & 1) ? min(iy + 1, a.H - 1) : iy;
    const int xa = (ox & 1) ? ix : max(ix - 1, 0), xb = (ox & 1) ? min(ix + 1, a.W - 1) : ix;
    const float wya = (oy & 1) ? 0.75f : 0.25f, wxa = (ox & 1) ? 0.75f : 0.25f;
    const float* src = a.lo.p + b * a.lo.sb + c * a.lo.sc;
    const int64_t ra = (int64_t)(z * a.H + ya) * a.W, rb = (int64_t)(z * a.H + yb) * a.W;
    const float top = wxa * ldg1(src + (ra + xa) * a.lo.sv) + (1.f - wxa) * ldg1(src + (ra + xb) * a.lo.sv);
    const float bot = wxa * ldg1(src + (rb + xa) * a.lo.sv) + (1.f - wxa) * ldg1(src + (rb + xb) * a.lo.sv);
    stg1(a.hi.p + b * a.hi.sb + c * a.hi.sc + ((int64_t)(z * H2 + oy) * W2 + ox) * a.hi.sv, wya * top + (1.f - wya) * bot);
  }
}

// The weight with which upsampled index 2 i - 1 + t (t = 0 .. 3) reads source index i on an axis of length L: 0.25, 0.75, 0.75,
// 0.25, with the clamped reads of the two borders added (upsampled 0 reads x[0] twice, upsampled 2 L - 1 reads x[L - 1] twice)
__device__ __forceinline__ float up_weight(int i, int t, int L) {
  if (t == 0) return i >= 1 ? 0.25f : 0.f;
  if (t == 1) return i == 0 ? 1.f : 0.75f;
  if (t == 2) return i == L - 1 ? 1.f : 0.75f;
  return i <= L - 2 ? 0.25f : 0.f;
}

// gather form: every source voxel adds the upsampled voxels that read it, in one fixed order
__global__ __launch_bounds__(256) void up_backward_kernel(const UpArgs a) {
  const int H2 = 2 * a.H, W2 = 2 * a.W;
  const int64_t plane = (int64_t)a.H * a.W, total = (int64_t)a.B * a.C * a.D * plane;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ix = (int)(e % a.W);
    int64_t t = e / a.W;
    const int iy = (int)(t % a.H);
    t /= a.H;
    const int z = (int)(t % a.D);
    t /= a.D;
    const int c = (int)(t % a.C);
    const int64_t b = t / a.C;
    const float* g = a.hi.p + b * a.hi.sb + c * a.hi.sc;
    float s = 0.f;
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
      const float wy = up_weight(iy, ty, a.H);
      const int oy = 2 * iy - 1 + ty;
      if (wy == 0.f) continue;
      float rowsum = 0.f;
#pragma unroll
      for (int tx = 0; tx < 4; ++tx) {
        const float wx = up_weight(ix, tx, a.W);
        const int ox = 2 * ix - 1 + tx;
        if (wx != 0.f) rowsum += wx * ldg1(g + ((int64_t)(z * H2 + oy) * W2 + ox) * a.hi.sv);
      }
      s += wy * rowsum;
    }
    stg1(a.lo.p + b * a.lo.sb + c * a.lo.sc + ((int64_t)(z * a.H + iy) * a.W + ix) * a.lo.sv, s);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
struct Geo {
  int B, cin, cout;
  int L[3], Lo[3], k[3], s[3];
  int64_t Mo;  // B x output voxels
  int T;       // taps
  int slabs;
};

int geometry(Geo& g, const char* what, const int32_t* geo) {
  static char msg[160];
  bool bad = geo == nullptr;
  if (!bad) {
    g.B = geo[0], g.cin = geo[1], g.cout = geo[2];
    bad = g.B <= 0 || g.cin <= 0 || g.cout <= 0;
    for (int i = 0; i < 3; ++i) {
      g.L[i] = geo[3 + i], g.k[i] = geo[6 + i], g.s[i] = geo[9 + i];
      bad = bad || g.L[i] <= 0 || (g.k[i] != 1 && g.k[i] != 3) || (g.s[i] != 1 && g.s[i] != 2);
    }
  }
  if (bad) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  int64_t vi = g.B, vo = g.B;
  g.T = 1;
  for (int i = 0; i < 3; ++i) g.Lo[i] = (g.L[i] - 1) / g.s[i] + 1, vi *= g.L[i], vo *= g.Lo[i], g.T *= g.k[i];
  const int64_t lim = ((int64_t)1 << 31) - 2 * kTile - kSlab;
  const int64_t cmax = g.cin > g.cout ? g.cin : g.cout;
  const int64_t tiles = ((vi + kTile - 1) / kTile) * ((cmax * g.T + 1 + kTile - 1) / kTile);
  if (vi >= lim || cmax * g.T >= lim || tiles >= lim) {
    snprintf(msg, sizeof msg, "%s: size exceeds int32", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  g.Mo = vo;
  g.slabs = (int)((vo + kSlab - 1) / kSlab);
  if (g.slabs > 65535) {
    snprintf(msg, sizeof msg, "%s: more than 65535 x %d output voxels", what, kSlab);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  return GW_OK;
}

size_t wgrad_bytes(const Geo& g) { return (size_t)g.slabs * g.cout * ((size_t)g.cin * g.T + 1) * sizeof(float); }

Vol vol(const float* p, const int64_t* st) { return Vol{const_cast<float*>(p), st[0], st[1], st[2]}; }

void forward_axes(Axis (&ax)[3], const Geo& g) {
  for (int i = 0; i < 3; ++i) ax[i] = Axis{g.Lo[i], g.Lo[i], g.L[i], g.s[i], g.k[i] / 2, 1, 0, g.k[i], 0, 1};
}

int elementwise_blocks(int64_t total) {
  const int64_t blocks = (total + 255) / 256;
  return (int)(blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks));
}

int tail_args(TailArgs& a, const char* what, int32_t batch, int32_t channels, int64_t voxels, const float* y2, const int64_t* stride_y2,
              const float* st2, const float* ys, const int64_t* stride_ys, const float* sts) {
  static char msg[160];
  if (batch <= 0 || channels <= 0 || voxels <= 0 || !y2 || !stride_y2 || !st2 || (ys != nullptr && (!stride_ys || !sts))) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  a.B = batch, a.C = channels, a.V = voxels, a.y2 = vol(y2, stride_y2), a.st2 = st2, a.sts = sts;
  a.ys = ys != nullptr ? vol(ys, stride_ys) : Vol{nullptr, 0, 0, 0};
  return GW_OK;
}

}  // namespace

extern "C" {

size_t gw_convnd_workspace_bytes(const int32_t* geo) {
  Geo g;
  if (geometry(g, "gw_convnd_workspace_bytes", geo) != GW_OK) return 0;
  return wgrad_bytes(g);
}

int gw_convnd_forward(const int32_t* geo, int32_t a_mode, const float* x, const int64_t* stride_x, const float* a_scale,
                      const float* a_shift, const float* weight, const float* bias, float* out, const int64_t* stride_out,
                      void* stream) {
  const bool bn = a_mode == GW_CONVND_A_BN_GELU;
  if (!x || !stride_x || !weight || !out || !stride_out || (a_mode != GW_CONVND_A_PLAIN && !bn) || (bn && (!a_scale || !a_shift)))
    return failf(GW_E_BADARG, "gw_convnd_forward: bad arguments");
  Geo g;
  if (int rc = geometry(g, "gw_convnd_forward", geo)) return rc;
  ConvArgs a = {};
  forward_axes(a.ax, g);
  a.B = g.B, a.M = (int)g.Mo, a.R = g.cin * g.T, a.J = g.cout, a.KH = g.k[1], a.KW = g.k[2];
  a.src = vol(x, stride_x), a.dst = vol(out, stride_out), a.w = weight, a.wsj = (int64_t)g.cin * g.T, a.wsc = g.T, a.bias = bias;
  a.a_scale = bn ? a_scale : nullptr, a.a_shift = bn ? a_shift : nullptr;
  const int64_t tiles = (int64_t)((a.M + kTile - 1) / kTile) * ((a.J + kTile - 1) / kTile);
  hipLaunchKernelGGL(conv_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("conv_kernel (forward) launch");
}

int gw_convnd_dgrad(const int32_t* geo, const float* dout, const int64_t* stride_dout, const float* weight, float* dx,
                    const int64_t* stride_dx, int32_t accumulate, void* stream) {
  if (!dout || !stride_dout || !weight || !dx || !stride_dx) return failf(GW_E_BADARG, "gw_convnd_dgrad: bad arguments");
  Geo g;
  if (int rc = geometry(g, "gw_convnd_dgrad", geo)) return rc;
  int classes[3];
  for (int i = 0; i < 3; ++i) classes[i] = g.s[i];
  for (int p0 = 0; p0 < classes[0]; ++p0)
    for (int p1 = 0; p1 < classes[1]; ++p1)
      for (int p2 = 0; p2 < classes[2]; ++p2) {
        const int par[3] = {p0, p1, p2};
        ConvArgs a = {};
        int64_t rows = g.B;
        int taps = 1;
        for (int i = 0; i < 3; ++i) {
          Axis& x = a.ax[i];
          x.Ld = g.L[i], x.Ls = g.Lo[i], x.s = g.s[i], x.p = g.k[i] / 2, x.rs = g.s[i], x.par = par[i];
          x.n = (g.L[i] - par[i] + g.s[i] - 1) / g.s[i];  // coordinates par, par + s, ... below L
          if (g.s[i] == 1) x.nt = g.k[i], x.kb = 0, x.ks = 1;
          else if (g.k[i] == 3) x.nt = par[i] ? 2 : 1, x.kb = par[i] ? 0 : 1, x.ks = 2;  // k = i + 1 (mod 2)
          else x.nt = par[i] ? 0 : 1, x.kb = 0, x.ks = 1;                                 // k = 0 reaches the even voxels only
          rows *= x.n, taps *= x.nt;
        }
        if (rows == 0) continue;  // an axis of length 1 has no odd class
        a.B = g.B, a.M = (int)rows, a.R = g.cout * taps, a.J = g.cin, a.KH = g.k[1], a.KW = g.k[2];
        a.src = vol(dout, stride_dout), a.dst = vol(dx, stride_dx), a.w = weight, a.wsj = g.T, a.wsc = (int64_t)g.cin * g.T;
        a.accumulate = accumulate != 0;
        if (taps == 0)  // tap_of divides by the tap counts: a class no tap reaches stores zeros (or keeps dst) with one dummy tap
          for (int i = 0; i < 3; ++i) a.ax[i].nt = a.ax[i].nt ? a.ax[i].nt : 1;
        const int64_t tiles = (int64_t)((a.M + kTile - 1) / kTile) * ((a.J + kTile - 1) / kTile);
        hipLaunchKernelGGL(conv_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
        if (int rc = check_launch("conv_kernel (data gradient) launch")) return rc;
      }
  return GW_OK;
}

int gw_convnd_wgrad(const int32_t* geo, int32_t a_mode, const float* x, const int64_t* stride_x, const float* a_scale,
                    const float* a_shift, const float* dout, const int64_t* stride_dout, void* workspace, size_t workspace_bytes,
                    float* dweight, float* dbias, void* stream) {
  const bool bn = a_mode == GW_CONVND_A_BN_GELU;
  if (!x || !stride_x || !dout || !stride_dout || !dweight || (a_mode != GW_CONVND_A_PLAIN && !bn) || (bn && (!a_scale || !a_shift)))
    return failf(GW_E_BADARG, "gw_convnd_wgrad: bad arguments");
  Geo g;
  if (int rc = geometry(g, "gw_convnd_wgrad", geo)) return rc;
  if (!workspace || workspace_bytes < wgrad_bytes(g)) return failf(GW_E_BADARG, "gw_convnd_wgrad: bad arguments (workspace)");
  WgradArgs a = {};
  forward_axes(a.ax, g);
  a.B = g.B, a.M = (int)g.Mo, a.a = vol(dout, stride_dout), a.I = g.cout, a.src = vol(x, stride_x), a.J = g.cin * g.T;
  a.a_scale = bn ? a_scale : nullptr, a.a_shift = bn ? a_shift : nullptr, a.part = (float*)workspace;
  const int64_t tiles = (int64_t)((a.I + kTile - 1) / kTile) * ((a.J + 1 + kTile - 1) / kTile);
  hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)tiles, (unsigned)g.slabs), dim3(256), 0, (hipStream_t)stream, a);
  if (int rc = check_launch("wgrad_kernel launch")) return rc;
  const int64_t total = (int64_t)a.I * a.J + a.I, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, g.slabs, a.I,
                     a.J, (const float*)workspace, dweight, dbias);
  return check_launch("reduce_kernel launch");
}

int gw_convnd_bn_stats(int32_t batch, int32_t channels, int64_t voxels, int32_t training, const float* x, const int64_t* stride_x,
                       const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* stats, void* stream) {
  if (batch <= 0 || channels <= 0 || voxels <= 0 || !gamma || !beta || !stats || (training && (!x || !stride_x)) ||
      (!training && (!running_mean || !running_var)) || (running_mean == nullptr) != (running_var == nullptr))
    return failf(GW_E_BADARG, "gw_convnd_bn_stats: bad arguments");
  BnArgs a = {};
  a.B = batch, a.C = channels, a.V = voxels, a.gamma = gamma, a.beta = beta, a.eps = eps, a.momentum = momentum;
  a.training = training != 0, a.running_mean = running_mean, a.running_var = running_var, a.stats = stats;
  if (training) a.x = vol(x, stride_x);
  hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)channels), dim3(kRed), 0, (hipStream_t)stream, a);
  return check_launch("bn_stats_kernel launch");
}

int gw_convnd_tail_forward(int32_t batch, int32_t channels, int64_t voxels, const float* y2, const int64_t* stride_y2, const float* st2,
                           const float* ys, const int64_t* stride_ys, const float* sts, float* out, const int64_t* stride_out,
                           void* stream) {
  TailArgs a = {};
  if (int rc = tail_args(a, "gw_convnd_tail_forward", batch, channels, voxels, y2, stride_y2, st2, ys, stride_ys, sts)) return rc;
  if (!out || !stride_out) return failf(GW_E_BADARG, "gw_convnd_tail_forward: bad arguments");
  a.g = vol(out, stride_out);
  hipLaunchKernelGGL(tail_forward_kernel, dim3((unsigned)elementwise_blocks((int64_t)batch * channels * voxels)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("tail_forward_kernel launch");
}

int gw_convnd_tail_backward(int32_t batch, int32_t channels, int64_t voxels, int32_t training, const float* dout,
                            const int64_t* stride_dout, const float* y2, const int64_t* stride_y2, const float* st2, const float* ys,
                            const int64_t* stride_ys, const float* sts, float* sums, float* dy2, const int64_t* stride_dy2, float* dys,
                            const int64_t* stride_dys, void* stream) {
  TailArgs a = {};
  if (int rc = tail_args(a, "gw_convnd_tail_backward", batch, channels, voxels, y2, stride_y2, st2, ys, stride_ys, sts)) return rc;
  if (!dout || !stride_dout || !sums || !dy2 || !stride_dy2 || (ys != nullptr && (!dys || !stride_dys)))
    return failf(GW_E_BADARG, "gw_convnd_tail_backward: bad arguments");
  a.training = training != 0, a.g = vol(dout, stride_dout), a.sums = sums, a.o2 = vol(dy2, stride_dy2);
  if (ys != nullptr) a.os = vol(dys, stride_dys);
  hipLaunchKernelGGL(tail_reduce_kernel, dim3((unsigned)channels), dim3(kRed), 0, (hipStream_t)stream, a);
  if (int rc = check_launch("tail_reduce_kernel launch")) return rc;
  hipLaunchKernelGGL(tail_apply_kernel, dim3((unsigned)elementwise_blocks((int64_t)batch * channels * voxels)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("tail_apply_kernel launch");
}

int gw_convnd_upsample2x(int32_t batch, int32_t channels, int32_t d, int32_t h, int32_t w, int32_t backward, const float* x,
                         const int64_t* stride_x, float* out, const int64_t* stride_out, void* stream) {
  if (batch <= 0 || channels <= 0 || d <= 0 || h <= 0 || w <= 0 || !x || !stride_x || !out || !stride_out)
    return failf(GW_E_BADARG, "gw_convnd_upsample2x: bad arguments");
  if ((int64_t)d * h * w * 4 >= ((int64_t)1 << 31)) return failf(GW_E_UNSUPPORTED, "gw_convnd_upsample2x: volume exceeds int32");
  UpArgs a = {};
  a.B = batch, a.C = channels, a.D = d, a.H = h, a.W = w;
  const int64_t lo = (int64_t)batch * channels * d * h * w;
  if (backward) {  // x: the gradient of the upsampled volume, out: the source's
    a.hi = vol(x, stride_x), a.lo = vol(out, stride_out);
    hipLaunchKernelGGL(up_backward_kernel, dim3((unsigned)elementwise_blocks(lo)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("up_backward_kernel launch");
  }
  a.lo = vol(x, stride_x), a.hi = vol(out, stride_out);
  hipLaunchKernelGGL(up_forward_kernel, dim3((unsigned)elementwise_blocks(4 * lo)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("up_forward_kernel launch");
}

}  // extern "C"
