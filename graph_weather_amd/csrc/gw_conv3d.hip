// gw_conv3d.hip - the 3 x 3 x 3 convolutions (stride 1, padding 1) of the Aurora models (graph_weather/models/aurora/
// encoder.py: Swin3DEncoder.conv1 = Conv3d; decoder.py: Decoder3D.deconv1 = ConvTranspose3d) as implicit GEMMs on
// v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate).  No im2col buffer: the 27 taps are read from the volume where it lies and
// the zero padding is a bounds predicate.
//
// A volume is addressed by three strides - element (b, c, voxel v = (z H + y) W + x) lies at b sb + c sc + v sv - so NCDHW
// tensors (sb = C V, sc = V, sv = 1) and channels-last rows [(b, v), C] (sb = V ld, sc = 1, sv = ld) are both read and written
// as they lie: Swin3DEncoder's convolution writes the rows its LayerNorm reads, there is no "b c d h w -> b d h w c" copy.
//
// With off(t) = (kz - 1, ky - 1, kx - 1) of tap t = (kz 3 + ky) 3 + kx, all six products are two kernels:
//
//   data_kernel   dst(b, j, v) = bias[j] + sum_{c, t} W(j, c, t) src(b, c, v + sign off(t))       C[m, j], reduction (c, t)
//       Conv3d forward            sign +, W(j, c, t) = weight[j, c, t]      ConvTranspose3d data gradient   the same, no bias
//       ConvTranspose3d forward   sign -, W(j, c, t) = weight[c, j, t]      Conv3d data gradient            the same, no bias
//   wgrad_kernel  dW(i, (c, t)) = sum_m a(m, i) src(m, c, v + off(t))                             C[i, (c, t)], reduction m
//       Conv3d           a = dout, src = x:  dweight [cout, cin, 27]; dbias = the column of ones appended to the view
//       ConvTranspose3d  a = x, src = dout:  dweight [cin, cout, 27]; dbias = the row of ones appended to a, at the centre tap
//     The voxels are split into slabs of kSlab; every slab writes a partial into the caller's workspace and reduce_kernel
//     adds the partials in slab order: no atomics, bitwise reproducible.
//
// Tiles are 64 x 64 with 16 reduction indices per LDS stage, four waves of 16 rows each; the accumulator is folded into a
// second one every 8 stages, so that a long reduction (96 channels x 27 taps, 1024 voxels) is a sum of short fp32 chains and
// not one long one.  All volume offsets are 64-bit.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kSlab = 1024;  // voxels per weight-gradient partial
constexpr int kTile = 64, kStep = 16, kLd = kStep + 1;
constexpr int kTaps = 27, kCentre = 13;

struct Vol {
  float* p;
  int64_t sb, sc, sv;
};

struct Geo {
  int B, D, H, W;
  int V;  // D H W
  int M;  // B V
};

struct DataArgs {
  Geo g;
  int sign;        // +1: tap t reads v + off(t); -1: v - off(t)
  Vol src;
  int R;           // reduction length: source channels x 27
  const float* w;  // W(j, c, t) at w[j wsj + c wsc + t]
  int64_t wsj, wsc;
  const float* bias;  // [J] or NULL
  Vol dst;
  int J;
};

struct WgradArgs {
  Geo g;
  Vol a;         // rows of the result: channel i of a(m, i), unshifted
  int I;         // channels of a
  int ones_row;  // 1: row i = I of the result is the sums of the view's columns
  Vol src;       // the view, read at v + off(t)
  int J;         // channels of src x 27
  int ones_col;  // 1: column j = J of the result is the sums of a's channels
  float* part;   // [slabs][I + ones_row][J + ones_col]
};

struct Voxel {
  int b, z, y, x;
  bool ok;
};

__device__ __forceinline__ Voxel voxel_of(const Geo& g, int m) {
  Voxel q;
  q.ok = m < g.M;
  const int mm = q.ok ? m : 0;
  q.b = mm / g.V;
  int v = mm - q.b * g.V;
  q.z = v / (g.H * g.W);
  v -= q.z * g.H * g.W;
  q.y = v / g.W;
  q.x = v - q.y * g.W;
  return q;
}

// src(b, c, voxel q + sign off(t)), zero outside the volume
__device__ __forceinline__ float tap(const Geo& g, const Vol& s, const Voxel& q, int c, int t, int sign) {
  const int kz = t / 9, ky = (t - 9 * kz) / 3, kx = t - 9 * kz - 3 * ky;
  const int z = q.z + sign * (kz - 1), y = q.y + sign * (ky - 1), x = q.x + sign * (kx - 1);
  if (!q.ok || z < 0 || z >= g.D || y < 0 || y >= g.H || x < 0 || x >= g.W) return 0.f;
  return ldg1(s.p + q.b * s.sb + c * s.sc + ((int64_t)(z * g.H + y) * g.W + x) * s.sv);
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

// grid (tiles of m) x (tiles of j), flattened; block 256.  A thread stages the taps of ONE voxel (tid & 63) for the whole sweep.
__global__ __launch_bounds__(256) void data_kernel(const DataArgs a) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int tj = (a.J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const Voxel q = voxel_of(a.g, i0 + (tid & 63));
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
      if (r < a.R) {
        const int c = r / kTaps;
        val = tap(a.g, a.src, q, c, r - c * kTaps, a.sign);
      }
      As[(tid & 63) * kLd + rr] = val;
    }
    for (int idx = tid; idx < kTile * kStep; idx += 256) {
      const int j = idx >> 4, rr = idx & 15, r = r0 + rr;
      float val = 0.f;
      if (j0 + j < a.J && r < a.R) {
        const int c = r / kTaps;
        val = ldg1(a.w + (j0 + j) * a.wsj + c * a.wsc + (r - c * kTaps));
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
    const int m = i0 + 16 * wave + 4 * kq + r;
    if (m >= a.g.M) continue;
    const int b = m / a.g.V, v = m - b * a.g.V;
    float* row = a.dst.p + b * a.dst.sb + v * a.dst.sv;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l16;
      if (j < a.J) stg1(row + j * a.dst.sc, tot[jt][r] + (a.bias != nullptr ? ldg1(a.bias + j) : 0.f));
    }
  }
}

// grid (tiles of i x tiles of j, slabs); block 256
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs a) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int I = a.I + a.ones_row, J = a.J + a.ones_col;
  const int tj = (J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const int m_begin = (int)blockIdx.y * kSlab, m_end = min(m_begin + kSlab, a.g.M);
  f32x4 acc[4], tot[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = tot[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int stage = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += kStep, ++stage) {
    __syncthreads();
    const int rr = tid & 15, m = m0 + rr;  // the voxel of this thread in both stages
    const bool mok = m < m_end;
    const Voxel q = voxel_of(a.g, mok ? m : a.g.M);
    const int v = mok ? m - q.b * a.g.V : 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int x = (tid >> 4) + 16 * s;
      const int i = i0 + x, j = j0 + x;
      float av = 0.f, bv = 0.f;
      if (mok) {
        if (i < a.I) av = ldg1(a.a.p + q.b * a.a.sb + i * a.a.sc + v * a.a.sv);
        else if (i < I) av = 1.f;
        if (j < a.J) {
          const int c = j / kTaps;
          bv = tap(a.g, a.src, q, c, j - c * kTaps, 1);
        } else if (j < J) {
          bv = 1.f;
        }
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
      if (i < I && j < J) stg1(a.part + ((int64_t)blockIdx.y * I + i) * J + j, tot[jt][r]);
    }
  }
}

// dw[i, j] = sum_s part[s][i][j] (s ascending); db from the ones column (db[i]) or the ones row at the centre taps (db[j / 27])
__global__ __launch_bounds__(256) void reduce_kernel(int S, int DI, int DJ, int ones_row, int ones_col, const float* __restrict__ part,
                                                     float* __restrict__ dw, float* __restrict__ db) {
  const int I = DI + ones_row, J = DJ + ones_col;
  const int nb = ones_col ? DI : DJ / kTaps;
  const int64_t nw = (int64_t)DI * DJ, total = nw + nb;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int i, j;
    if (e < nw) {
      i = (int)(e / DJ), j = (int)(e - (int64_t)i * DJ);
    } else if (ones_col) {
      i = (int)(e - nw), j = DJ;
    } else {
      i = DI, j = (int)(e - nw) * kTaps + kCentre;
    }
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += (double)ldg1(part + ((int64_t)sl * I + i) * J + j);
    if (e < nw) stg1(dw + e, (float)s);
    else stg1(db + (e - nw), (float)s);
  }
}

int geometry(Geo& g, int& slabs, const char* what, int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w) {
  static char msg[160];
  if (batch <= 0 || cin <= 0 || cout <= 0 || d <= 0 || h <= 0 || w <= 0) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  const int64_t v = (int64_t)d * h * w, m = (int64_t)batch * v, lim = ((int64_t)1 << 31) - 2 * kTile - kSlab;
  const int64_t cmax = cin > cout ? cin : cout;
  const int64_t tiles = ((m + kTile - 1) / kTile) * ((cmax + kTile - 1) / kTile);
  if (m >= lim || cmax * kTaps >= lim || tiles >= lim) {
    snprintf(msg, sizeof msg, "%s: size exceeds int32", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  g.B = batch, g.D = d, g.H = h, g.W = w, g.V = (int)v, g.M = (int)m;
  slabs = (g.M + kSlab - 1) / kSlab;
  if (slabs > 65535) {
    snprintf(msg, sizeof msg, "%s: more than 65535 x %d voxels", what, kSlab);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  return GW_OK;
}

size_t workspace_bytes(int slabs, int cin, int cout, bool transposed) {
  const size_t i = (size_t)(transposed ? cin : cout) + 1, j = (size_t)(transposed ? cout : cin) * kTaps + 1;
  return (size_t)slabs * i * j * sizeof(float);
}

Vol vol(const float* p, const int64_t* st) { return Vol{const_cast<float*>(p), st[0], st[1], st[2]}; }

int launch_data(const DataArgs& a, const char* what, void* stream) {
  const int64_t tiles = (int64_t)((a.g.M + kTile - 1) / kTile) * ((a.J + kTile - 1) / kTile);
  hipLaunchKernelGGL(data_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(what);
}

}  // namespace

extern "C" {

size_t gw_conv3d_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed) {
  Geo g;
  int slabs;
  if (geometry(g, slabs, "gw_conv3d_workspace_bytes", batch, cin, cout, d, h, w) != GW_OK) return 0;
  return workspace_bytes(slabs, cin, cout, transposed != 0);
}

int gw_conv3d_forward(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed, const float* x,
                      const int64_t* stride_x, const float* weight, const float* bias, float* out, const int64_t* stride_out,
                      void* stream) {
  if (!x || !stride_x || !weight || !out || !stride_out) return failf(GW_E_BADARG, "gw_conv3d_forward: bad arguments");
  DataArgs a = {};
  int slabs;
  if (int rc = geometry(a.g, slabs, "gw_conv3d_forward", batch, cin, cout, d, h, w)) return rc;
  a.src = vol(x, stride_x), a.R = cin * kTaps, a.w = weight, a.bias = bias, a.dst = vol(out, stride_out), a.J = cout;
  if (transposed) a.sign = -1, a.wsj = kTaps, a.wsc = (int64_t)cout * kTaps;  // weight [cin, cout, 27]
  else a.sign = 1, a.wsj = (int64_t)cin * kTaps, a.wsc = kTaps;               // weight [cout, cin, 27]
  return launch_data(a, "data_kernel (forward) launch", stream);
}

int gw_conv3d_backward(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed, const float* x,
                       const int64_t* stride_x, const float* weight, const float* dout, const int64_t* stride_dout, void* workspace,
                       size_t workspace_bytes_, float* dx, const int64_t* stride_dx, float* dweight, float* dbias, void* stream) {
  const char* bad = "gw_conv3d_backward: bad arguments";
  if (!x || !stride_x || !weight || !dout || !stride_dout || (dweight == nullptr) != (dbias == nullptr) || (!dx && !dweight) ||
      (dx && !stride_dx))
    return failf(GW_E_BADARG, bad);
  Geo g;
  int slabs;
  if (int rc = geometry(g, slabs, "gw_conv3d_backward", batch, cin, cout, d, h, w)) return rc;
  const bool tr = transposed != 0;
  if (dweight != nullptr && (!workspace || workspace_bytes_ < workspace_bytes(slabs, cin, cout, tr)))  // before anything is launched
    return failf(GW_E_BADARG, "gw_conv3d_backward: bad arguments (workspace)");
  if (dx != nullptr) {  // the other convolution over dout, no bias
    DataArgs a = {};
    a.g = g, a.src = vol(dout, stride_dout), a.R = cout * kTaps, a.w = weight, a.dst = vol(dx, stride_dx), a.J = cin;
    if (tr) a.sign = 1, a.wsj = (int64_t)cout * kTaps, a.wsc = kTaps;  // dx(b, i, v) = sum_{o, t} weight[i, o, t] dout(b, o, v + off)
    else a.sign = -1, a.wsj = kTaps, a.wsc = (int64_t)cin * kTaps;     // dx(b, c, v) = sum_{o, t} weight[o, c, t] dout(b, o, v - off)
    if (int rc = launch_data(a, "data_kernel (data gradient) launch", stream)) return rc;
  }
  if (dweight != nullptr) {
    WgradArgs a = {};
    a.g = g, a.part = (float*)workspace;
    if (tr) a.a = vol(x, stride_x), a.I = cin, a.ones_row = 1, a.src = vol(dout, stride_dout), a.J = cout * kTaps, a.ones_col = 0;
    else a.a = vol(dout, stride_dout), a.I = cout, a.ones_row = 0, a.src = vol(x, stride_x), a.J = cin * kTaps, a.ones_col = 1;
    const int I = a.I + a.ones_row, J = a.J + a.ones_col;
    const int64_t tiles = (int64_t)((I + kTile - 1) / kTile) * ((J + kTile - 1) / kTile);
    hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, a);
    if (int rc = check_launch("wgrad_kernel launch")) return rc;
    const int64_t total = (int64_t)a.I * a.J + (tr ? cout : cout), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, slabs, a.I,
                       a.J, a.ones_row, a.ones_col, (const float*)workspace, dweight, dbias);
    return check_launch("reduce_kernel launch");
  }
  return GW_OK;
}

}  // extern "C"
