// gw_cafa.hip - the patch convolutions of the CaFA models (graph_weather/models/cafa/encoder.py, decoder.py, model.py):
//
//   gw_patch_embed_forward / _backward    Conv2d(C, D, kernel = stride = f) on an NCHW image read as it lies -> channels-last rows
//                                         [(b, py, px), D]; pixels past H or W read zero (the forecaster's F.pad, as a predicate)
//   gw_patch_expand_forward / _backward   ConvTranspose2d(D, C, kernel = stride = f) from rows to an NCHW image, writing only the
//                                         H x W crop
//
// A kernel equal to its stride makes both a plain matrix product over the PATCH VIEW of the image: the [M, K] matrix with
// M = B . oh . ow patches (oh = ceil(H / f), ow = ceil(W / f)), K = C . f . f, element (m = (b, py, px), k = (c, ky, kx)) =
// image[b, c, f py + ky, f px + kx], zero outside H x W.  Every pixel of the image is exactly one element of the view, so a
// product whose OUTPUT is the view writes the whole image once and nothing else.  One kernel, C(i, j) = sum_r A(i, r) B(j, r),
// whose operands are dense rows or a patch view, either way round:
//
//   embed forward    rows[m, d]   = sum_k  view(x)[m, k]   W[d, k]   + bias[d]
//   embed dx         view(dx)[m, k] = sum_d  W^T[k, d]      dout[m, d]                     (i = k, j = m)
//   embed dW, db     dW[d, k]     = sum_m  dout^T[d, m]    view(x)^T[k, m];   db = the column of ones appended to view(x)^T
//   expand forward   view(out)[m, k] = sum_d  W^T[k, d]    rows[m, d] + bias[k / f^2]     (i = k, j = m)
//   expand d_rows    d_rows[m, d] = sum_k  view(dout)[m, k] W[d, k]
//   expand dW, db    dW[d, k]     = sum_m  rows^T[d, m]    view(dout)^T[k, m];  db = the row of ones appended to rows^T, folded f^2
//
// (Conv2d's weight [D, C, f, f] and ConvTranspose2d's [D, C, f, f] are both the dense [D, K] matrix.)  Products run on
// v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) from LDS tiles of 64 x 16; a view is written with the patch index on the
// lanes, so a wave stores runs of pixels f apart in one image row.  The weight gradients split the M patches into slabs of
// kSlab, one partial [D(+1), K(+1)] per slab in the caller's workspace, added by a second kernel in slab order: no atomics,
// bitwise reproducible.  All image offsets are 64-bit.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kSlab = 1024;  // patches per weight-gradient partial
constexpr int kTile = 64, kStep = 16, kLd = kStep + 1;  // LDS tile: 64 rows x 16 reduction indices, odd row stride

enum { V_DENSE = 0, V_PATCH = 1 };
enum { C_DENSE = 0, C_PATCH = 1, C_PARTIAL = 2 };

struct View {     // an [M, K] matrix
  float* p;
  int64_t ld;     // V_DENSE: element (m, k) at p[m ld + k]
  int C, H, W, f, oh, ow;  // V_PATCH: the patches of p[B, C, H, W]
  int ones;       // transposed operands: the index k whose elements are all 1 (-1: none)
};

// offset of element (m, k) of the patch view, or -1 where it lies outside H x W
__device__ __forceinline__ int64_t patch_offset(const View& v, int m, int k) {
  const int ff = v.f * v.f;
  const int c = k / ff, t = k - c * ff;
  const int ky = t / v.f, kx = t - ky * v.f;
  const int q = m / v.ow, px = m - q * v.ow;
  const int b = q / v.oh, py = q - b * v.oh;
  const int y = py * v.f + ky, x = px * v.f + kx;
  if (y >= v.H || x >= v.W) return -1;
  return (((int64_t)b * v.C + c) * v.H + y) * v.W + x;
}

template <int MODE>
__device__ __forceinline__ float view_at(const View& v, int m, int k, int M, int K) {
  if (m >= M) return 0.f;
  if (k == v.ones) return 1.f;
  if (k >= K) return 0.f;
  if (MODE == V_DENSE) return ldg1(v.p + (int64_t)m * v.ld + k);
  const int64_t off = patch_offset(v, m, k);
  return off < 0 ? 0.f : ldg1(v.p + off);
}

struct GemmArgs {
  int I, J, R;      // C is [I, J]; R = the full reduction length
  int slab;         // reduction indices per blockIdx.y
  View a, b;        // A(i, r): element (i, r) of a, or (r, i) if transposed; B(j, r) alike
  int ak, bk;       // the K of a and of b (without the column of ones)
  View c;           // C_DENSE: rows [I, J]; C_PATCH: the view, element (m = j, k = i); C_PARTIAL: p[blockIdx.y][I][J]
  const float* bias;  // C_DENSE: [J]; C_PATCH: [C] by channel; may be NULL
};

// 64 x 16 tile of an operand: rows x0 .. x0 + 63 of the output index, reduction indices r0 .. r0 + 15 (below r1)
template <int MODE, bool T>
__device__ __forceinline__ void stage(float* lds, const View& v, int K, int X, int R, int x0, int r0, int r1, int tid) {
  constexpr bool kFastR = (MODE == V_DENSE) != T;  // which index walks memory with the smaller stride
  for (int idx = tid; idx < kTile * kStep; idx += 256) {
    const int x = kFastR ? idx >> 4 : idx & 63, r = kFastR ? idx & 15 : idx >> 6;
    float val = 0.f;
    if (r0 + r < r1) val = T ? view_at<MODE>(v, r0 + r, x0 + x, R, K) : view_at<MODE>(v, x0 + x, r0 + r, X, K);
    lds[x * kLd + r] = val;
  }
}

template <int AMODE, bool AT, int BMODE, bool BT, int CMODE>
__global__ __launch_bounds__(256) void patch_gemm_kernel(const GemmArgs g) {
  __shared__ float As[kTile * kLd];
  __shared__ float Bs[kTile * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kq = lane >> 4;
  const int tj = (g.J + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.x / tj) * kTile, j0 = (int)(blockIdx.x % tj) * kTile;
  const int64_t rlo = (int64_t)blockIdx.y * g.slab;
  const int r_begin = (int)rlo, r_end = (int)(rlo + g.slab < g.R ? rlo + g.slab : g.R);
  f32x4 acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = r_begin; r0 < r_end; r0 += kStep) {
    __syncthreads();
    stage<AMODE, AT>(As, g.a, g.ak, g.I, g.R, i0, r0, r_end, threadIdx.x);
    stage<BMODE, BT>(Bs, g.b, g.bk, g.J, g.R, j0, r0, r_end, threadIdx.x);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kStep / 4; ++ks) {
      const float av = As[(16 * wave + l16) * kLd + 4 * ks + kq];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[(16 * jt + l16) * kLd + 4 * ks + kq], acc[jt], 0, 0, 0);
    }
  }
  // acc[jt][r] = C[i0 + 16 wave + 4 kq + r][j0 + 16 jt + l16]
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int j = j0 + 16 * jt + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * wave + 4 * kq + r;
      if (i >= g.I || j >= g.J) continue;
      if (CMODE == C_DENSE) {
        stg1(g.c.p + (int64_t)i * g.c.ld + j, acc[jt][r] + (g.bias != nullptr ? ldg1(g.bias + j) : 0.f));
      } else if (CMODE == C_PATCH) {
        const int64_t off = patch_offset(g.c, j, i);
        if (off >= 0) stg1(g.c.p + off, acc[jt][r] + (g.bias != nullptr ? ldg1(g.bias + i / (g.c.f * g.c.f)) : 0.f));
      } else {
        stg1(g.c.p + ((int64_t)blockIdx.y * g.I + i) * g.J + j, acc[jt][r]);
      }
    }
  }
}

// dw[i, j] = sum_s ws[s][i][j] for i < DI, j < DJ, and the bias gradient from the extra row i = DI (db_row: db[g] = the sum
// over s and over the `fold` columns of group g) or the extra column j = DJ (db[g] = sum_s ws[s][g][DJ]); s ascending.
__global__ __launch_bounds__(256) void patch_reduce_kernel(int S, int I, int J, const float* __restrict__ ws, int DI, int DJ,
                                                           float* __restrict__ dw, float* __restrict__ db, int db_n, int fold,
                                                           int db_row) {
  const int64_t nw = (int64_t)DI * DJ, total = nw + db_n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    if (e < nw) {
      const int i = (int)(e / DJ), j = (int)(e - (int64_t)i * DJ);
      for (int sl = 0; sl < S; ++sl) s += ldg1(ws + ((int64_t)sl * I + i) * J + j);
      stg1(dw + e, s);
    } else {
      const int gidx = (int)(e - nw);
      for (int sl = 0; sl < S; ++sl) {
        if (db_row) {
          for (int t = 0; t < fold; ++t) s += ldg1(ws + ((int64_t)sl * I + DI) * J + (int64_t)gidx * fold + t);
        } else {
          s += ldg1(ws + ((int64_t)sl * I + gidx) * J + DJ);
        }
      }
      stg1(db + gidx, s);
    }
  }
}

struct Geo {
  int batch, C, H, W, f, D, oh, ow, K;
  int M;
  int slabs;
};

int geometry(Geo& g, const char* what, int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim) {
  static char msg[160];
  if (batch <= 0 || channels <= 0 || h <= 0 || w <= 0 || f <= 0 || dim <= 0) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  const int64_t oh = ((int64_t)h + f - 1) / f, ow = ((int64_t)w + f - 1) / f;
  const int64_t m = (int64_t)batch * oh * ow, k = (int64_t)channels * f * f;
  const int64_t lim = ((int64_t)1 << 31) - 2 * kTile - 2;
  if (m >= lim || k >= lim || oh * f >= lim || ow * f >= lim || dim >= lim) {
    snprintf(msg, sizeof msg, "%s: size exceeds int32", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  g.batch = batch, g.C = channels, g.H = h, g.W = w, g.f = f, g.D = dim, g.oh = (int)oh, g.ow = (int)ow, g.K = (int)k, g.M = (int)m;
  g.slabs = (g.M + kSlab - 1) / kSlab;
  if (g.slabs > 65535) {  // the slab is the grid's y index
    snprintf(msg, sizeof msg, "%s: more than 65535 x %d patches", what, kSlab);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  return GW_OK;
}

View dense(const float* p, int64_t ld) {
  View v = {};
  v.p = const_cast<float*>(p), v.ld = ld, v.ones = -1;
  return v;
}
View patches(const Geo& g, const float* p) {
  View v = {};
  v.p = const_cast<float*>(p), v.C = g.C, v.H = g.H, v.W = g.W, v.f = g.f, v.oh = g.oh, v.ow = g.ow, v.ones = -1;
  return v;
}

template <int AMODE, bool AT, int BMODE, bool BT, int CMODE>
int launch(const GemmArgs& a, int grid_y, const char* what, void* stream) {
  const int64_t tiles = (int64_t)((a.I + kTile - 1) / kTile) * ((a.J + kTile - 1) / kTile);
  if (tiles >= ((int64_t)1 << 31)) return failf(GW_E_UNSUPPORTED, "patch_gemm_kernel: too many tiles");
  hipLaunchKernelGGL((patch_gemm_kernel<AMODE, AT, BMODE, BT, CMODE>), dim3((unsigned)tiles, (unsigned)grid_y), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch(what);
}

size_t workspace_bytes(const Geo& g) { return (size_t)g.slabs * (size_t)(g.D + 1) * (size_t)(g.K + 1) * sizeof(float); }

// dW [D, K] and db from x_t(i = d, r = m) and y_t(j = k, r = m), one of them carrying the ones
int wgrad(const Geo& g, const View& rows_t, const View& view_t, bool ones_on_rows, float* ws, float* dw, float* db, void* stream) {
  GemmArgs a = {};
  a.I = g.D + (ones_on_rows ? 1 : 0), a.J = g.K + (ones_on_rows ? 0 : 1), a.R = g.M, a.slab = kSlab;
  a.a = rows_t, a.b = view_t, a.ak = g.D, a.bk = g.K;
  if (ones_on_rows) a.a.ones = g.D; else a.b.ones = g.K;
  a.c = dense(ws, 0);
  int rc = launch<V_DENSE, true, V_PATCH, true, C_PARTIAL>(a, g.slabs, "patch_gemm_kernel (weight gradient) launch", stream);
  if (rc != GW_OK) return rc;
  const int db_n = ones_on_rows ? g.C : g.D;
  const int64_t total = (int64_t)g.D * g.K + db_n;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(patch_reduce_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, g.slabs,
                     a.I, a.J, ws, g.D, g.K, dw, db, db_n, g.f * g.f, ones_on_rows ? 1 : 0);
  return check_launch("patch_reduce_kernel launch");
}

}  // namespace

extern "C" {

size_t gw_patch_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim) {
  Geo g;
  if (geometry(g, "gw_patch_workspace_bytes", batch, channels, h, w, f, dim) != GW_OK) return 0;
  return workspace_bytes(g);
}

int gw_patch_embed_forward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* x,
                           const float* weight, const float* bias, float* out, int32_t ld_out, void* stream) {
  Geo g;
  if (!x || !weight || !out || ld_out < dim) return failf(GW_E_BADARG, "gw_patch_embed_forward: bad arguments");
  int rc = geometry(g, "gw_patch_embed_forward", batch, channels, h, w, f, dim);
  if (rc != GW_OK) return rc;
  GemmArgs a = {};
  a.I = g.M, a.J = g.D, a.R = g.K, a.slab = g.K;
  a.a = patches(g, x), a.ak = g.K, a.b = dense(weight, g.K), a.bk = g.K, a.c = dense(out, ld_out), a.bias = bias;
  return launch<V_PATCH, false, V_DENSE, false, C_DENSE>(a, 1, "patch_gemm_kernel (embed forward) launch", stream);
}

int gw_patch_embed_backward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* x,
                            const float* weight, const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes_,
                            float* dx, float* dweight, float* dbias, void* stream) {
  Geo g;
  if (!x || !weight || !dout || ld_dout < dim || (dweight == nullptr) != (dbias == nullptr) || (!dx && !dweight))
    return failf(GW_E_BADARG, "gw_patch_embed_backward: bad arguments");
  int rc = geometry(g, "gw_patch_embed_backward", batch, channels, h, w, f, dim);
  if (rc != GW_OK) return rc;
  if (dweight != nullptr && (!workspace || workspace_bytes_ < workspace_bytes(g)))  // before anything is launched
    return failf(GW_E_BADARG, "gw_patch_embed_backward: bad arguments (workspace)");
  if (dx != nullptr) {  // view(dx)[m, k] = sum_d W[d, k] dout[m, d]
    GemmArgs a = {};
    a.I = g.K, a.J = g.M, a.R = g.D, a.slab = g.D;
    a.a = dense(weight, g.K), a.ak = g.K, a.b = dense(dout, ld_dout), a.bk = g.D, a.c = patches(g, dx);
    rc = launch<V_DENSE, true, V_DENSE, false, C_PATCH>(a, 1, "patch_gemm_kernel (embed dx) launch", stream);
    if (rc != GW_OK) return rc;
  }
  if (dweight != nullptr) {
    rc = wgrad(g, dense(dout, ld_dout), patches(g, x), false, (float*)workspace, dweight, dbias, stream);
  }
  return rc;
}

int gw_patch_expand_forward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* rows,
                            int32_t ld_rows, const float* weight, const float* bias, float* out, void* stream) {
  Geo g;
  if (!rows || !weight || !out || ld_rows < dim) return failf(GW_E_BADARG, "gw_patch_expand_forward: bad arguments");
  int rc = geometry(g, "gw_patch_expand_forward", batch, channels, h, w, f, dim);
  if (rc != GW_OK) return rc;
  GemmArgs a = {};  // view(out)[m, k] = sum_d W[d, k] rows[m, d] + bias[channel of k]
  a.I = g.K, a.J = g.M, a.R = g.D, a.slab = g.D;
  a.a = dense(weight, g.K), a.ak = g.K, a.b = dense(rows, ld_rows), a.bk = g.D, a.c = patches(g, out), a.bias = bias;
  return launch<V_DENSE, true, V_DENSE, false, C_PATCH>(a, 1, "patch_gemm_kernel (expand forward) launch", stream);
}

int gw_patch_expand_backward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* rows,
                             int32_t ld_rows, const float* weight, const float* dout, void* workspace, size_t workspace_bytes_,
                             float* d_rows, int32_t ld_drows, float* dweight, float* dbias, void* stream) {
  Geo g;
  if (!rows || !weight || !dout || ld_rows < dim || (dweight == nullptr) != (dbias == nullptr) || (!d_rows && !dweight) ||
      (d_rows && ld_drows < dim))
    return failf(GW_E_BADARG, "gw_patch_expand_backward: bad arguments");
  int rc = geometry(g, "gw_patch_expand_backward", batch, channels, h, w, f, dim);
  if (rc != GW_OK) return rc;
  if (dweight != nullptr && (!workspace || workspace_bytes_ < workspace_bytes(g)))  // before anything is launched
    return failf(GW_E_BADARG, "gw_patch_expand_backward: bad arguments (workspace)");
  if (d_rows != nullptr) {  // d_rows[m, d] = sum_k view(dout)[m, k] W[d, k]
    GemmArgs a = {};
    a.I = g.M, a.J = g.D, a.R = g.K, a.slab = g.K;
    a.a = patches(g, dout), a.ak = g.K, a.b = dense(weight, g.K), a.bk = g.K, a.c = dense(d_rows, ld_drows);
    rc = launch<V_PATCH, false, V_DENSE, false, C_DENSE>(a, 1, "patch_gemm_kernel (expand d_rows) launch", stream);
    if (rc != GW_OK) return rc;
  }
  if (dweight != nullptr) {
    rc = wgrad(g, dense(rows, ld_rows), patches(g, dout), true, (float*)workspace, dweight, dbias, stream);
  }
  return rc;
}

}  // extern "C"
