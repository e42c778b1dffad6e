// gw_na3d.hip - 3-D neighbourhood attention (the NeighborhoodAttention3D layers of WeatherMesh's processor,
// graph_weather/models/weathermesh/processor.py), restated from NATTEN's documentation: non-causal, stride 1, dilation 1.
//
//   Tokens form a [B, D, H, W] volume, one row of heads * dh floats per token, head h the segment [h dh, (h + 1) dh).  Per axis of
//   length L with an odd kernel k <= L the query at index i attends to the k indices from start(i) = clamp(i - k / 2, 0, L - k):
//   near a border the window shifts inward and keeps its k keys.  The neighbourhood is the product of the three ranges; per head
//     s = scale q . k,  p = softmax of s over the kD kH kW keys,  out = sum p v.
//   The queries that see key j are a box too: per axis the range [j < k ? 0 : j - k / 2, j >= L - k ? L - 1 : j + k / 2], which is
//   longer than k within k / 2 of a border.
//
//   na_fwd_kernel   a workgroup owns a tile of 8 x 8 queries of one depth plane and one head, 4 lanes per query (a lane holds every
//                   fourth 16-byte piece of the head's segment, as the lane groups of gw_sparse_attn.hip do).  For each of the kD
//                   key planes the union of the tile's windows - at most (8 + kH - 1) x (8 + kW - 1) keys - is staged in LDS once,
//                   K beside V; a query then walks its own kH x kW window in LDS, one window row (kW scores, one rescale) per step
//                   of an online softmax that runs on across the planes.  Writes out and the (maximum, log sum exp) planes.
//   na_bwd_q_kernel the same staging; recomputes p from q, k and the planes, writes delta = rowsum(dout o out) and dq.
//   na_bwd_k_kernel a tile of 8 x 8 KEYS; stages q, dout and (maximum, log sum exp, delta) of the box of queries that see the tile,
//                   plane by plane, and each key walks its own box of queries in one fixed order: dk and dv.
//   na_*_gen_kernel any head count and head size up to 256, any odd kernel, unaligned rows: one wave per token, the heads in order,
//                   everything streamed from global memory.  Coverage, not speed.
//
// fp32, plain stores, no atomics, every sum in one fixed order: equal inputs give bitwise equal results; every row of out, dq, dk
// and dv is written once.  All volume offsets are 64-bit.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kNaTile = 8;              // queries (keys) per tile along H and along W: 64 items x 4 lanes = 256 threads
constexpr int kNaFastK = 7;             // largest kernel along H and W of the tiled path
constexpr int kNaFastDh = 64;           // largest head size of the tiled path
constexpr int kNaGenDh = 256;           // largest head size at all (4 columns per lane of the general path)
constexpr int kNaPad = 4;               // floats between staged rows: consecutive rows start 4 banks apart
constexpr int kNaLdsMax = 160 * 1024;   // bytes of LDS a workgroup may ask for

struct NaArgs {
  int B, D, H, W, heads, dh;
  int kd, kh, kw;
  int tiles_h, tiles_w;
  int halo;  // staged items per plane at most (the LDS images are sized by it)
  int rs;    // floats per staged row: dh + kNaPad
  float scale;
  const float *q, *k, *v;
  long long ld_q, ld_k, ld_v;
  float* out;  // forward: written; backward: the forward's rows
  long long ld_out;
  float* lse;  // [2][rows heads]
  long long planes;
  const float* dout;
  long long ld_dout;
  float* delta;  // [rows heads]
  float *dq, *dk, *dv;
  long long ld_dq, ld_dk, ld_dv;
};

__host__ __device__ __forceinline__ int na_start(int i, int k, int L) {
  int s = i - (k >> 1);
  s = s < 0 ? 0 : s;
  return s > L - k ? L - k : s;
}
// first and last query that see key j
__host__ __device__ __forceinline__ int na_inv_lo(int j, int k, int L) { return j < k ? 0 : j - (k >> 1); }
__host__ __device__ __forceinline__ int na_inv_hi(int j, int k, int L) { return j >= L - k ? L - 1 : j + (k >> 1); }

__device__ __forceinline__ float na_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int N>
__device__ __forceinline__ void na_quad_sum(float (&s)[N]) {  // sums over the 4 lanes of an item; every lane gets the total
#pragma unroll
  for (int u = 0; u < N; ++u) s[u] += __shfl_xor(s[u], 1);
#pragma unroll
  for (int u = 0; u < N; ++u) s[u] += __shfl_xor(s[u], 2);
}

// A lane's part of a head segment: NJ pieces of 4 floats at offsets 4 gl + 16 j; pieces past the segment's end hold zeros.
template <int NJ>
struct NaFrag {
  f32x4 r[NJ];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void load(const float* __restrict__ p, int off, int dh) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = off + 16 * j;
      r[j] = c < dh ? ldg4(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void load_lds(const float* p, int off, int dh) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = off + 16 * j;
      r[j] = c < dh ? *(const f32x4*)(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int off, int dh) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = off + 16 * j;
      if (c < dh) stg4(p + c, r[j]);
    }
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] *= s;
  }
  __device__ __forceinline__ void divide(float s) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] /= s;
  }
  __device__ __forceinline__ void axpy(float s, const NaFrag& o) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      r[j].x = fmaf(s, o.r[j].x, r[j].x), r[j].y = fmaf(s, o.r[j].y, r[j].y);
      r[j].z = fmaf(s, o.r[j].z, r[j].z), r[j].w = fmaf(s, o.r[j].w, r[j].w);
    }
  }
  __device__ __forceinline__ float dot(const NaFrag& o) const {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      s = fmaf(r[j].x, o.r[j].x, s), s = fmaf(r[j].y, o.r[j].y, s);
      s = fmaf(r[j].z, o.r[j].z, s), s = fmaf(r[j].w, o.r[j].w, s);
    }
    return s;
  }
};

// A workgroup's place: tile (th, tw) of depth plane d of volume b, head `head`; the thread's item and lane within it.
struct NaTile {
  int head, d, h0, w0, h1, w1;  // h1, w1: last valid index of the tile
  long long b;
  int item, gl, ih, iw;  // the item's coordinates, clamped into the tile's valid part
  bool live;             // the item exists (partial tiles: the others compute a valid neighbour's values and store nothing)
};
__device__ __forceinline__ NaTile na_tile(const NaArgs& a) {
  NaTile t;
  t.head = blockIdx.y;
  long long x = blockIdx.x;
  const int tw = (int)(x % a.tiles_w);
  x /= a.tiles_w;
  const int th = (int)(x % a.tiles_h);
  x /= a.tiles_h;
  t.d = (int)(x % a.D);
  t.b = x / a.D;
  t.h0 = th * kNaTile, t.w0 = tw * kNaTile;
  t.h1 = min(t.h0 + kNaTile, a.H) - 1, t.w1 = min(t.w0 + kNaTile, a.W) - 1;
  t.item = threadIdx.x >> 2, t.gl = threadIdx.x & 3;
  const int ih = t.h0 + (t.item >> 3), iw = t.w0 + (t.item & 7);
  t.live = ih <= t.h1 && iw <= t.w1;
  t.ih = min(ih, t.h1), t.iw = min(iw, t.w1);
  return t;
}

// Stages the head segments of rows (plane_row0 + (hs + y) W + ws + x), y < nh, x < nw, of two tables into two LDS images of
// `rs` floats per row; dh is a multiple of 4.  256 threads.
__device__ __forceinline__ void na_stage2(const float* __restrict__ ta, long long ld_a, const float* __restrict__ tb, long long ld_b,
                                          long long plane_row0, int W, int hs, int ws, int nh, int nw, int hc, int dh, int rs,
                                          float* la, float* lb) {
  const int ppk = dh >> 2, total = nh * nw * ppk;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int item = idx / ppk, p = idx - item * ppk;
    const int y = item / nw, x = item - y * nw;
    const long long row = plane_row0 + (long long)(hs + y) * W + ws + x;
    const f32x4 va = ldg4(ta + row * ld_a + hc + 4 * p), vb = ldg4(tb + row * ld_b + hc + 4 * p);
    *(f32x4*)(la + item * rs + 4 * p) = va;
    *(f32x4*)(lb + item * rs + 4 * p) = vb;
  }
}

// grid (B D tiles_h tiles_w, heads), block 256
template <int NJ, int KW>
__global__ __launch_bounds__(256) void na_fwd_kernel(NaArgs a) {
  typedef NaFrag<NJ> F;
  extern __shared__ __attribute__((aligned(16))) float na_lds[];
  float* Ks = na_lds;
  float* Vs = na_lds + (long long)a.halo * a.rs;
  const NaTile t = na_tile(a);
  const int dh = a.dh, rs = a.rs, hc = t.head * dh, off = 4 * t.gl;
  const int hs = na_start(t.h0, a.kh, a.H), nh = na_start(t.h1, a.kh, a.H) + a.kh - hs;
  const int ws = na_start(t.w0, a.kw, a.W), nw = na_start(t.w1, a.kw, a.W) + a.kw - ws;
  const int zs = na_start(t.d, a.kd, a.D);
  const int mh = na_start(t.ih, a.kh, a.H) - hs, mw = na_start(t.iw, a.kw, a.W) - ws;
  const long long vol = t.b * a.D;
  const long long qrow = ((vol + t.d) * a.H + t.ih) * a.W + t.iw;
  F qf, acc;
  qf.load(a.q + qrow * a.ld_q + hc, off, dh);
  qf.scale(a.scale);
  acc.zero();
  float m = -INFINITY, l = 0.f;
  for (int dz = 0; dz < a.kd; ++dz) {
    if (dz) __syncthreads();
    na_stage2(a.k, a.ld_k, a.v, a.ld_v, (vol + zs + dz) * a.H * a.W, a.W, hs, ws, nh, nw, hc, dh, rs, Ks, Vs);
    __syncthreads();
    for (int dy = 0; dy < a.kh; ++dy) {
      const int base = ((mh + dy) * nw + mw) * rs;
      float s[KW];
#pragma unroll
      for (int u = 0; u < KW; ++u) {
        F kf;
        kf.load_lds(Ks + base + u * rs, off, dh);
        s[u] = qf.dot(kf);
      }
      na_quad_sum<KW>(s);
      float mn = m;
#pragma unroll
      for (int u = 0; u < KW; ++u) mn = fmaxf(mn, s[u]);
      const float sc = expf(m - mn);  // 0 at the first step (m = -inf, mn finite)
      l *= sc;
      acc.scale(sc);
#pragma unroll
      for (int u = 0; u < KW; ++u) {
        const float p = expf(s[u] - mn);
        F vf;
        vf.load_lds(Vs + base + u * rs, off, dh);
        l += p;
        acc.axpy(p, vf);
      }
      m = mn;
    }
  }
  if (!t.live) return;
  acc.divide(l);
  acc.store(a.out + qrow * a.ld_out + hc, off, dh);
  if (t.gl == 0) {
    a.lse[qrow * a.heads + t.head] = m;
    a.lse[a.planes + qrow * a.heads + t.head] = logf(l);
  }
}

// grid (B D tiles_h tiles_w, heads), block 256: writes delta and dq (the gradient of the unscaled q)
template <int NJ, int KW>
__global__ __launch_bounds__(256) void na_bwd_q_kernel(NaArgs a) {
  typedef NaFrag<NJ> F;
  extern __shared__ __attribute__((aligned(16))) float na_lds[];
  float* Ks = na_lds;
  float* Vs = na_lds + (long long)a.halo * a.rs;
  const NaTile t = na_tile(a);
  const int dh = a.dh, rs = a.rs, hc = t.head * dh, off = 4 * t.gl;
  const int hs = na_start(t.h0, a.kh, a.H), nh = na_start(t.h1, a.kh, a.H) + a.kh - hs;
  const int ws = na_start(t.w0, a.kw, a.W), nw = na_start(t.w1, a.kw, a.W) + a.kw - ws;
  const int zs = na_start(t.d, a.kd, a.D);
  const int mh = na_start(t.ih, a.kh, a.H) - hs, mw = na_start(t.iw, a.kw, a.W) - ws;
  const long long vol = t.b * a.D;
  const long long qrow = ((vol + t.d) * a.H + t.ih) * a.W + t.iw;
  F qf, dof, dqf;
  qf.load(a.q + qrow * a.ld_q + hc, off, dh);
  qf.scale(a.scale);
  dof.load(a.dout + qrow * a.ld_dout + hc, off, dh);
  float dl[1];
  {
    F of;
    of.load(a.out + qrow * a.ld_out + hc, off, dh);
    dl[0] = dof.dot(of);
  }
  na_quad_sum<1>(dl);
  const float delta = dl[0];
  const long long ih = qrow * a.heads + t.head;
  const float m = a.lse[ih], ll = a.lse[a.planes + ih];
  dqf.zero();
  for (int dz = 0; dz < a.kd; ++dz) {
    if (dz) __syncthreads();
    na_stage2(a.k, a.ld_k, a.v, a.ld_v, (vol + zs + dz) * a.H * a.W, a.W, hs, ws, nh, nw, hc, dh, rs, Ks, Vs);
    __syncthreads();
    for (int dy = 0; dy < a.kh; ++dy) {
      const int base = ((mh + dy) * nw + mw) * rs;
      float s[2 * KW];
      F kf[KW];
#pragma unroll
      for (int u = 0; u < KW; ++u) {
        F vf;
        kf[u].load_lds(Ks + base + u * rs, off, dh);
        vf.load_lds(Vs + base + u * rs, off, dh);
        s[u] = qf.dot(kf[u]);
        s[KW + u] = dof.dot(vf);
      }
      na_quad_sum<2 * KW>(s);
#pragma unroll
      for (int u = 0; u < KW; ++u) {
        const float p = expf((s[u] - m) - ll);
        dqf.axpy(p * (s[KW + u] - delta), kf[u]);
      }
    }
  }
  if (!t.live) return;
  dqf.scale(a.scale);
  dqf.store(a.dq + qrow * a.ld_dq + hc, off, dh);
  if (t.gl == 0) a.delta[ih] = delta;
}

// grid (B D tiles_h tiles_w, heads), block 256: a tile of keys; reads delta of na_bwd_q_kernel, writes dk and dv
template <int NJ>
__global__ __launch_bounds__(256) void na_bwd_k_kernel(NaArgs a) {
  typedef NaFrag<NJ> F;
  extern __shared__ __attribute__((aligned(16))) float na_lds[];
  float* Qs = na_lds;
  float* Gs = na_lds + (long long)a.halo * a.rs;
  float* Ss = na_lds + 2ll * a.halo * a.rs;  // [halo][4]: maximum, log sum exp, delta of the staged query
  const NaTile t = na_tile(a);
  const int dh = a.dh, rs = a.rs, hc = t.head * dh, off = 4 * t.gl;
  const int hs = na_inv_lo(t.h0, a.kh, a.H), nh = na_inv_hi(t.h1, a.kh, a.H) + 1 - hs;
  const int ws = na_inv_lo(t.w0, a.kw, a.W), nw = na_inv_hi(t.w1, a.kw, a.W) + 1 - ws;
  const int z0 = na_inv_lo(t.d, a.kd, a.D), z1 = na_inv_hi(t.d, a.kd, a.D);
  const int y0 = na_inv_lo(t.ih, a.kh, a.H) - hs, y1 = na_inv_hi(t.ih, a.kh, a.H) - hs;
  const int x0 = na_inv_lo(t.iw, a.kw, a.W) - ws, x1 = na_inv_hi(t.iw, a.kw, a.W) - ws;
  const long long vol = t.b * a.D;
  const long long krow = ((vol + t.d) * a.H + t.ih) * a.W + t.iw;
  F kf, vf, dkf, dvf;
  kf.load(a.k + krow * a.ld_k + hc, off, dh);
  kf.scale(a.scale);
  vf.load(a.v + krow * a.ld_v + hc, off, dh);
  dkf.zero();
  dvf.zero();
  for (int z = z0; z <= z1; ++z) {
    if (z != z0) __syncthreads();
    const long long plane = (vol + z) * a.H * a.W;
    na_stage2(a.q, a.ld_q, a.dout, a.ld_dout, plane, a.W, hs, ws, nh, nw, hc, dh, rs, Qs, Gs);
    for (int item = threadIdx.x; item < nh * nw; item += 256) {
      const int y = item / nw, x = item - y * nw;
      const long long ih = (plane + (long long)(hs + y) * a.W + ws + x) * a.heads + t.head;
      Ss[4 * item] = a.lse[ih], Ss[4 * item + 1] = a.lse[a.planes + ih], Ss[4 * item + 2] = a.delta[ih];
    }
    __syncthreads();
    for (int y = y0; y <= y1; ++y) {
      for (int x = x0; x <= x1; ++x) {
        const int item = y * nw + x;
        F qf, gf;
        qf.load_lds(Qs + item * rs, off, dh);
        gf.load_lds(Gs + item * rs, off, dh);
        const float m = Ss[4 * item], ll = Ss[4 * item + 1], delta = Ss[4 * item + 2];
        float s[2] = {qf.dot(kf), gf.dot(vf)};
        na_quad_sum<2>(s);
        const float p = expf((s[0] - m) - ll);
        dkf.axpy(p * (s[1] - delta), qf);
        dvf.axpy(p, gf);
      }
    }
  }
  if (!t.live) return;
  dkf.scale(a.scale);
  dkf.store(a.dk + krow * a.ld_dk + hc, off, dh);
  dvf.store(a.dv + krow * a.ld_dv + hc, off, dh);
}

// ---- the general path -----------------------------------------------------------------------------------------------------------
// One wave per workgroup and token, the heads in order; lane l owns columns l, l + 64, l + 128, l + 192 of a head's segment.
struct NaTok {
  long long vol;  // b * D
  int d, h, w;
};
__device__ __forceinline__ NaTok na_tok(const NaArgs& a) {
  NaTok t;
  long long x = blockIdx.x;
  t.w = (int)(x % a.W);
  x /= a.W;
  t.h = (int)(x % a.H);
  x /= a.H;
  t.d = (int)(x % a.D);
  t.vol = (x / a.D) * a.D;
  return t;
}
struct NaCols {
  float r[4];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = 0.f;
  }
  __device__ __forceinline__ void load(const float* __restrict__ p, int lane, int dh) {
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = lane + 64 * u < dh ? ldg1(p + lane + 64 * u) : 0.f;
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int lane, int dh, float s) const {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (lane + 64 * u < dh) stg1(p + lane + 64 * u, r[u] * s);
  }
  __device__ __forceinline__ float dot(const NaCols& o) const {  // the wave's total
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) s = fmaf(r[u], o.r[u], s);
    return na_wave_sum(s);
  }
  __device__ __forceinline__ void axpy(float s, const NaCols& o) {
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = fmaf(s, o.r[u], r[u]);
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] *= s;
  }
};

__global__ __launch_bounds__(64) void na_fwd_gen_kernel(NaArgs a) {
  const int lane = threadIdx.x, dh = a.dh;
  const NaTok t = na_tok(a);
  const long long row = blockIdx.x;
  const int zs = na_start(t.d, a.kd, a.D), hs = na_start(t.h, a.kh, a.H), ws = na_start(t.w, a.kw, a.W);
  for (int h = 0; h < a.heads; ++h) {
    const int hc = h * dh;
    NaCols qc, acc;
    qc.load(a.q + row * a.ld_q + hc, lane, dh);
    qc.scale(a.scale);
    acc.zero();
    float m = -INFINITY, l = 0.f;
    for (int z = zs; z < zs + a.kd; ++z)
      for (int y = hs; y < hs + a.kh; ++y)
        for (int x = ws; x < ws + a.kw; ++x) {
          const long long j = ((t.vol + z) * a.H + y) * a.W + x;
          NaCols kc, vc;
          kc.load(a.k + j * a.ld_k + hc, lane, dh);
          vc.load(a.v + j * a.ld_v + hc, lane, dh);
          const float s = qc.dot(kc);
          const float mn = fmaxf(m, s), sc = expf(m - mn), p = expf(s - mn);
          l = l * sc + p;
          acc.scale(sc);
          acc.axpy(p, vc);
          m = mn;
        }
    acc.store(a.out + row * a.ld_out + hc, lane, dh, 1.f / l);
    if (lane == 0) {
      a.lse[row * a.heads + h] = m;
      a.lse[a.planes + row * a.heads + h] = logf(l);
    }
  }
}

__global__ __launch_bounds__(64) void na_bwd_q_gen_kernel(NaArgs a) {
  const int lane = threadIdx.x, dh = a.dh;
  const NaTok t = na_tok(a);
  const long long row = blockIdx.x;
  const int zs = na_start(t.d, a.kd, a.D), hs = na_start(t.h, a.kh, a.H), ws = na_start(t.w, a.kw, a.W);
  for (int h = 0; h < a.heads; ++h) {
    const int hc = h * dh;
    NaCols qc, gc, oc, acc;
    qc.load(a.q + row * a.ld_q + hc, lane, dh);
    qc.scale(a.scale);
    gc.load(a.dout + row * a.ld_dout + hc, lane, dh);
    oc.load(a.out + row * a.ld_out + hc, lane, dh);
    const float delta = gc.dot(oc);
    const long long ih = row * a.heads + h;
    const float m = a.lse[ih], ll = a.lse[a.planes + ih];
    acc.zero();
    for (int z = zs; z < zs + a.kd; ++z)
      for (int y = hs; y < hs + a.kh; ++y)
        for (int x = ws; x < ws + a.kw; ++x) {
          const long long j = ((t.vol + z) * a.H + y) * a.W + x;
          NaCols kc, vc;
          kc.load(a.k + j * a.ld_k + hc, lane, dh);
          vc.load(a.v + j * a.ld_v + hc, lane, dh);
          const float s = qc.dot(kc), dp = gc.dot(vc);
          acc.axpy(expf((s - m) - ll) * (dp - delta), kc);
        }
    acc.store(a.dq + row * a.ld_dq + hc, lane, dh, a.scale);
    if (lane == 0) a.delta[ih] = delta;
  }
}

__global__ __launch_bounds__(64) void na_bwd_k_gen_kernel(NaArgs a) {
  const int lane = threadIdx.x, dh = a.dh;
  const NaTok t = na_tok(a);
  const long long row = blockIdx.x;
  const int z0 = na_inv_lo(t.d, a.kd, a.D), z1 = na_inv_hi(t.d, a.kd, a.D);
  const int y0 = na_inv_lo(t.h, a.kh, a.H), y1 = na_inv_hi(t.h, a.kh, a.H);
  const int x0 = na_inv_lo(t.w, a.kw, a.W), x1 = na_inv_hi(t.w, a.kw, a.W);
  for (int h = 0; h < a.heads; ++h) {
    const int hc = h * dh;
    NaCols kc, vc, dkc, dvc;
    kc.load(a.k + row * a.ld_k + hc, lane, dh);
    kc.scale(a.scale);
    vc.load(a.v + row * a.ld_v + hc, lane, dh);
    dkc.zero();
    dvc.zero();
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
          const long long i = ((t.vol + z) * a.H + y) * a.W + x;
          NaCols qc, gc;
          qc.load(a.q + i * a.ld_q + hc, lane, dh);
          gc.load(a.dout + i * a.ld_dout + hc, lane, dh);
          const long long ih = i * a.heads + h;
          const float m = a.lse[ih], ll = a.lse[a.planes + ih], delta = a.delta[ih];
          const float s = qc.dot(kc), dp = gc.dot(vc);
          const float p = expf((s - m) - ll);
          dkc.axpy(p * (dp - delta), qc);
          dvc.axpy(p, gc);
        }
    dkc.store(a.dk + row * a.ld_dk + hc, lane, dh, a.scale);
    dvc.store(a.dv + row * a.ld_dv + hc, lane, dh, 1.f);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool na_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the most indices one tile's union of windows (keys = false) or of inverse ranges (keys = true) spans along an axis
int na_halo_axis(int L, int k, bool keys) {
  int most = 0;
  for (int j0 = 0; j0 < L; j0 += kNaTile) {
    const int j1 = (j0 + kNaTile < L ? j0 + kNaTile : L) - 1;
    const int n = keys ? na_inv_hi(j1, k, L) + 1 - na_inv_lo(j0, k, L) : na_start(j1, k, L) + k - na_start(j0, k, L);
    most = n > most ? n : most;
  }
  return most;
}

int na_check(const char* bad, int32_t B, int32_t D, int32_t H, int32_t W, int32_t heads, int32_t dh, int32_t kd, int32_t kh, int32_t kw,
             float scale) {
  if (B < 0 || D < 1 || H < 1 || W < 1 || heads < 1 || dh < 1 || !(scale == scale) || isinf(scale)) return set_error(GW_E_BADARG, bad);
  if (kd < 1 || kh < 1 || kw < 1 || !(kd & 1) || !(kh & 1) || !(kw & 1) || kd > D || kh > H || kw > W) return set_error(GW_E_BADARG, bad);
  if (dh > kNaGenDh) return set_error(GW_E_UNSUPPORTED, "neighbourhood attention: dim_head must be at most 256");
  const int64_t rows = (int64_t)B * D * H * W;
  if (rows >= ((int64_t)1 << 31) || rows * heads >= ((int64_t)1 << 31) || heads > 65535) return set_error(GW_E_BADARG, bad);
  return GW_OK;
}

// fills the geometry; returns the LDS bytes of the tiled path or 0 when the launch takes the general path
size_t na_plan(NaArgs& a, bool vec, bool keys) {
  a.tiles_h = (a.H + kNaTile - 1) / kNaTile, a.tiles_w = (a.W + kNaTile - 1) / kNaTile;
  a.rs = a.dh + kNaPad;
  if (!vec || a.dh % 4 != 0 || a.dh > kNaFastDh || a.kh > kNaFastK || a.kw > kNaFastK) return 0;
  a.halo = na_halo_axis(a.H, a.kh, keys) * na_halo_axis(a.W, a.kw, keys);
  const size_t bytes = ((size_t)2 * a.halo * a.rs + (keys ? (size_t)4 * a.halo : 0)) * sizeof(float);
  return bytes <= (size_t)kNaLdsMax ? bytes : 0;
}

#define GW_NA_LAUNCH(KERNEL, GRID, LDS)                                                                                   \
  do {                                                                                                                    \
    static DeviceOnce once;                                                                                               \
    if (once.first()) (void)hipFuncSetAttribute((const void*)(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, kNaLdsMax); \
    hipLaunchKernelGGL((KERNEL), GRID, dim3(256), LDS, (hipStream_t)stream, a);                                           \
  } while (0)

#define GW_NA_BY_KW(NAME, NJ, GRID, LDS)                              \
  switch (a.kw) {                                                     \
    case 1: GW_NA_LAUNCH((NAME<NJ, 1>), GRID, LDS); break;            \
    case 3: GW_NA_LAUNCH((NAME<NJ, 3>), GRID, LDS); break;            \
    case 5: GW_NA_LAUNCH((NAME<NJ, 5>), GRID, LDS); break;            \
    default: GW_NA_LAUNCH((NAME<NJ, 7>), GRID, LDS); break;           \
  }

#define GW_NA_BY_DH(NAME, GRID, LDS)                                  \
  if (a.dh <= 16) {                                                   \
    GW_NA_BY_KW(NAME, 1, GRID, LDS)                                   \
  } else if (a.dh <= 32) {                                            \
    GW_NA_BY_KW(NAME, 2, GRID, LDS)                                   \
  } else {                                                            \
    GW_NA_BY_KW(NAME, 4, GRID, LDS)                                   \
  }

}  // namespace

extern "C" {

int gw_na3d_forward(int32_t batch, int32_t depth, int32_t height, int32_t width, int32_t heads, int32_t dim_head, int32_t kd, int32_t kh,
                    int32_t kw, float scale, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v,
                    float* out, int32_t ld_out, float* lse, void* stream) {
  const char* bad = "gw_na3d_forward: bad arguments";
  if (int rc = na_check(bad, batch, depth, height, width, heads, dim_head, kd, kh, kw, scale)) return rc;
  if (batch == 0) return GW_OK;
  const int C = heads * dim_head;
  if (!q || !k || !v || !out || !lse || ld_q < C || ld_k < C || ld_v < C || ld_out < C) return set_error(GW_E_BADARG, bad);
  const bool vec = ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && na_aligned16(q) && na_aligned16(k) &&
                   na_aligned16(v) && na_aligned16(out);
  NaArgs a = {};
  a.B = batch, a.D = depth, a.H = height, a.W = width, a.heads = heads, a.dh = dim_head, a.kd = kd, a.kh = kh, a.kw = kw, a.scale = scale;
  a.q = q, a.k = k, a.v = v, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v, a.out = out, a.ld_out = ld_out, a.lse = lse;
  const int64_t rows = (int64_t)batch * depth * height * width;
  a.planes = rows * heads;
  const size_t lds = na_plan(a, vec, false);
  if (lds) {
    const dim3 grid((unsigned)((int64_t)batch * depth * a.tiles_h * a.tiles_w), (unsigned)heads);
    GW_NA_BY_DH(na_fwd_kernel, grid, lds)
  } else {
    hipLaunchKernelGGL(na_fwd_gen_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, a);
  }
  return check_launch("na_fwd_kernel launch");
}

int gw_na3d_backward(int32_t batch, int32_t depth, int32_t height, int32_t width, int32_t heads, int32_t dim_head, int32_t kd, int32_t kh,
                     int32_t kw, float scale, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v,
                     const float* out, int32_t ld_out, const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq,
                     int32_t ld_dq, float* dk, int32_t ld_dk, float* dv, int32_t ld_dv, void* stream) {
  const char* bad = "gw_na3d_backward: bad arguments";
  if (int rc = na_check(bad, batch, depth, height, width, heads, dim_head, kd, kh, kw, scale)) return rc;
  if (batch == 0) return GW_OK;
  const int C = heads * dim_head;
  if (!q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv || ld_q < C || ld_k < C || ld_v < C || ld_out < C ||
      ld_dout < C || ld_dq < C || ld_dk < C || ld_dv < C)
    return set_error(GW_E_BADARG, bad);
  const bool vec = ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && ld_dout % 4 == 0 && ld_dq % 4 == 0 &&
                   ld_dk % 4 == 0 && ld_dv % 4 == 0 && na_aligned16(q) && na_aligned16(k) && na_aligned16(v) && na_aligned16(out) &&
                   na_aligned16(dout) && na_aligned16(dq) && na_aligned16(dk) && na_aligned16(dv);
  NaArgs a = {};
  a.B = batch, a.D = depth, a.H = height, a.W = width, a.heads = heads, a.dh = dim_head, a.kd = kd, a.kh = kh, a.kw = kw, a.scale = scale;
  a.q = q, a.k = k, a.v = v, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v;
  a.out = const_cast<float*>(out), a.ld_out = ld_out, a.lse = const_cast<float*>(lse);
  a.dout = dout, a.ld_dout = ld_dout, a.delta = delta;
  a.dq = dq, a.dk = dk, a.dv = dv, a.ld_dq = ld_dq, a.ld_dk = ld_dk, a.ld_dv = ld_dv;
  const int64_t rows = (int64_t)batch * depth * height * width;
  a.planes = rows * heads;
  const size_t lds_q = na_plan(a, vec, false);
  if (lds_q) {
    const dim3 grid((unsigned)((int64_t)batch * depth * a.tiles_h * a.tiles_w), (unsigned)heads);
    GW_NA_BY_DH(na_bwd_q_kernel, grid, lds_q)
  } else {
    hipLaunchKernelGGL(na_bwd_q_gen_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, a);
  }
  if (int rc = check_launch("na_bwd_q_kernel launch")) return rc;
  const size_t lds_k = na_plan(a, vec, true);
  if (lds_k) {
    const dim3 grid((unsigned)((int64_t)batch * depth * a.tiles_h * a.tiles_w), (unsigned)heads);
    if (a.dh <= 16) {
      GW_NA_LAUNCH((na_bwd_k_kernel<1>), grid, lds_k);
    } else if (a.dh <= 32) {
      GW_NA_LAUNCH((na_bwd_k_kernel<2>), grid, lds_k);
    } else {
      GW_NA_LAUNCH((na_bwd_k_kernel<4>), grid, lds_k);
    }
  } else {
    hipLaunchKernelGGL(na_bwd_k_gen_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, a);
  }
  return check_launch("na_bwd_k_kernel launch");
}

}  // extern "C"
