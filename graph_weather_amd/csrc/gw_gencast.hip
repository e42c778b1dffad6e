// gw_gencast.hip - the GenCast layers (graph_weather/models/gencast/layers): graph-transformer attention over the incoming edges
// of every node (the TransformerConv of the mesh processor) and the row operations around it.
//
//   attn_fwd_kernel      one wave per (destination, head) - per destination with the head-mean, the heads then in order - walks the
//                        destination's run of the destination-sorted edge list once: the q row stays in registers, the k, v (and e)
//                        rows of U edges are gathered into registers with 16-byte loads, the scores are wave sums, the softmax is
//                        online (running maximum, sum and output row in registers).  Nothing of size E x H x C or E x H is written;
//                        per (destination, head) the score maximum and log sum exp(s - max) go to two planes for the backward.
//   attn_bwd_dst_kernel  backward by recomputation, one wave per (destination, head): delta = rowsum(dout o out), then the same walk
//                        writes dq and - every edge belongs to one destination - de in the caller's edge order with plain stores.
//   attn_bwd_src_kernel  one wave per (source, head) walks the source-sorted list (GraphPlan.src_sorted) and writes dk and dv.
//   A row fragment is NE floats per lane: columns 4 lane + 256 j .. + 3 (VEC: dim_head and every stride a multiple of 4, 16-byte
//   loads) or lane + 64 j (scalar path, any dim_head and stride); columns past dim_head hold zeros, so dot products need no guard.
//   attn_*_long_kernel   rows too long for register fragments (a scalar dim_head above 512, any above 2048): one wave per workgroup,
//                        running rows in LDS, everything else streamed - coverage up to heads * dim_head = 4096.
//   A destination with many edges is one wave's serial walk: correct at any degree, fast only for near-uniform degrees.
//
//   cln_*_kernel         ConditionalLayerNorm: act(scale[r] o LN(x[r]) + bias[r]) (LN without affine, eps 1e-5), one wave per row
//   gate_*_kernel        TransformerConv's beta gate: g = sigmoid(w_a.out + w_b.x_r + w_c.(out - x_r)), y = g x_r + (1 - g) out; the
//                        weight gradient is per-slab partials (256 rows, one thread per column, rows in order) added in slab order
//   silu_*, fourier_*    SiLU; cos / sin features of the noise level (accurate cosf / sinf) and their gradient
//
// fp32 data, no atomics, every sum in one fixed order: equal inputs give bitwise equal results.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kMaxRow = 4096;   // heads * dim_head
constexpr int kGateSlab = 256;  // rows per partial of the gate's weight gradient

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

unsigned grid_for(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

// ---- row fragments -----------------------------------------------------------------------------------------------------------
template <int NE, bool VEC>
struct Frag {
  float r[NE];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] = 0.f;
  }
  __device__ __forceinline__ void load(const float* __restrict__ p, int C, int lane) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NE / 4; ++j) {
        const int c = 4 * lane + 256 * j;
        const f32x4 v = c < C ? ldg4(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int c = lane + 64 * j;
        r[j] = c < C ? ldg1(p + c) : 0.f;
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int C, int lane) const {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NE / 4; ++j) {
        const int c = 4 * lane + 256 * j;
        if (c < C) stg4(p + c, f32x4{r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]});
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int c = lane + 64 * j;
        if (c < C) stg1(p + c, r[j]);
      }
    }
  }
  __device__ __forceinline__ void add(const Frag& o) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] += o.r[j];
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] *= s;
  }
  __device__ __forceinline__ void divide(float s) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] /= s;
  }
  __device__ __forceinline__ void axpy(float s, const Frag& o) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] = fmaf(s, o.r[j], r[j]);
  }
  __device__ __forceinline__ float dot(const Frag& o) const {  // this lane's part; wave_sum makes the row's
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NE; ++j) s = fmaf(r[j], o.r[j], s);
    return s;
  }
};

struct AttnArgs {
  int n_dst, n_src, heads, C, mean;
  const int* dst_ptr;        // [n_dst + 1]
  const int* src;            // [E] source row of destination-sorted edge t
  const int* dst;            // [E] destination row of destination-sorted edge t (source pass)
  const long long* perm;     // [E] caller's edge id of destination-sorted edge t (NULL: t itself)
  const int* src_pos;        // [E] destination-sorted positions grouped by source row (source pass)
  const int* src_ptr;        // [n_src + 1]
  const float *q, *k, *v, *e;
  long long ld_q, ld_k, ld_v, ld_e;
  float* out;
  long long ld_out;
  float* out_heads;          // forward: per-head rows beside the head-mean (may be NULL); backward: the per-head output rows
  long long ld_oh;
  float* lse;                // [2][n_dst * heads]
  const float* dout;
  long long ld_dout;
  float* delta;              // [n_dst * heads]
  float *dq, *dk, *dv, *de;
  long long ld_dq, ld_dk, ld_dv, ld_de;
  float sqrt_c;
};

// grid ceil(items / 4), block 256: wave = one (destination, head), or one destination with its heads in order (head-mean)
template <int NE, bool VEC, int U>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  typedef Frag<NE, VEC> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * 4 + wave;
  const long long n_items = a.mean ? (long long)a.n_dst : (long long)a.n_dst * a.heads;
  if (item >= n_items) return;
  const int i = a.mean ? (int)item : (int)(item / a.heads);
  const int h0 = a.mean ? 0 : (int)(item % a.heads), hn = a.mean ? a.heads : 1;
  const int C = a.C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const long long planes = (long long)a.n_dst * a.heads;
  F macc;
  macc.zero();
  for (int hh = 0; hh < hn; ++hh) {
    const int h = h0 + hh;
    const long long hc = (long long)h * C;
    F qf, acc;
    qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
    acc.zero();
    float m = -INFINITY, l = 0.f;
    for (int t = e0; t < e1; t += U) {
      float s[U];
      F vf[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int tt = t + u < e1 ? t + u : e1 - 1;  // past the run: the last edge again, with a score of -inf
        const int j = ldgi(a.src + tt);
        F kf;
        kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
        vf[u].load(a.v + (long long)j * a.ld_v + hc, C, lane);
        if (a.e != nullptr) {
          const long long eid = a.perm != nullptr ? a.perm[tt] : (long long)tt;
          F ef;
          ef.load(a.e + eid * a.ld_e + hc, C, lane);
          kf.add(ef);
          vf[u].add(ef);
        }
        const float d = wave_sum(qf.dot(kf)) / a.sqrt_c;
        s[u] = t + u < e1 ? d : -INFINITY;
      }
      float mn = m;
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
      const float sc = expf(m - mn);  // 0 at the first step (m = -inf, mn finite: s[0] is a real edge)
      l *= sc;
      acc.scale(sc);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = expf(s[u] - mn);
        l += p;
        acc.axpy(p, vf[u]);
      }
      m = mn;
    }
    const bool any = e1 > e0;  // a destination without edges: output 0 (and 0 in both planes, which nothing reads)
    if (any) acc.divide(l);
    if (lane == 0) {
      a.lse[(long long)i * a.heads + h] = any ? m : 0.f;
      a.lse[planes + (long long)i * a.heads + h] = any ? logf(l) : 0.f;
    }
    if (a.mean) {
      macc.add(acc);
      if (a.out_heads != nullptr) acc.store(a.out_heads + (long long)i * a.ld_oh + hc, C, lane);
    } else {
      acc.store(a.out + (long long)i * a.ld_out + hc, C, lane);
    }
  }
  if (a.mean) {
    macc.divide((float)a.heads);
    macc.store(a.out + (long long)i * a.ld_out, C, lane);
  }
}

// grid ceil(n_dst * heads / 4), block 256
template <int NE, bool VEC>
__global__ __launch_bounds__(256) void attn_bwd_dst_kernel(AttnArgs a) {
  typedef Frag<NE, VEC> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.n_dst * a.heads) return;
  const int i = (int)(item / a.heads), h = (int)(item % a.heads), C = a.C;
  const long long hc = (long long)h * C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  F qf, dof, dqf;
  qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
  dof.load(a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc), C, lane);
  if (a.mean) dof.divide((float)a.heads);
  float delta;
  {
    F of;
    of.load(a.out_heads + (long long)i * a.ld_oh + hc, C, lane);
    delta = wave_sum(dof.dot(of));
  }
  if (lane == 0) a.delta[item] = delta;
  const float m = a.lse[item], ll = a.lse[(long long)a.n_dst * a.heads + item];
  dqf.zero();
  for (int t = e0; t < e1; ++t) {
    const int j = ldgi(a.src + t);
    const long long eid = a.perm != nullptr ? a.perm[t] : (long long)t;
    const float* er = a.e != nullptr ? a.e + eid * a.ld_e + hc : nullptr;
    F kf;
    kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
    if (er != nullptr) {
      F ef;
      ef.load(er, C, lane);
      kf.add(ef);
    }
    const float s = wave_sum(qf.dot(kf)) / a.sqrt_c;
    float dp;
    {  // (the widest fragments read e a second time instead of keeping it: registers)
      F vf;
      vf.load(a.v + (long long)j * a.ld_v + hc, C, lane);
      if (er != nullptr) {
        F ef;
        ef.load(er, C, lane);
        vf.add(ef);
      }
      dp = wave_sum(dof.dot(vf));
    }
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    dqf.axpy(g, kf);
    if (a.de != nullptr) {  // d(k + e) + d(v + e) of this edge and head
      F def;
      def.zero();
      def.axpy(g, qf);
      def.axpy(p, dof);
      def.store(a.de + eid * a.ld_de + hc, C, lane);
    }
  }
  dqf.store(a.dq + (long long)i * a.ld_dq + hc, C, lane);
}

// grid ceil(n_src * heads / 4), block 256; reads delta of attn_bwd_dst_kernel
template <int NE, bool VEC>
__global__ __launch_bounds__(256) void attn_bwd_src_kernel(AttnArgs a) {
  typedef Frag<NE, VEC> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.n_src * a.heads) return;
  const int j = (int)(item / a.heads), h = (int)(item % a.heads), C = a.C;
  const long long hc = (long long)h * C, planes = (long long)a.n_dst * a.heads;
  const int s0 = ldgi(a.src_ptr + j), s1 = ldgi(a.src_ptr + j + 1);
  F kf, vf, dkf, dvf;
  kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
  vf.load(a.v + (long long)j * a.ld_v + hc, C, lane);
  dkf.zero();
  dvf.zero();
  for (int t = s0; t < s1; ++t) {
    const int pos = ldgi(a.src_pos + t);
    const int i = ldgi(a.dst + pos);
    F ke = kf, ve = vf, qf, dof;
    if (a.e != nullptr) {
      const long long eid = a.perm != nullptr ? a.perm[pos] : (long long)pos;
      F ef;
      ef.load(a.e + eid * a.ld_e + hc, C, lane);
      ke.add(ef);
      ve.add(ef);
    }
    qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
    dof.load(a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc), C, lane);
    if (a.mean) dof.divide((float)a.heads);
    const long long ih = (long long)i * a.heads + h;
    const float m = a.lse[ih], ll = a.lse[planes + ih], delta = a.delta[ih];
    const float s = wave_sum(qf.dot(ke)) / a.sqrt_c;
    const float dp = wave_sum(dof.dot(ve));
    const float p = expf((s - m) - ll);
    dkf.axpy(p * (dp - delta) / a.sqrt_c, qf);
    dvf.axpy(p, dof);
  }
  dkf.store(a.dk + (long long)j * a.ld_dk + hc, C, lane);
  dvf.store(a.dv + (long long)j * a.ld_dv + hc, C, lane);
}

// ---- rows too long for register fragments (a scalar dim_head above 512, any dim_head above 2048) ------------------------------
// The same three walks with one wave per workgroup: the rows are streamed (lane l owns columns l, l + 64, ...), the running rows
// live in LDS (each lane reads and writes its own columns only: no barrier).  Coverage, not speed.
__device__ __forceinline__ float row_dot(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ e, int C,
                                         int lane) {  // sum_c x[c] (y[c] + e[c]) over this lane's columns
  float d = 0.f;
  for (int c = lane; c < C; c += 64) d = fmaf(ldg1(x + c), ldg1(y + c) + (e != nullptr ? ldg1(e + c) : 0.f), d);
  return d;
}

__global__ __launch_bounds__(64) void attn_fwd_long_kernel(AttnArgs a) {
  __shared__ float acc[kMaxRow], macc[kMaxRow];
  const int lane = threadIdx.x, C = a.C;
  const int i = a.mean ? (int)blockIdx.x : (int)(blockIdx.x / a.heads);
  const int h0 = a.mean ? 0 : (int)(blockIdx.x % a.heads), hn = a.mean ? a.heads : 1;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const long long planes = (long long)a.n_dst * a.heads;
  for (int c = lane; c < C; c += 64) macc[c] = 0.f;
  for (int hh = 0; hh < hn; ++hh) {
    const int h = h0 + hh;
    const long long hc = (long long)h * C;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    for (int c = lane; c < C; c += 64) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = e0; t < e1; ++t) {
      const int j = ldgi(a.src + t);
      const float* er = a.e != nullptr ? a.e + (a.perm != nullptr ? a.perm[t] : (long long)t) * a.ld_e + hc : nullptr;
      const float* vr = a.v + (long long)j * a.ld_v + hc;
      const float s = wave_sum(row_dot(qr, a.k + (long long)j * a.ld_k + hc, er, C, lane)) / a.sqrt_c;
      const float mn = fmaxf(m, s), sc = expf(m - mn), p = expf(s - mn);
      l = l * sc + p;
      for (int c = lane; c < C; c += 64) acc[c] = fmaf(p, ldg1(vr + c) + (er != nullptr ? ldg1(er + c) : 0.f), acc[c] * sc);
      m = mn;
    }
    const bool any = e1 > e0;
    if (lane == 0) {
      a.lse[(long long)i * a.heads + h] = any ? m : 0.f;
      a.lse[planes + (long long)i * a.heads + h] = any ? logf(l) : 0.f;
    }
    for (int c = lane; c < C; c += 64) {
      const float o = any ? acc[c] / l : 0.f;
      if (a.mean) {
        macc[c] += o;
        if (a.out_heads != nullptr) stg1(a.out_heads + (long long)i * a.ld_oh + hc + c, o);
      } else {
        stg1(a.out + (long long)i * a.ld_out + hc + c, o);
      }
    }
  }
  if (a.mean)
    for (int c = lane; c < C; c += 64) stg1(a.out + (long long)i * a.ld_out + c, macc[c] / (float)a.heads);
}

__global__ __launch_bounds__(64) void attn_bwd_dst_long_kernel(AttnArgs a) {
  __shared__ float acc[kMaxRow];
  const int lane = threadIdx.x, C = a.C;
  const long long item = blockIdx.x;
  const int i = (int)(item / a.heads), h = (int)(item % a.heads);
  const long long hc = (long long)h * C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const float* qr = a.q + (long long)i * a.ld_q + hc;
  const float* gr = a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc);
  const float hdiv = a.mean ? (float)a.heads : 1.f;  // (x / 1 is x)
  float d = 0.f;
  for (int c = lane; c < C; c += 64) d = fmaf(ldg1(gr + c) / hdiv, ldg1(a.out_heads + (long long)i * a.ld_oh + hc + c), d);
  const float delta = wave_sum(d);
  if (lane == 0) a.delta[item] = delta;
  const float m = a.lse[item], ll = a.lse[(long long)a.n_dst * a.heads + item];
  for (int c = lane; c < C; c += 64) acc[c] = 0.f;
  for (int t = e0; t < e1; ++t) {
    const int j = ldgi(a.src + t);
    const long long eid = a.perm != nullptr ? a.perm[t] : (long long)t;
    const float* er = a.e != nullptr ? a.e + eid * a.ld_e + hc : nullptr;
    const float* kr = a.k + (long long)j * a.ld_k + hc;
    const float s = wave_sum(row_dot(qr, kr, er, C, lane)) / a.sqrt_c;
    const float dp = wave_sum(row_dot(gr, a.v + (long long)j * a.ld_v + hc, er, C, lane)) / hdiv;
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    for (int c = lane; c < C; c += 64) {
      acc[c] = fmaf(g, ldg1(kr + c) + (er != nullptr ? ldg1(er + c) : 0.f), acc[c]);
      if (a.de != nullptr) stg1(a.de + eid * a.ld_de + hc + c, fmaf(p, ldg1(gr + c) / hdiv, g * ldg1(qr + c)));
    }
  }
  for (int c = lane; c < C; c += 64) stg1(a.dq + (long long)i * a.ld_dq + hc + c, acc[c]);
}

__global__ __launch_bounds__(64) void attn_bwd_src_long_kernel(AttnArgs a) {
  __shared__ float acck[kMaxRow], accv[kMaxRow];
  const int lane = threadIdx.x, C = a.C;
  const long long item = blockIdx.x;
  const int j = (int)(item / a.heads), h = (int)(item % a.heads);
  const long long hc = (long long)h * C, planes = (long long)a.n_dst * a.heads;
  const int s0 = ldgi(a.src_ptr + j), s1 = ldgi(a.src_ptr + j + 1);
  const float* kr = a.k + (long long)j * a.ld_k + hc;
  const float* vr = a.v + (long long)j * a.ld_v + hc;
  const float hdiv = a.mean ? (float)a.heads : 1.f;
  for (int c = lane; c < C; c += 64) acck[c] = 0.f, accv[c] = 0.f;
  for (int t = s0; t < s1; ++t) {
    const int pos = ldgi(a.src_pos + t);
    const int i = ldgi(a.dst + pos);
    const float* er = a.e != nullptr ? a.e + (a.perm != nullptr ? a.perm[pos] : (long long)pos) * a.ld_e + hc : nullptr;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    const float* gr = a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc);
    const long long ih = (long long)i * a.heads + h;
    const float m = a.lse[ih], ll = a.lse[planes + ih], delta = a.delta[ih];
    const float s = wave_sum(row_dot(qr, kr, er, C, lane)) / a.sqrt_c;
    const float dp = wave_sum(row_dot(gr, vr, er, C, lane)) / hdiv;
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    for (int c = lane; c < C; c += 64) {
      acck[c] = fmaf(g, ldg1(qr + c), acck[c]);
      accv[c] = fmaf(p, ldg1(gr + c) / hdiv, accv[c]);
    }
  }
  for (int c = lane; c < C; c += 64) {
    stg1(a.dk + (long long)j * a.ld_dk + hc + c, acck[c]);
    stg1(a.dv + (long long)j * a.ld_dv + hc + c, accv[c]);
  }
}

// fragment variants: 0..3 VEC with dim_head <= 256 / 512 / 1024 / 2048, 4..5 scalar with dim_head <= 128 / 512, 6 the long-row kernels
int attn_variant(int C, bool vec) {
  if (vec && C <= 2048) return C <= 256 ? 0 : C <= 512 ? 1 : C <= 1024 ? 2 : 3;
  return C <= 128 ? 4 : C <= 512 ? 5 : 6;
}

#define GW_GC_VARIANTS(X, LONG) \
  switch (variant) {            \
    case 0: X(4, true, 4); break;    \
    case 1: X(8, true, 4); break;    \
    case 2: X(16, true, 2); break;   \
    case 3: X(32, true, 1); break;   \
    case 4: X(2, false, 4); break;   \
    case 5: X(8, false, 2); break;   \
    default: LONG; break;            \
  }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- activations ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float act_f(float z, int act) {
  if (act == GW_ACT_RELU) return z > 0.f ? z : 0.f;
  if (act == GW_ACT_SILU) return z * sigmoidf_(z);
  return z;
}
__device__ __forceinline__ float act_d(float z, int act) {
  if (act == GW_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == GW_ACT_SILU) {
    const float sg = sigmoidf_(z);
    return sg * (1.f + z * (1.f - sg));
  }
  return 1.f;
}

// ---- ConditionalLayerNorm: one wave per row, four rows per workgroup ------------------------------------------------------------
__device__ __forceinline__ void row_stats(const float* __restrict__ xr, int width, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = lane; c < width; c += 64) s += ldg1(xr + c);
  mean = wave_sum(s) / (float)width;
  float v = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float d = ldg1(xr + c) - mean;
    v = fmaf(d, d, v);
  }
  rstd = 1.0f / sqrtf(wave_sum(v) / (float)width + 1e-5f);
}

__global__ __launch_bounds__(256) void cln_fwd_kernel(long long rows, int width, int act, const float* __restrict__ x, long long ld_x,
                                                      const float* __restrict__ scale, long long ld_s, const float* __restrict__ bias,
                                                      long long ld_b, float* __restrict__ out, long long ld_o) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd;
    stg1(out + r * ld_o + c, act_f(ldg1(scale + r * ld_s + c) * xh + ldg1(bias + r * ld_b + c), act));
  }
}

__global__ __launch_bounds__(256) void cln_bwd_kernel(long long rows, int width, int act, const float* __restrict__ x, long long ld_x,
                                                      const float* __restrict__ scale, long long ld_s, const float* __restrict__ bias,
                                                      long long ld_b, const float* __restrict__ dout, long long ld_do,
                                                      float* __restrict__ dx, long long ld_dx, float* __restrict__ dscale,
                                                      float* __restrict__ dbias, long long ld_dsb) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  float sa = 0.f, sb = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd, sc = ldg1(scale + r * ld_s + c);
    const float dz = ldg1(dout + r * ld_do + c) * act_d(sc * xh + ldg1(bias + r * ld_b + c), act);
    if (dscale != nullptr) stg1(dscale + r * ld_dsb + c, dz * xh);
    if (dbias != nullptr) stg1(dbias + r * ld_dsb + c, dz);
    const float g = dz * sc;
    sa += g;
    sb = fmaf(g, xh, sb);
  }
  if (dx == nullptr) return;
  sa = wave_sum(sa) / (float)width;
  sb = wave_sum(sb) / (float)width;
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd, sc = ldg1(scale + r * ld_s + c);
    const float g = ldg1(dout + r * ld_do + c) * act_d(sc * xh + ldg1(bias + r * ld_b + c), act) * sc;
    stg1(dx + r * ld_dx + c, rstd * (g - sa - xh * sb));
  }
}

// ---- beta gate ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_fwd_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                       const float* __restrict__ xr, long long ld_x, const float* __restrict__ w,
                                                       float* __restrict__ y, long long ld_y, float* __restrict__ gate) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float t = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    t = fmaf(ldg1(w + c), ov, t);
    t = fmaf(ldg1(w + width + c), xv, t);
    t = fmaf(ldg1(w + 2 * width + c), ov - xv, t);
  }
  const float g = sigmoidf_(wave_sum(t));
  for (int c = lane; c < width; c += 64) {
    const float ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    stg1(y + r * ld_y + c, g * xv + (1.f - g) * ov);
  }
  if (lane == 0) gate[r] = g;
}

__global__ __launch_bounds__(256) void gate_bwd_rows_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                            const float* __restrict__ xr, long long ld_x, const float* __restrict__ w,
                                                            const float* __restrict__ gate, const float* __restrict__ dy,
                                                            long long ld_dy, float* __restrict__ d_o, float* __restrict__ d_x,
                                                            long long ld_d, float* __restrict__ dt) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s = 0.f;
  for (int c = lane; c < width; c += 64)
    s = fmaf(ldg1(dy + r * ld_dy + c), ldg1(xr + r * ld_x + c) - ldg1(o + r * ld_o + c), s);
  const float g = gate[r];
  const float d = wave_sum(s) * g * (1.f - g);
  for (int c = lane; c < width; c += 64) {
    const float dv = ldg1(dy + r * ld_dy + c), wc = ldg1(w + 2 * width + c);
    if (d_o != nullptr) stg1(d_o + r * ld_d + c, dv * (1.f - g) + d * (ldg1(w + c) + wc));
    if (d_x != nullptr) stg1(d_x + r * ld_d + c, dv * g + d * (ldg1(w + width + c) - wc));
  }
  if (lane == 0) dt[r] = d;
}

// part[slab][3][width]: one thread per column walks the slab's rows in order
__global__ __launch_bounds__(256) void gate_cols_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                        const float* __restrict__ xr, long long ld_x, const float* __restrict__ dt,
                                                        float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const long long r0 = (long long)blockIdx.y * kGateSlab, r1 = r0 + kGateSlab < rows ? r0 + kGateSlab : rows;
  double a = 0.0, b = 0.0, d = 0.0;  // fp64: a chain of 256 fp32 additions would cost more than a pairwise float32 sum
  for (long long r = r0; r < r1; ++r) {
    const float t = dt[r], ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    a += (double)(t * ov);
    b += (double)(t * xv);
    d += (double)(t * (ov - xv));
  }
  float* p = part + (long long)blockIdx.y * 3 * width;
  p[c] = (float)a;
  p[width + c] = (float)b;
  p[2 * width + c] = (float)d;
}

__global__ __launch_bounds__(256) void gate_sum_kernel(int slabs, int n, const float* __restrict__ part, float* __restrict__ dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int sl = 0; sl < slabs; ++sl) s += (double)ldg1(part + (long long)sl * n + e);
  dw[e] = (float)s;
}

bool gate_ok(int64_t rows, int width) {
  return rows >= 0 && width >= 1 && width <= (1 << 20) && (rows + kGateSlab - 1) / kGateSlab <= 65535;
}
size_t gate_bytes(int64_t rows, int width) {
  return ((size_t)rows + (size_t)((rows + kGateSlab - 1) / kGateSlab) * 3 * (size_t)width) * sizeof(float);
}

// ---- SiLU, Fourier features -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void silu_fwd_kernel(long long n, const float* __restrict__ x, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = act_f(x[i], GW_ACT_SILU);
}
__global__ __launch_bounds__(256) void silu_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    dx[i] = dy[i] * act_d(x[i], GW_ACT_SILU);
}

// f_i = exp(-ln(base_period) i / F) in float32, operation by operation as modules.py:184-188 forms it
__device__ __forceinline__ float fourier_freq(int i, int F, float neg_log_base) { return expf(neg_log_base * (float)i / (float)F); }

__global__ __launch_bounds__(256) void fourier_fwd_kernel(long long rows, int F, float neg_log_base, const float* __restrict__ t,
                                                          float* __restrict__ out, long long ld_o) {
  const long long n = rows * F;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const long long r = idx / F;
    const int i = (int)(idx - r * F);
    const float arg = t[r] * fourier_freq(i, F, neg_log_base);
    out[r * ld_o + i] = cosf(arg);
    out[r * ld_o + F + i] = sinf(arg);
  }
}

__global__ __launch_bounds__(256) void fourier_bwd_kernel(long long rows, int F, float neg_log_base, const float* __restrict__ t,
                                                          const float* __restrict__ dout, long long ld_do, float* __restrict__ dt) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float tv = t[r];
  float s = 0.f;
  for (int i = lane; i < F; i += 64) {
    const float f = fourier_freq(i, F, neg_log_base), arg = tv * f;
    s += f * (cosf(arg) * ldg1(dout + r * ld_do + F + i) - sinf(arg) * ldg1(dout + r * ld_do + i));
  }
  s = wave_sum(s);
  if (lane == 0) dt[r] = s;
}

int attn_check(const char* bad, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head) {
  if (n_dst < 0 || n_src < 0 || n_edges < 0 || heads < 1 || dim_head < 1) return failf(GW_E_BADARG, bad);
  if ((int64_t)heads * dim_head > kMaxRow) return failf(GW_E_UNSUPPORTED, "graph attention: heads * dim_head must be at most 4096");
  if ((int64_t)n_dst * heads >= ((int64_t)1 << 31) || (int64_t)n_src * heads >= ((int64_t)1 << 31)) return failf(GW_E_BADARG, bad);
  return GW_OK;
}

}  // namespace

extern "C" {

int gw_graph_attention_forward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                               const int32_t* src, const int64_t* perm, const float* q, int32_t ld_q, const float* k, int32_t ld_k,
                               const float* v, int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, float* out, int32_t ld_out,
                               float* out_heads, int32_t ld_out_heads, float* lse, void* stream) {
  const char* bad = "gw_graph_attention_forward: bad arguments";
  if (int rc = attn_check(bad, n_dst, n_src, n_edges, heads, dim_head)) return rc;
  if (n_dst == 0 || n_edges == 0) return GW_OK;
  const int hc = heads * dim_head;
  if (!dst_ptr || !src || !q || !k || !v || !out || !lse || n_src < 1 || ld_q < hc || ld_k < hc || ld_v < hc || (e && ld_e < hc) ||
      ld_out < (mean ? dim_head : hc) || (out_heads && ld_out_heads < hc))
    return failf(GW_E_BADARG, bad);
  const bool vec = dim_head % 4 == 0 && ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && (!e || ld_e % 4 == 0) &&
                   (!out_heads || ld_out_heads % 4 == 0) && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(e) &&
                   aligned16(out) && aligned16(out_heads);
  AttnArgs a = {};
  a.n_dst = n_dst, a.n_src = n_src, a.heads = heads, a.C = dim_head, a.mean = mean ? 1 : 0;
  a.dst_ptr = dst_ptr, a.src = src, a.perm = (const long long*)perm;
  a.q = q, a.k = k, a.v = v, a.e = e, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v, a.ld_e = ld_e;
  a.out = out, a.ld_out = ld_out, a.out_heads = mean ? out_heads : nullptr, a.ld_oh = ld_out_heads, a.lse = lse;
  a.sqrt_c = sqrtf((float)dim_head);
  const int64_t items = mean ? (int64_t)n_dst : (int64_t)n_dst * heads;
  const unsigned grid = (unsigned)((items + 3) / 4);
  const int variant = attn_variant(dim_head, vec);
#define GW_GC_FWD(NE, VEC, U) hipLaunchKernelGGL((attn_fwd_kernel<NE, VEC, U>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_FWD, hipLaunchKernelGGL(attn_fwd_long_kernel, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, a))
#undef GW_GC_FWD
  return check_launch("attn_fwd_kernel launch");
}

int gw_graph_attention_backward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                                const int32_t* src, const int32_t* dst, const int64_t* perm, const int32_t* src_pos,
                                const int32_t* src_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v,
                                int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, const float* out_heads, int32_t ld_out_heads,
                                const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq, int32_t ld_dq, float* dk,
                                int32_t ld_dk, float* dv, int32_t ld_dv, float* de, int32_t ld_de, void* stream) {
  const char* bad = "gw_graph_attention_backward: bad arguments";
  if (int rc = attn_check(bad, n_dst, n_src, n_edges, heads, dim_head)) return rc;
  if (n_edges == 0 || n_dst == 0 || n_src == 0) return GW_OK;
  const int hc = heads * dim_head;
  if (!dst_ptr || !src || !dst || !src_pos || !src_ptr || !q || !k || !v || !out_heads || !dout || !lse || !delta || !dq || !dk || !dv ||
      (de && !e) || ld_q < hc || ld_k < hc || ld_v < hc || (e && ld_e < hc) || ld_out_heads < hc || ld_dout < (mean ? dim_head : hc) ||
      ld_dq < hc || ld_dk < hc || ld_dv < hc || (de && ld_de < hc))
    return failf(GW_E_BADARG, bad);
  const bool vec = dim_head % 4 == 0 && ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && (!e || ld_e % 4 == 0) && ld_out_heads % 4 == 0 &&
                   ld_dout % 4 == 0 && ld_dq % 4 == 0 && ld_dk % 4 == 0 && ld_dv % 4 == 0 && (!de || ld_de % 4 == 0) && aligned16(q) &&
                   aligned16(k) && aligned16(v) && aligned16(e) && aligned16(out_heads) && aligned16(dout) && aligned16(dq) &&
                   aligned16(dk) && aligned16(dv) && aligned16(de);
  AttnArgs a = {};
  a.n_dst = n_dst, a.n_src = n_src, a.heads = heads, a.C = dim_head, a.mean = mean ? 1 : 0;
  a.dst_ptr = dst_ptr, a.src = src, a.dst = dst, a.perm = (const long long*)perm, a.src_pos = src_pos, a.src_ptr = src_ptr;
  a.q = q, a.k = k, a.v = v, a.e = e, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v, a.ld_e = ld_e;
  a.out_heads = const_cast<float*>(out_heads), a.ld_oh = ld_out_heads, a.lse = const_cast<float*>(lse);
  a.dout = dout, a.ld_dout = ld_dout, a.delta = delta;
  a.dq = dq, a.dk = dk, a.dv = dv, a.de = de, a.ld_dq = ld_dq, a.ld_dk = ld_dk, a.ld_dv = ld_dv, a.ld_de = ld_de;
  a.sqrt_c = sqrtf((float)dim_head);
  const int variant = attn_variant(dim_head, vec);
  const unsigned grid_d = (unsigned)(((int64_t)n_dst * heads + 3) / 4), grid_s = (unsigned)(((int64_t)n_src * heads + 3) / 4);
#define GW_GC_BWD_DST(NE, VEC, U) hipLaunchKernelGGL((attn_bwd_dst_kernel<NE, VEC>), dim3(grid_d), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_BWD_DST, hipLaunchKernelGGL(attn_bwd_dst_long_kernel, dim3((unsigned)((int64_t)n_dst * heads)), dim3(64), 0,
                                                   (hipStream_t)stream, a))
#undef GW_GC_BWD_DST
  if (int rc = check_launch("attn_bwd_dst_kernel launch")) return rc;
#define GW_GC_BWD_SRC(NE, VEC, U) hipLaunchKernelGGL((attn_bwd_src_kernel<NE, VEC>), dim3(grid_s), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_BWD_SRC, hipLaunchKernelGGL(attn_bwd_src_long_kernel, dim3((unsigned)((int64_t)n_src * heads)), dim3(64), 0,
                                                   (hipStream_t)stream, a))
#undef GW_GC_BWD_SRC
  return check_launch("attn_bwd_src_kernel launch");
}

int gw_cond_layernorm_forward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale, int32_t ld_scale,
                              const float* bias, int32_t ld_bias, float* out, int32_t ld_out, void* stream) {
  if (!x || !scale || !bias || !out || rows < 0 || rows >= ((int64_t)1 << 33) || width < 1 || act < GW_ACT_NONE || act > GW_ACT_SILU ||
      ld_x < width || ld_scale < width || ld_bias < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_cond_layernorm_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width,
                     (int)act, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, out, (long long)ld_out);
  return check_launch("cln_fwd_kernel launch");
}

int gw_cond_layernorm_backward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale,
                               int32_t ld_scale, const float* bias, int32_t ld_bias, const float* dout, int32_t ld_dout, float* dx,
                               int32_t ld_dx, float* dscale, float* dbias, int32_t ld_dsb, void* stream) {
  if (!x || !scale || !bias || !dout || (!dx && !dscale && !dbias) || rows < 0 || rows >= ((int64_t)1 << 33) || width < 1 ||
      act < GW_ACT_NONE || act > GW_ACT_SILU || ld_x < width || ld_scale < width || ld_bias < width || ld_dout < width ||
      (dx && ld_dx < width) || ((dscale || dbias) && ld_dsb < width))
    return failf(GW_E_BADARG, "gw_cond_layernorm_backward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width,
                     (int)act, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, dout, (long long)ld_dout, dx,
                     (long long)ld_dx, dscale, dbias, (long long)ld_dsb);
  return check_launch("cln_bwd_kernel launch");
}

int gw_beta_gate_forward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                         float* y, int32_t ld_y, float* gate, void* stream) {
  if (!out || !x_r || !w || !y || !gate || !gate_ok(rows, width) || ld_out < width || ld_xr < width || ld_y < width)
    return failf(GW_E_BADARG, "gw_beta_gate_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(gate_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width, out,
                     (long long)ld_out, x_r, (long long)ld_xr, w, y, (long long)ld_y, gate);
  return check_launch("gate_fwd_kernel launch");
}

size_t gw_beta_gate_workspace_bytes(int64_t rows, int32_t width) {
  if (!gate_ok(rows, width) || rows < 1) {
    failf(GW_E_BADARG, "gw_beta_gate_workspace_bytes: bad arguments");
    return 0;
  }
  return gate_bytes(rows, width);
}

int gw_beta_gate_backward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                          const float* gate, const float* dy, int32_t ld_dy, void* workspace, size_t workspace_bytes, float* d_out,
                          float* d_xr, int32_t ld_d, float* dw, void* stream) {
  const char* bad = "gw_beta_gate_backward: bad arguments";
  if (!out || !x_r || !w || !gate || !dy || !workspace || !dw || !gate_ok(rows, width) || ld_out < width || ld_xr < width ||
      ld_dy < width || ((d_out || d_xr) && ld_d < width))
    return failf(GW_E_BADARG, bad);
  if (rows == 0) return GW_OK;
  if (workspace_bytes < gate_bytes(rows, width)) return failf(GW_E_BADARG, "gw_beta_gate_backward: bad arguments (workspace)");
  float* dt = (float*)workspace;
  float* part = dt + rows;
  const int slabs = (int)((rows + kGateSlab - 1) / kGateSlab);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gate_bwd_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (long long)rows, (int)width, out,
                     (long long)ld_out, x_r, (long long)ld_xr, w, gate, dy, (long long)ld_dy, d_out, d_xr, (long long)ld_d, dt);
  if (int rc = check_launch("gate_bwd_rows_kernel launch")) return rc;
  hipLaunchKernelGGL(gate_cols_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)slabs), dim3(256), 0, st, (long long)rows,
                     (int)width, out, (long long)ld_out, x_r, (long long)ld_xr, (const float*)dt, part);
  if (int rc = check_launch("gate_cols_kernel launch")) return rc;
  hipLaunchKernelGGL(gate_sum_kernel, dim3((unsigned)((3 * width + 255) / 256)), dim3(256), 0, st, slabs, 3 * (int)width, (const float*)part,
                     dw);
  return check_launch("gate_sum_kernel launch");
}

int gw_silu_forward(int64_t n, const float* x, float* y, void* stream) {
  if (!x || !y || n < 0) return failf(GW_E_BADARG, "gw_silu_forward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(silu_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long long)n, x, y);
  return check_launch("silu_fwd_kernel launch");
}

int gw_silu_backward(int64_t n, const float* x, const float* dy, float* dx, void* stream) {
  if (!x || !dy || !dx || n < 0) return failf(GW_E_BADARG, "gw_silu_backward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long long)n, x, dy, dx);
  return check_launch("silu_bwd_kernel launch");
}

int gw_fourier_forward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, float* out, int32_t ld_out, void* stream) {
  if (!t || !out || rows < 0 || num_frequencies < 1 || !(base_period > 0.f) || ld_out < 2 * num_frequencies)
    return failf(GW_E_BADARG, "gw_fourier_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(fourier_fwd_kernel, dim3(grid_for(rows * num_frequencies)), dim3(256), 0, (hipStream_t)stream, (long long)rows,
                     (int)num_frequencies, (float)(-log((double)base_period)), t, out, (long long)ld_out);
  return check_launch("fourier_fwd_kernel launch");
}

int gw_fourier_backward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, const float* dout, int32_t ld_dout,
                        float* dt, void* stream) {
  if (!t || !dout || !dt || rows < 0 || rows >= ((int64_t)1 << 33) || num_frequencies < 1 || !(base_period > 0.f) ||
      ld_dout < 2 * num_frequencies)
    return failf(GW_E_BADARG, "gw_fourier_backward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(fourier_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows,
                     (int)num_frequencies, (float)(-log((double)base_period)), t, dout, (long long)ld_dout, dt);
  return check_launch("fourier_bwd_kernel launch");
}

}  // extern "C"
